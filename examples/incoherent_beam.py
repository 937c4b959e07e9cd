#!/usr/bin/env python3
"""The incoherent beam beside the detected beams (include/dcs_incoherent_beam.h, include/dcs_beam_power.h) on an MI355X:
two 256-sample calls, each detected by the matrix-core beamformer AND summed incoherently from the same samples in device
memory, both integrated over the same runs into ONE spectrum per 512 samples (``accumulate`` on the second call).  One
antenna is flagged out of the incoherent sum by a zero weight.

    python examples/incoherent_beam.py [ant beams chan]

The check at the end restates the incoherent beam's contract in numpy integers: it is exact, so it must agree bit for bit."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, block_power_bytes, incoherent_block_power_bytes,  # noqa: E402
                                   incoherent_spectra_bytes, power_spectra_bytes, simulate_input)

A, B, C = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 16, 64)
NT = 256                                                      # samples per call: 16 blocks of 16
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=NT)
gen = SteeringCoefficientGenerator(p)
gen.upload_delays(simulate_input(p))

nblk = NT // 16
pbytes, sbytes = block_power_bytes(p, NT), power_spectra_bytes(p, nblk, nblk)
ipbytes, isbytes = incoherent_block_power_bytes(p, NT), incoherent_spectra_bytes(p, nblk, nblk)
d_ant, d_power, d_spectrum = mem_alloc(A * C * NT * 2), mem_alloc(pbytes), mem_alloc(sbytes)
d_ipower, d_ispectrum, d_flags = mem_alloc(ipbytes), mem_alloc(isbytes), mem_alloc(A * 4)
flags = np.ones(A, np.float32)                                # flags, not a taper: a value other than 0 does not scale
flags[A // 2] = 0.0                                           # one antenna out of the incoherent sum
memcpy_htod(d_flags, flags)
rng = np.random.default_rng(1)
calls = [(rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8), t_coeff) for t_coeff in (0, 256)]
for i, (samples, t_coeff) in enumerate(calls):
    memcpy_htod(d_ant, samples)
    gen.beamform_accumulated_power(d_ant, samples.nbytes, d_power, pbytes, NT, t_coeff=t_coeff)
    gen.integrate_block_power(d_power, pbytes, nblk, nblk, d_spectrum, sbytes, accumulate=i > 0)
    gen.incoherent_block_power(d_ant, samples.nbytes, d_ipower, ipbytes, NT, d_weights=d_flags)
    gen.integrate_incoherent_power(d_ipower, ipbytes, nblk, nblk, d_ispectrum, isbytes, accumulate=i > 0)
synchronize()
spectrum = np.empty((1, C, B), np.float32)                    # [time][channel][beam]
incoherent = np.empty((1, C), np.float32)                     # [time][channel]
memcpy_dtoh(spectrum, d_spectrum)
memcpy_dtoh(incoherent, d_ispectrum)
print(f"{A} ant x {B} beams x {C} chan, {len(calls) * NT} samples per spectrum: mean detected beam power {spectrum.mean():.6g}, "
      f"mean incoherent power of {int(flags.sum())} antennas {incoherent.mean():.6g}")

# the contract: exact integer sums per call, one rounding each, the second call's added to the first's
acc = None
for samples, _ in calls:
    x = samples.astype(np.int64)
    S = ((x * x).sum(axis=(3, 4)) * (flags != 0)).sum(axis=(1, 2))           # [C]: all blocks of the call
    f = S.astype(np.float64).astype(np.float32)               # S < 2^53: the double is exact, so this rounds once
    acc = f if acc is None else (acc + f).astype(np.float32)
same = np.array_equal(acc.view(np.uint32), incoherent[0].view(np.uint32))
print("bit-identical to the integer contract:", same)
sys.exit(0 if same else 1)
