#!/usr/bin/env python3
"""Detected, time-integrated beam power (include/dcs_beam_power.h) on an MI355X: two 256-sample calls of the matrix-core
beamformer with different coefficient times, integrated into ONE spectrum per 512 samples -- the second integration
starts from the first one's sums (``accumulate``), so the coefficients are renewed inside the integration.

    python examples/detected_beams.py [ant beams chan]

The check at the end restates the contract in numpy on what the float call returns for the same samples."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, block_power_bytes, power_spectra_bytes,  # noqa: E402
                                   simulate_input)

A, B, C = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 16, 64)
NT = 256                                                      # samples per call: 16 blocks of 16
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=NT)
gen = SteeringCoefficientGenerator(p)
gen.upload_delays(simulate_input(p))

nblk = NT // 16
pbytes, sbytes = block_power_bytes(p, NT), power_spectra_bytes(p, nblk, nblk)  # one spectrum per call's worth of blocks
d_ant, d_power, d_spectrum = mem_alloc(A * C * NT * 2), mem_alloc(pbytes), mem_alloc(sbytes)
rng = np.random.default_rng(1)
calls = [(rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8), t_coeff) for t_coeff in (0, 256)]
for i, (samples, t_coeff) in enumerate(calls):
    memcpy_htod(d_ant, samples)
    gen.beamform_accumulated_power(d_ant, samples.nbytes, d_power, pbytes, NT, t_coeff=t_coeff)
    gen.integrate_block_power(d_power, pbytes, nblk, nblk, d_spectrum, sbytes, accumulate=i > 0)
synchronize()
spectrum = np.empty((1, C, B), np.float32)                    # [time][channel][beam]: 512 samples in one spectrum
memcpy_dtoh(spectrum, d_spectrum)
print(f"{A} ant x {B} beams x {C} chan: one spectrum of {len(calls) * NT} samples, mean power {spectrum.mean():.6g}, "
      f"{pbytes} bytes of block powers per call instead of {B * C * NT * 8} bytes of fp32 beams")

# the contract, on the float call's output: |v|^2 per sample, pairwise per block, the blocks in order
d_beams = mem_alloc(B * C * NT * 8)
acc = None
for samples, t_coeff in calls:
    memcpy_htod(d_ant, samples)
    gen.beamform_accumulated(d_ant, samples.nbytes, d_beams, B * C * NT * 8, NT, t_coeff=t_coeff)
    v = np.empty((C, nblk, B, 16, 2), np.float32)
    memcpy_dtoh(v, d_beams)
    s = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]).astype(np.float32)
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    for j in range(nblk):
        acc = s[:, j, :, 0] if acc is None else acc + s[:, j, :, 0]
same = np.array_equal(acc.view(np.uint32), spectrum[0].view(np.uint32))
print("bit-identical to the contract applied to the float call's beams:", same)
sys.exit(0 if same else 1)
