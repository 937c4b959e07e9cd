#!/usr/bin/env python3
"""Full-Stokes search filterbanks from a dual-polarisation array (include/dcs_stokes.h) on an MI355X: one context, the
antenna tensors of polarisations X and Y, two 8-bit tied-array beamformer calls with the same coefficients and the same
per-beam gains (include/dcs_beam_complex_quant.h), the exact block Stokes parameters I, Q, U, V of the two int8 beam
tensors, their integration into spectra, and the 8-bit filterbanks of include/dcs_filterbank.h over 4 B series.

    python examples/dual_pol_stokes.py [ant beams chan]

The check at the end restates the Stokes contract in numpy integers on the very int8 beams the beamformer wrote: it is exact,
so it must agree bit for bit."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, block_stokes_bytes, filterbank_bytes,  # noqa: E402
                                   filterbank_scales_bytes, quantised_beams_bytes, simulate_input, spectra_sums_bytes,
                                   stokes_spectra_bytes)

A, B, C = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 16, 64)
NT, N, NS = 256, 2, 4                                         # samples per call; blocks per spectrum; I, Q, U, V
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=NT)
gen = SteeringCoefficientGenerator(p)
gen.upload_delays(simulate_input(p))

nblk, T, NB = NT // 16, NT // 16 // N, NS * B                 # spectra per call; filterbank series
qbytes = quantised_beams_bytes(p, NT)
bsbytes, spbytes = block_stokes_bytes(p, NT, NS), stokes_spectra_bytes(p, nblk, N, NS)
sumbytes, scbytes, fbbytes = spectra_sums_bytes(p, NB), filterbank_scales_bytes(p, NB), filterbank_bytes(p, NB, T)
rng = np.random.default_rng(2)
ant = {pol: rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8) for pol in "xy"}
ant["y"][..., 1] >>= 1                                       # polarisation y a little weaker: Q > 0 on average
d_ant = {pol: mem_alloc(a.nbytes) for pol, a in ant.items()}
d_q = {pol: mem_alloc(qbytes) for pol in "xy"}
d_gains, d_block, d_spectra = mem_alloc(B * 4), mem_alloc(bsbytes), mem_alloc(spbytes)
d_sums, d_scales, d_fb = mem_alloc(sumbytes), mem_alloc(scbytes), mem_alloc(fbbytes)
# the SAME gain per beam for both polarisations, or Q is biased: noise of A antennas at full scale, 4 sigma inside +-127
memcpy_htod(d_gains, np.full(B, 127.0 / (4.0 * 74.0 * np.sqrt(2.0 * A)), np.float32))
for pol in "xy":
    memcpy_htod(d_ant[pol], ant[pol])
    gen.beamform_accumulated_complex_q8(d_ant[pol], ant[pol].nbytes, d_gains, d_q[pol], qbytes, NT, t_coeff=0)
gen.stokes_block(d_q["x"], d_q["y"], qbytes, d_block, bsbytes, NT, nr_stokes=NS)
gen.integrate_stokes(d_block, bsbytes, nblk, N, NS, d_spectra, spbytes)
gen.spectra_sums(d_spectra, spbytes, T, NB, d_sums, sumbytes)
gen.filterbank_scales(d_sums, sumbytes, T, NB, 20.0, d_scales, scbytes)
gen.filterbank_q8(d_spectra, spbytes, T, NB, d_scales, 128.0, d_fb, fbbytes, T)
synchronize()
spectra = np.empty((T, C, B, NS), np.float32)                 # [time][channel][beam][Stokes]
fb = np.empty((NB, T, C), np.uint8)                           # [series][time][channel]
memcpy_dtoh(spectra, d_spectra)
memcpy_dtoh(fb, d_fb)
print(f"{A} ant x {B} beams x {C} chan, two polarisations, {N * 16} samples per spectrum, {T} spectra")
print("mean I, Q, U, V:", ", ".join(f"{spectra[..., s].mean():.6g}" for s in range(NS)))
print(f"{NB} filterbanks uint8 [{T}][{C}]: series 4 * b + s is Stokes s (0 = I, 1 = Q, 2 = U, 3 = V) of beam b; "
      f"series 0 (I of beam 0) has mean {fb[0].mean():.1f}, series 3 (V of beam 0) {fb[3].mean():.1f}")

# the contract, on the int8 beams as they are in device memory: exact integers, one rounding per spectrum
q = {pol: np.empty((C, nblk, B, 16, 2), np.int8) for pol in "xy"}
for pol in "xy":
    memcpy_dtoh(q[pol], d_q[pol])
xr, xi, yr, yi = (q[pol][..., k].astype(np.int64) for pol in "xy" for k in (0, 1))
pxx, pyy = (xr * xr + xi * xi).sum(axis=3), (yr * yr + yi * yi).sum(axis=3)
block = np.stack([pxx + pyy, pxx - pyy, 2 * (xr * yr + xi * yi).sum(axis=3), 2 * ((xi * yr).sum(axis=3) - (xr * yi).sum(axis=3))],
                 axis=-1)                                     # [C][nblk][B][4]
S = block.reshape(C, T, N, B, NS).sum(axis=2).transpose(1, 0, 2, 3)
expected = S.astype(np.float64).astype(np.float32)            # |S| < 2^53: the double is exact, so this rounds once
same = np.array_equal(expected.view(np.uint32), spectra.view(np.uint32))
print("bit-identical to the integer contract:", same)
sys.exit(0 if same else 1)
