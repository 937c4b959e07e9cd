#!/usr/bin/env python3
"""A tied-array beam on an MI355X (include/dcs_beam_complex.h): the samples of a point source in the direction of beam b0,
x_a = 100 * w_{a, b0} rounded to int8, beamformed with the complex product and ``conjugate=True``.  Beam b0 adds the
antennas coherently -- (100 A, 0), detected power 16 * (100 A)^2 per block -- while the other beams, and the element-wise
product of ``beamform_accumulated`` on every beam, do not.

    python examples/tied_array_beam.py [ant beams chan]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device  # noqa: E402
from dc_sand_amd.generator import SteeringCoefficientGenerator, block_power_bytes  # noqa: E402
from dc_sand_amd.parameters import delay_vals_dtype  # noqa: E402

A, B, C = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 16, 4)
NT, T_COEFF = 32, 0
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=NT)
rng = np.random.default_rng(0x5EED)                           # seeded delay polynomials: every beam its own direction
table = np.empty(p.n_pairs, dtype=delay_vals_dtype)           # the beamformers index it [beam * A + antenna]
table["fDelay_s"] = rng.uniform(-1e-7 / 3, 1e-7 / 3, p.n_pairs)
table["fDelayRate_sps"] = rng.uniform(-2e-6, 2e-6, p.n_pairs)
table["fPhase_rad"] = rng.uniform(-np.pi, np.pi, p.n_pairs)
table["fPhaseRate_radps"] = rng.uniform(-3e-6, 3e-6, p.n_pairs)
gen = SteeringCoefficientGenerator(p)
gen.upload_delays(table)

# the steering coefficients w[c][a][b] of that table at the coefficient time, from the generator (its table order is
# [antenna * B + beam])
coeffs = SteeringCoefficientGenerator(p)
coeffs.upload_delays(np.ascontiguousarray(table.reshape(B, A).T).ravel())
d_w = mem_alloc(coeffs.output_bytes(nt=1))
coeffs.generate(d_w, coeffs.output_bytes(nt=1), t0=T_COEFF, nt=1)
w = np.empty((C, A, B, 2), np.float32)
memcpy_dtoh(w, d_w)

b0 = B // 3
nblk = NT // 16
source = np.rint(100.0 * w[:, :, b0, :]).astype(np.int8)      # [c][a][{re, im}]: the same sample at every time
samples = np.ascontiguousarray(np.broadcast_to(source[:, None, :, None, :], (C, nblk, A, 16, 2)))
d_ant, d_beams, d_power = mem_alloc(samples.nbytes), mem_alloc(B * C * NT * 8), mem_alloc(block_power_bytes(p, NT))
memcpy_htod(d_ant, samples)


def read(d, shape):
    out = np.empty(shape, np.float32)
    memcpy_dtoh(out, d)
    return out


gen.beamform_accumulated_complex_power(d_ant, samples.nbytes, d_power, block_power_bytes(p, NT), NT, t_coeff=T_COEFF, conjugate=True)
tied = read(d_power, (C, nblk, B)).mean(axis=(0, 1))
gen.beamform_accumulated_power(d_ant, samples.nbytes, d_power, block_power_bytes(p, NT), NT, t_coeff=T_COEFF)
elementwise = read(d_power, (C, nblk, B)).mean(axis=(0, 1))
gen.beamform_accumulated_complex(d_ant, samples.nbytes, d_beams, B * C * NT * 8, NT, t_coeff=T_COEFF, conjugate=True)
v = read(d_beams, (C, nblk, B, 16, 2))[0, 0, b0, 0]

peak = 16.0 * (100.0 * A) ** 2
print(f"{A} antennas, {B} beams, {C} channels; a source in the direction of beam {b0}; coherent peak 16 (100 A)^2 = {peak:.4g}")
print(f"beam {b0}, first sample: ({v[0]:.1f}, {v[1]:.1f}); expected ({100.0 * A:.1f}, 0) within {0.7072 * A:.1f}")
print("beam   complex product (conjugate)   element-wise product      [block power / peak]")
for b in range(B):
    print(f"{b:4d}   {tied[b] / peak:27.4f}   {elementwise[b] / peak:20.4f}{'   <- the source' if b == b0 else ''}")
ok = abs(v[0] - 100.0 * A) <= 0.7072 * A + 1e-3 and abs(v[1]) <= 0.7072 * A + 1e-3 and tied[b0] > 4.0 * np.delete(tied, b0).max()
sys.exit(0 if ok else 1)
