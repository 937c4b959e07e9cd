#!/usr/bin/env python3
"""Beams of beams on an MI355X (include/dcs_beam_complex_quant.h): A antennas in B1 sub-arrays, a point source in the
direction all of them are steered at, x_a = 100 * w_a rounded to int8.

Stage 1 forms one tied-array beam per sub-array -- the complex product with ``conjugate=True``, weights that select the
sub-array's antennas -- and requantises it to int8 in the kernel's epilogue: 100 A / B1 per beam, brought back to about
100 by the beams' gains.  That int8 tensor [C][nt / 16][B1][16][{re, im}] is, as it lies in device memory, the antenna
tensor of stage 2: a second context with B1 "antennas", whose beam 0 adds the sub-array beams in phase (zero delays) and
whose other beams do not.

    python examples/hierarchical_beams.py [ant subarrays chan]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.beam_quant import BeamQuantGains  # noqa: E402
from dc_sand_amd.beam_weights import BeamWeights  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device  # noqa: E402
from dc_sand_amd.generator import SteeringCoefficientGenerator, quantised_beams_bytes  # noqa: E402
from dc_sand_amd.parameters import delay_vals_dtype  # noqa: E402

A, B1, C = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 8, 4)
B2, NT, T_COEFF = 4, 32, 0
assert A % B1 == 0 and A <= 256 and B1 % 2 == 0, "equal sub-arrays, at most 256 antennas, an even number of sub-arrays"
require_device()
set_device(0)
rng = np.random.default_rng(0x5EED)

# ---- stage 1: every sub-array beam steered in the same direction (one delay polynomial per antenna)
p1 = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B1, NR_SAMPLES_PER_CHANNEL=NT)
direction = np.empty(A, dtype=delay_vals_dtype)
direction["fDelay_s"] = rng.uniform(-1e-7 / 3, 1e-7 / 3, A)
direction["fDelayRate_sps"] = rng.uniform(-2e-6, 2e-6, A)
direction["fPhase_rad"] = rng.uniform(-np.pi, np.pi, A)
direction["fPhaseRate_radps"] = rng.uniform(-3e-6, 3e-6, A)
stage1 = SteeringCoefficientGenerator(p1)
stage1.upload_delays(np.tile(direction, B1))                  # the beamformers index the table [beam * A + antenna]
sub = BeamWeights(p1)                                         # beam s: the antennas of sub-array s
sub.host[:] = (np.arange(A)[None, :] // (A // B1) == np.arange(B1)[:, None]).astype(np.float32)
sub.upload()

# the source: the steering coefficients of that direction at the coefficient time, from the generator ([antenna * B + beam])
coeffs = SteeringCoefficientGenerator(p1)
coeffs.upload_delays(np.repeat(direction, B1))
d_w = mem_alloc(coeffs.output_bytes(nt=1))
coeffs.generate(d_w, coeffs.output_bytes(nt=1), t0=T_COEFF, nt=1)
w = np.empty((C, A, B1, 2), np.float32)
memcpy_dtoh(w, d_w)
nblk = NT // 16
source = np.rint(100.0 * w[:, :, 0, :]).astype(np.int8)       # [c][a][{re, im}]: the same sample at every time
samples = np.ascontiguousarray(np.broadcast_to(source[:, None, :, None, :], (C, nblk, A, 16, 2)))
d_ant = mem_alloc(samples.nbytes)
memcpy_htod(d_ant, samples)

gains = BeamQuantGains(p1)                                    # 100 A / B1 per sub-array beam -> about 100
for s in range(B1):
    gains.set(s, B1 / A)
gains.upload()
q1_bytes = quantised_beams_bytes(p1, NT)
d_q1 = mem_alloc(q1_bytes)
stage1.beamform_accumulated_complex_q8(d_ant, samples.nbytes, gains.device_ptr(), d_q1, q1_bytes, NT, t_coeff=T_COEFF,
                                       d_weights=sub.device_ptr(), conjugate=True, d_clip_count=gains.clip_count_ptr())
clips = gains.clip_counts()
q1 = np.empty((C, nblk, B1, 16, 2), np.int8)
memcpy_dtoh(q1, d_q1)

# ---- stage 2: B1 inputs; beam 0 has zero delays and phases (w = 1: the sum), the others random phases
p2 = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=B1, NR_BEAMS=B2, NR_SAMPLES_PER_CHANNEL=NT)
table2 = np.zeros(p2.n_pairs, dtype=delay_vals_dtype)
table2["fPhase_rad"][B1:] = rng.uniform(-np.pi, np.pi, p2.n_pairs - B1)
stage2 = SteeringCoefficientGenerator(p2)
stage2.upload_delays(table2)
d_beams = mem_alloc(B2 * C * NT * 8)
stage2.beamform_accumulated_complex(d_q1, q1_bytes, d_beams, B2 * C * NT * 8, NT, t_coeff=T_COEFF, conjugate=True)
v2 = np.empty((C, nblk, B2, 16, 2), np.float32)
memcpy_dtoh(v2, d_beams)

print(f"{A} antennas in {B1} sub-arrays of {A // B1}, {C} channels; stage 1 writes {q1_bytes} bytes (float beams: {4 * q1_bytes})")
print(f"stage 1, sub-array beams (int8), first sample of channel 0: {[tuple(int(x) for x in q1[0, 0, s, 0]) for s in range(B1)]}")
print(f"stage 1, clipped components per sub-array beam: {clips.tolist()}")
mag = np.hypot(v2[..., 0], v2[..., 1]).mean(axis=(0, 1, 3))
print(f"stage 2, beam 0, first sample: ({v2[0, 0, 0, 0, 0]:.1f}, {v2[0, 0, 0, 0, 1]:.1f}); expected about ({100.0 * B1:.1f}, 0)")
print("stage 2, mean |beam|: " + ", ".join(f"beam {b}: {mag[b]:.1f}" for b in range(B2)))
tol = 1.5 * B1  # per sub-array beam: the samples' roundings (0.7072 per antenna, scaled by B1 / A) and the quantiser's half
ok = (clips.sum() == 0 and np.all(np.abs(v2[:, :, 0, :, 0] - 100.0 * B1) <= tol) and np.all(np.abs(v2[:, :, 0, :, 1]) <= tol)
      and mag[0] > 1.5 * mag[1:].max())
sys.exit(0 if ok else 1)
