#!/usr/bin/env python3
"""The correlator (include/dcs_correlator.h) on an MI355X: the visibilities of every antenna pair of a noise-free tone that
arrives at every antenna with a known phase, three visibilities of ``blocks`` 16-sample blocks each, integrated into one.

    python examples/correlator.py [ant chan blocks]

The checks at the end: the argument of every V[a][b] is the phase difference of a and b to within what the 8-bit
quantisation of the samples allows; the autocorrelations, summed over the antennas, are exactly the incoherent beam's power
of the same blocks (include/dcs_incoherent_beam.h); and the integrated visibilities are the exact sums, rounded once."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, block_visibilities_bytes, incoherent_block_power_bytes,  # noqa: E402
                                   nr_baselines, visibilities_bytes)

A, C, N = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 16, 8)
NR_VIS = 3
NBLK = N * NR_VIS
NT = 16 * NBLK
AMPLITUDE = 100.0                                             # of the unit tone in int8 steps
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=NT)
gen = SteeringCoefficientGenerator(p)                         # no delay table: the correlator has no coefficients

# x_a[t] = exp(i (phase_a + omega_c t)), quantised to int8 [C][NT / 16][A][16][{re, im}]
rng = np.random.default_rng(2)
phase = rng.uniform(-np.pi, np.pi, A)
omega = 2 * np.pi * (0.013 + 0.007 * np.arange(C))
arg = phase[None, None, :] + omega[:, None, None] * np.arange(NT)[None, :, None]                # [C][NT][A]
tone = AMPLITUDE * np.stack([np.cos(arg), np.sin(arg)], axis=-1)                                # [C][NT][A][2]
samples = np.rint(tone).astype(np.int8).reshape(C, NBLK, 16, A, 2).transpose(0, 1, 3, 2, 4).copy()

NB = nr_baselines(A)
vbytes, obytes = block_visibilities_bytes(p, NT, N), visibilities_bytes(p, NR_VIS, NR_VIS)
pbytes = incoherent_block_power_bytes(p, NT)
d_ant, d_vis, d_out, d_power = mem_alloc(samples.nbytes), mem_alloc(vbytes), mem_alloc(obytes), mem_alloc(pbytes)
memcpy_htod(d_ant, samples)
gen.correlate_block(d_ant, samples.nbytes, d_vis, vbytes, NT, N)
gen.integrate_visibilities(d_vis, vbytes, NR_VIS, NR_VIS, d_out, obytes)
gen.incoherent_block_power(d_ant, samples.nbytes, d_power, pbytes, NT)
synchronize()
vis = np.empty((C, NR_VIS, NB, 2), np.int32)
out = np.empty((1, C, NB, 2), np.float32)
power = np.empty((C, NBLK), np.uint32)
memcpy_dtoh(vis, d_vis)
memcpy_dtoh(out, d_out)
memcpy_dtoh(power, d_power)

# 1. arg V[a][b] = phase_a - phase_b.  A quantised sample is off by at most sqrt(1/2) in the plane, so a product x_a conj(x_b)
#    is off by at most e (|x_b| + |x_a| + e) with e = sqrt(1/2) and |x| = AMPLITUDE, and so is their mean: the angle between
#    it and the true product of length AMPLITUDE^2 is at most asin of the ratio
a, b = np.tril_indices(A)
e = np.sqrt(0.5)
bound = np.arcsin(e * (2 * AMPLITUDE + e) / AMPLITUDE ** 2)
got = np.arctan2(vis[..., 1].astype(np.float64), vis[..., 0].astype(np.float64))                # [C][NR_VIS][NB]
err = np.angle(np.exp(1j * (got - (phase[a] - phase[b])[None, None, :])))
print(f"{A} ant ({NB} baselines) x {C} chan, {NR_VIS} visibilities of {16 * N} samples: "
      f"largest phase error {np.abs(err).max():.5f} rad (bound {bound:.5f})")
ok = bool(np.abs(err).max() <= bound)

# 2. the autocorrelations (the last of every row of the triangle) against the incoherent beam, exactly
autos = vis[:, :, a == b, 0].astype(np.int64).sum(axis=2)                                        # [C][NR_VIS]
incoherent = power.astype(np.int64).reshape(C, NR_VIS, N).sum(axis=2)
ok &= bool(np.array_equal(autos, incoherent)) and not vis[:, :, a == b, 1].any()

# 3. the integration: the exact sum of the three visibilities, rounded once (below 2^53 a double holds it exactly)
S = vis.astype(np.int64).sum(axis=1)[None]
ok &= bool(np.array_equal(S.astype(np.float64).astype(np.float32).view(np.uint32), out.view(np.uint32)))
gen.close()
print("OK" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
