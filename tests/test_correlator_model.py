"""The numpy model of the correlator (tests/helpers/correlator_model.py) anchored on arithmetic that needs no numpy: Python
integers in a triple loop, enumeration for the baseline index, fractions.Fraction for the integrator's one rounding.  No GPU."""
from fractions import Fraction

import numpy as np

from helpers.correlator_model import MAX_BLOCKS, baseline, full_matrix, integrate, nr_baselines, pairs, visibilities


def seeded(C, K, A, seed):
    ant = np.random.default_rng(seed).integers(-128, 128, size=(C, K, A, 16, 2), dtype=np.int8)
    ant.reshape(-1)[0], ant.reshape(-1)[-1] = -128, 127
    return ant


def test_model_is_the_triple_loop_over_python_integers():
    A, C, n, nr_vis = 3, 2, 2, 2
    ant = seeded(C, n * nr_vis, A, seed=1)
    got = visibilities(ant, n)
    assert got.dtype == np.int32 and got.shape == (C, nr_vis, nr_baselines(A), 2)
    x = ant.tolist()
    for c in range(C):
        for v in range(nr_vis):
            k = 0
            for a in range(A):
                for b in range(a + 1):
                    re = im = 0
                    for blk in range(v * n, v * n + n):
                        for t in range(16):
                            (ra, ia), (rb, ib) = x[c][blk][a][t], x[c][blk][b][t]
                            re += ra * rb + ia * ib
                            im += ia * rb - ra * ib
                    assert got[c, v, k].tolist() == [re, im], (c, v, a, b)
                    assert baseline(a, b) == k
                    k += 1
            assert k == nr_baselines(A)
    assert np.unique(got).size >= 30


def test_baseline_index_is_the_enumeration_for_every_station_count():
    k, seen = 0, []
    for a in range(256):
        for b in range(a + 1):
            assert baseline(a, b) == k
            k += 1
        assert baseline(a, a) == k - 1  # the autocorrelation is the last of its row
        A = a + 1
        assert nr_baselines(A) == k
        seen.append(k)
    assert seen[0] == 1 and seen[-1] == 32896
    for A in (1, 2, 17, 256):
        pa, pb = pairs(A)
        assert pa.size == nr_baselines(A) and np.all(pb <= pa) and [baseline(a, b) for a, b in zip(pa[:50], pb[:50])] == list(range(min(50, pa.size)))


def test_autocorrelations_are_real_and_the_matrix_is_hermitian():
    A, n = 7, 3
    ant = seeded(2, 6, A, seed=2)
    re, im = full_matrix(ant, n)
    assert not np.diagonal(im, axis1=2, axis2=3).any()
    assert np.all(np.diagonal(re, axis1=2, axis2=3) > 0)
    # V[b][a] computed with a and b swapped is the conjugate of V[a][b]
    assert np.array_equal(re, re.transpose(0, 1, 3, 2)) and np.array_equal(im, -im.transpose(0, 1, 3, 2))
    swapped = ant[:, :, ::-1]  # antenna a' = A - 1 - a: the pair (a, b) becomes (A - 1 - a, A - 1 - b), the other triangle
    rs, is_ = full_matrix(swapped, n)
    assert np.array_equal(rs[:, :, ::-1, ::-1], re) and np.array_equal(is_[:, :, ::-1, ::-1], im)
    vis = visibilities(ant, n)
    for a in range(A):
        assert not vis[:, :, baseline(a, a), 1].any()
        for b in range(a):
            assert np.array_equal(vis[:, :, baseline(a, b), 0], re[:, :, b, a])
            assert np.array_equal(vis[:, :, baseline(a, b), 1], -im[:, :, b, a])
    assert (vis[..., 1] > 0).any() and (vis[..., 1] < 0).any() and (vis[..., 0] < 0).any()


def test_4095_blocks_is_the_most_that_cannot_wrap():
    assert MAX_BLOCKS == 4095
    largest = MAX_BLOCKS * 16 * 2 * 128 * 128
    assert largest == 2_146_959_360 < 1 << 31 and (1 << 31) - largest == 524_288
    assert (MAX_BLOCKS + 1) * 16 * 2 * 128 * 128 == 1 << 31  # one block more does not fit
    ant = np.full((1, MAX_BLOCKS, 2, 16, 2), -128, dtype=np.int8)
    vis = visibilities(ant, MAX_BLOCKS)
    assert vis.shape == (1, 1, 3, 2) and np.all(vis[..., 0] == largest) and not vis[..., 1].any()
    # the cross terms' extremes: im = +-(n * 16 * 128^2) from one product each, the other one zero
    ant = np.zeros((1, 4, 2, 16, 2), dtype=np.int8)
    ant[:, :, 1, :, 1], ant[:, :, 0, :, 0] = -128, -128  # x_1 = -128 i, x_0 = -128
    assert visibilities(ant, 4)[0, 0, baseline(1, 0)].tolist() == [0, 4 * 16 * 128 * 128]
    ant = ant[:, :, ::-1]
    assert visibilities(ant, 4)[0, 0, baseline(1, 0)].tolist() == [0, -4 * 16 * 128 * 128]


def test_integration_rounds_the_exact_sum_once():
    rng = np.random.default_rng(3)
    C, nr_vis, NB, m = 2, 6, 3, 3
    vis = rng.integers(-(1 << 31), 1 << 31, size=(C, nr_vis, NB, 2), dtype=np.int64).astype(np.int32)
    vis[0, :3, 0, 0] = [(1 << 24) + 1, 1, 1]        # 2^24 + 3: no float, and rounding the words first would lose it
    vis[1, 3:, 2, 1] = [-(1 << 30), -(1 << 30), -3]
    out = integrate(vis, m)
    assert out.dtype == np.float32 and out.shape == (nr_vis // m, C, NB, 2)
    inexact = 0
    for i in range(nr_vis // m):
        for c in range(C):
            for k in range(NB):
                for p in range(2):
                    S = sum(int(v) for v in vis[c, i * m:(i + 1) * m, k, p])
                    f = float(out[i, c, k, p])
                    lo, hi = np.nextafter(np.float32(f), np.float32(-np.inf)), np.nextafter(np.float32(f), np.float32(np.inf))
                    assert abs(Fraction(f) - S) <= min(abs(Fraction(float(lo)) - S), abs(Fraction(float(hi)) - S))
                    inexact += Fraction(f) != S
    assert inexact >= 10
    assert float(out[0, 0, 0, 0]) == float((1 << 24) + 4)  # 2^24 + 3 lies between 2^24 + 2 and 2^24 + 4: the tie goes to even
    prior = rng.uniform(-3e9, 3e9, size=out.shape).astype(np.float32)
    acc = integrate(vis, m, prior=prior)
    assert np.array_equal(acc, (prior + out).astype(np.float32)) and not np.array_equal(acc, out)
