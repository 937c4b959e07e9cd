"""Anchors the numpy model of the Stokes detection (helpers/stokes_model.py; include/dcs_stokes.h) against plain Python-int
arithmetic: the block Stokes parameters from complex(xr, xi) * conj(complex(yr, yi)) sample by sample, the int8 extremes,
the sign of V, and the integration's one rounding.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

from helpers.stokes_model import block_stokes, integrate, same_bits


def python_stokes(x, y):
    """[C][K][B][16][2] int8 twice -> nested lists [C][K][B] of (I, Q, U, V) in Python ints, from the complex product."""
    C, K, B = x.shape[:3]
    out = np.empty((C, K, B, 4), dtype=object)
    for c in range(C):
        for k in range(K):
            for b in range(B):
                pxx = pyy = cr = ci = 0
                for t in range(16):
                    xr, xi = int(x[c, k, b, t, 0]), int(x[c, k, b, t, 1])
                    yr, yi = int(y[c, k, b, t, 0]), int(y[c, k, b, t, 1])
                    p = complex(xr, xi) * complex(yr, -yi)  # exact: every part is below 2^15
                    assert p.real == int(p.real) and p.imag == int(p.imag)
                    pxx += xr * xr + xi * xi
                    pyy += yr * yr + yi * yi
                    cr += int(p.real)
                    ci += int(p.imag)
                out[c, k, b] = (pxx + pyy, pxx - pyy, 2 * cr, 2 * ci)
    return out


def filled(shape, re, im):
    a = np.empty(shape + (16, 2), dtype=np.int8)
    a[..., 0], a[..., 1] = re, im
    return a


def test_block_stokes_is_the_complex_product_sample_by_sample():
    rng = np.random.default_rng(12)
    x = rng.integers(-128, 128, size=(3, 2, 5, 16, 2), dtype=np.int8)
    y = rng.integers(-128, 128, size=(3, 2, 5, 16, 2), dtype=np.int8)
    x.reshape(-1)[0], x.reshape(-1)[-1], y.reshape(-1)[0], y.reshape(-1)[-1] = -128, 127, 127, -128
    exp = python_stokes(x, y)
    got = block_stokes(x, y, 4)
    assert got.dtype == np.int32 and got.shape == (3, 2, 5, 4)
    assert all(int(g) == e for g, e in zip(got.ravel(), exp.ravel()))
    assert len({int(v) for v in got.ravel()}) >= 100
    only_i = block_stokes(x, y, 1)
    assert only_i.shape == (3, 2, 5, 1) and np.array_equal(only_i[..., 0], got[..., 0])
    assert (got[..., 1] < 0).any() and (got[..., 2] < 0).any() and (got[..., 3] < 0).any()


def test_all_minus_128_in_both_tensors():
    x = filled((2, 1, 3), -128, -128)
    got = block_stokes(x, x.copy(), 4)
    assert np.all(got == np.array([1 << 20, 0, 1 << 20, 0]))
    assert np.all(block_stokes(x, x, 1) == 1 << 20)


def test_the_pair_that_makes_ci_extreme():
    x, y = filled((1, 2, 2), -128, 127), filled((1, 2, 2), 127, -128)
    # per sample: xi yr - xr yi = 127 * 127 - (-128)(-128); xr yr + xi yi = 2 * (-128 * 127)
    ci = 16 * (127 * 127 - 128 * 128)
    cr = 16 * 2 * (-128 * 127)
    p = 16 * (128 * 128 + 127 * 127)
    assert ci == -4080 and all(int(v) == e for v, e in zip(python_stokes(x, y)[0, 0, 0], (2 * p, 0, 2 * cr, 2 * ci)))
    assert np.all(block_stokes(x, y, 4) == np.array([2 * p, 0, 2 * cr, 2 * ci]))
    # the other way round the sign of V turns and nothing else
    assert np.all(block_stokes(y, x, 4) == np.array([2 * p, 0, 2 * cr, -2 * ci]))
    # the two products of Ci at their extremes, one at a time: sum xi yr = 16 * 2^14 with xr yi = 0, and the reverse
    assert np.all(block_stokes(filled((1, 1, 1), 0, -128), filled((1, 1, 1), -128, 0), 4)[..., 3] == 2 * 16 * (1 << 14))
    assert np.all(block_stokes(filled((1, 1, 1), -128, 0), filled((1, 1, 1), 0, -128), 4)[..., 3] == -2 * 16 * (1 << 14))


def test_the_sign_of_v():
    x, y = filled((1, 1, 1), 0, 1), filled((1, 1, 1), 1, 0)  # x = i, y = 1 in all 16 samples: V = +2 per sample
    assert block_stokes(x, y, 4).ravel().tolist() == [32, 0, 0, 32]
    assert block_stokes(y, x, 4).ravel().tolist() == [32, 0, 0, -32]


def python_integrate(block, n, prior=None):
    C, K, B, NS = block.shape
    out = np.empty((K // n, C, B, NS), dtype=np.float32)
    exact = np.empty((K // n, C, B, NS), dtype=object)
    for i in range(K // n):
        for c in range(C):
            for b in range(B):
                for s in range(NS):
                    S = sum(int(block[c, i * n + j, b, s]) for j in range(n))
                    exact[i, c, b, s] = S
                    f = np.float32(S)  # through a double that holds S exactly: one rounding
                    assert abs(Fraction(float(f)) - S) <= Fraction(abs(S), 1 << 24)  # within half an ulp of S
                    out[i, c, b, s] = f if prior is None else np.float32(prior[i, c, b, s]) + f
    return out, exact


@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_integrate_is_the_exact_sum_rounded_once(n):
    rng = np.random.default_rng(n)
    block = rng.integers(-(1 << 20), (1 << 20) + 1, size=(2, 6, 3, 4), dtype=np.int64).astype(np.int32)
    block[0, :, 0, 0] = (1 << 23) + 1 + np.arange(6) ** 2  # planted: sums beyond 2^24 that are no floats once n >= 2 ...
    block[1, :, 2, 3] = -(1 << 23) - 1 - np.arange(6) ** 2  # ... and negative ones
    exp, exact = python_integrate(block, n)
    got = integrate(block, n)
    assert got.dtype == np.float32 and same_bits(got, exp) is None
    if n >= 2:
        inexact = [abs(S) > 1 << 24 and Fraction(float(e)) != S for e, S in zip(exp.ravel(), exact.ravel())]
        assert any(inexact)
        assert any(i and S < 0 for i, S in zip(inexact, exact.ravel()))
    prior = rng.uniform(-3e7, 3e7, size=exp.shape).astype(np.float32)
    prior.reshape(-1)[:4] = [np.nan, np.inf, -np.inf, -0.0]
    exp_acc, _ = python_integrate(block, n, prior=prior)
    assert same_bits(integrate(block, n, prior=prior), exp_acc) is None


def test_integrate_rounds_ties_to_even_and_keeps_minus_zero_out():
    block = np.zeros((1, 17, 1, 1), dtype=np.int32)
    block[0, :16, 0, 0] = 1 << 20  # 2^24 ...
    block[0, 16, 0, 0] = 1  # ... + 1: a tie, to even
    assert integrate(block, 17).ravel().tolist() == [float(1 << 24)]
    block[0, 16, 0, 0] = 3  # 2^24 + 3: a tie again, up to 2^24 + 4
    assert integrate(block, 17).ravel().tolist() == [float((1 << 24) + 4)]
    zero = integrate(np.zeros((1, 2, 1, 1), np.int32), 2)
    assert not np.signbit(zero).any()  # an exact sum of 0 is +0 ...
    acc = integrate(np.zeros((1, 2, 1, 1), np.int32), 2, prior=np.full((1, 1, 1, 1), -0.0, np.float32))
    assert not np.signbit(acc).any()  # ... and -0 + +0 is +0, to nearest
