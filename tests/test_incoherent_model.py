"""The numpy model of the incoherent beam (helpers/incoherent_model.py) against plain Python-int loops that follow
include/dcs_incoherent_beam.h word for word, on small tensors.  No GPU needed."""
import struct
from fractions import Fraction

import numpy as np
import pytest

from helpers import stokes_model
from helpers.incoherent_model import block_power, flags, full_range_words, integrate, same_bits, to_float


def _loop_block_power(ant, weights):
    C, K, A = ant.shape[:3]
    out = [[0] * K for _ in range(C)]
    for c in range(C):
        for k in range(K):
            for a in range(A):
                if weights is not None and float(weights[a]) == 0.0:  # +0 and -0; NaN == 0 is False
                    continue
                for t in range(16):
                    re, im = int(ant[c, k, a, t, 0]), int(ant[c, k, a, t, 1])
                    out[c][k] += re * re + im * im
    return out


def _rn_float(s):
    """The float32 nearest to the Python int s, ties to even, by exact rational arithmetic (not through a double)."""
    if s == 0:
        return np.float32(0.0)
    e = s.bit_length() - 24  # s = m * 2^e with 2^23 <= m < 2^24
    if e <= 0:
        return np.float32(s)
    m, rest = divmod(s, 1 << e)
    half = Fraction(rest, 1 << e)
    if half > Fraction(1, 2) or (half == Fraction(1, 2) and m & 1):
        m += 1
    return np.float32(struct.unpack("<f", struct.pack("<f", float(m) * 2.0 ** e))[0])


@pytest.mark.parametrize("A,C,nt", [(1, 1, 16), (3, 2, 32), (5, 3, 48), (33, 1, 16)])
def test_block_power_is_the_integer_loop(A, C, nt):
    rng = np.random.default_rng(A * 100 + C)
    ant = rng.integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    ant[0, 0, 0] = -128  # a whole block of the most negative sample
    ant[-1, -1, -1, :, 1] = -128
    specials = np.array([-0.0, np.nan, np.inf, 0.5, 0.0, -np.inf, 1.0, -3.0, 1e-45], dtype=np.float32)
    w = specials[np.arange(A) % specials.size]
    for weights in (None, w, np.ones(A, np.float32), np.zeros(A, np.float32)):
        got = block_power(ant, weights)
        assert got.dtype == np.uint32 and got.shape == (C, nt // 16)
        assert got.tolist() == _loop_block_power(ant, weights)
    assert np.array_equal(block_power(ant, None), block_power(ant, np.ones(A, np.float32)))
    assert not block_power(ant, np.zeros(A, np.float32)).any()
    assert block_power(ant[:1, :1, :1], None)[0, 0] == 16 * 2 * 128 * 128


def test_flags_are_flags_only():
    w = np.array([0.0, -0.0, 0.5, -3.0, np.nan, np.inf, -np.inf, 1e-45, 1.0], dtype=np.float32)
    assert flags(w, w.size).tolist() == [False, False, True, True, True, True, True, True, True]
    assert flags(None, 3).tolist() == [True, True, True]
    # other values do not scale: 0.5 and 2 give what 1 gives
    ant = np.random.default_rng(1).integers(-128, 128, size=(1, 2, 4, 16, 2), dtype=np.int8)
    ref = block_power(ant, np.array([1, 0, 1, 1], np.float32))
    assert np.array_equal(block_power(ant, np.array([0.5, -0.0, 2.0, np.nan], np.float32)), ref)


def test_full_scale_fits_32_bits_and_the_integration_64():
    ant = np.full((1, 40, 256, 16, 2), -128, dtype=np.int8)
    P = block_power(ant)
    assert np.all(P == 1 << 27)
    S = integrate(P, 40)
    assert S.shape == (1, 1) and float(S[0, 0]) == float(5 << 30) and 5 << 30 > 1 << 32


def test_integration_is_the_exact_sum_rounded_once():
    rng = np.random.default_rng(7)
    C, K = 3, 24
    P = rng.integers(0, (1 << 27) + 1, size=(C, K), dtype=np.int64).astype(np.uint32)
    P[0, :4] = 1 << 27
    for n in (1, 2, 3, 8, 24):
        got = integrate(P, n)
        assert got.dtype == np.float32 and got.shape == (K // n, C)
        inexact = 0
        for i in range(K // n):
            for c in range(C):
                s = sum(int(P[c, i * n + j]) for j in range(n))
                exp = _rn_float(s)
                inexact += int(exp) != s
                assert got[i, c].tobytes() == exp.tobytes(), (n, i, c, s)
        assert n == 1 or inexact > 0  # sums above 2^24 that are no floats: the rounding is exercised
        # accumulate: RN(old + RN((float)S))
        prior = rng.integers(0, 1 << 30, size=got.shape).astype(np.float32)
        acc = integrate(P, n, prior=prior)
        for i in range(K // n):
            for c in range(C):
                s = sum(int(P[c, i * n + j]) for j in range(n))
                # prior and RN((float)S) are integers below 2^31 here, so their exact sum is one, and _rn_float rounds it
                exact = int(prior[i, c]) + int(_rn_float(s))
                assert float(prior[i, c]) == int(prior[i, c])
                assert acc[i, c].tobytes() == _rn_float(exact).tobytes(), (n, i, c)
    # across two calls: the second adds its own rounded sum to the first's
    first = integrate(P[:, :12], 12)
    both = integrate(P[:, 12:], 12, prior=first)
    assert same_bits(both, (first + integrate(P[:, 12:], 12)).astype(np.float32)) is None


def test_words_with_bit_31_set_are_unsigned():
    """Full-range words: the exact sums are Python ints of the unsigned words, up to 12 (2^32 - 1).  The same bits read as
    int32 give other spectra, so a signed sum would show."""
    P = full_range_words()
    C, K = P.shape
    assert {0xFFFFFFFF, 0x80000000, 0x7FFFFFFF} <= set(P.ravel().tolist()) and (P >> 31).any(axis=1).all()
    rng = np.random.default_rng(33)
    for n in (1, 2, 3, 12):
        got = integrate(P, n)
        prior = rng.integers(0, 1 << 36, size=got.shape).astype(np.float32)  # integers, so prior + RN((float)S) is one exactly
        acc = integrate(P, n, prior=prior)
        for i in range(K // n):
            for c in range(C):
                s = sum(int(P[c, i * n + j]) for j in range(n))
                assert got[i, c].tobytes() == _rn_float(s).tobytes(), (n, i, c, s)
                assert float(prior[i, c]) == int(prior[i, c])
                assert acc[i, c].tobytes() == _rn_float(int(prior[i, c]) + int(_rn_float(s))).tobytes(), (n, i, c)
        signed = stokes_model.integrate(P.view(np.int32).reshape(C, K, 1, 1), n).reshape(K // n, C)
        assert (signed != got).any(axis=1).all(), n  # every spectrum tells the two readings apart


def test_one_rounding_differs_from_rounding_through_an_intermediate():
    """S = (2^24 + 1) + 1 = 2^24 + 2 is a float; summing the blocks as floats first rounds 2^24 + 1 to 2^24 (tie to even),
    then 2^24 + 1 again to 2^24: the contract's single rounding of the exact sum is not that."""
    P = np.array([[(1 << 24) + 1, 1]], dtype=np.uint32)
    got = integrate(P, 2)
    assert float(got[0, 0]) == float((1 << 24) + 2)
    through_floats = np.float32(np.float32(P[0, 0]) + np.float32(P[0, 1]))
    assert float(through_floats) == float(1 << 24) and through_floats != got[0, 0]
    # an inexact one: the exact sum 2^25 + 3 is above the tie between the floats 2^25 and 2^25 + 4 and goes up; through
    # floats, 2^24 + 1 and 2^24 + 2 become 2^24 and 2^24 + 2, whose sum 2^25 + 2 is the tie and goes down to 2^25
    P = np.array([[(1 << 24) + 1, (1 << 24) + 2]], dtype=np.uint32)
    assert float(integrate(P, 2)[0, 0]) == float((1 << 25) + 4)
    assert float(np.float32(np.float32(P[0, 0]) + np.float32(P[0, 1]))) == float(1 << 25)
    # ties go to even, both ways
    assert float(to_float([(1 << 24) + 1])[0]) == float(1 << 24)
    assert float(to_float([(1 << 24) + 3])[0]) == float((1 << 24) + 4)
    for s in (0, 1, (1 << 24) + 1, (1 << 24) + 3, (1 << 32) + (1 << 8), 5 << 30, (1 << 40) + (1 << 16) + 1, (1 << 52) + 12345):
        assert to_float([s])[0].tobytes() == _rn_float(s).tobytes(), s
