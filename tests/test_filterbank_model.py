"""Anchors of the numpy model of the 8-bit search filterbanks (helpers/filterbank_model.py; include/dcs_filterbank.h):
the fp64 sums against exact rationals rounded explicitly, the scales against the same, the quantiser against a plain
per-element Python loop, ties to even, and that float32 sums over time are a different function.  No GPU needed."""
import math
import struct
from fractions import Fraction

import numpy as np

from helpers.filterbank_model import filterbank, quantise, same_bits, scales, spectra_sums


def rn64(q):
    """A rational rounded to the nearest double, ties to even, by explicit arithmetic on its integer significand (finite,
    normal results only)."""
    if q == 0:
        return 0.0
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()  # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1) and -1022 <= e <= 1023
    scaled = q / Fraction(2) ** (e - 52)  # in [2^52, 2^53)
    n, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and n & 1):
        n += 1
    return sign * math.ldexp(float(n), e - 52)  # n <= 2^53: exact


def test_rn64_is_the_ieee_rounding():
    for num, den in ((1, 3), (2, 3), (1, 10), (-7, 9), (10 ** 30 + 1, 7), (1, 10 ** 20)):
        assert rn64(Fraction(num, den)) == num / den  # Python's int / int is correctly rounded
    assert rn64(Fraction(2 ** 53 + 1)) == 2.0 ** 53 and rn64(Fraction(2 ** 53 + 3)) == 2.0 ** 53 + 4  # ties to even


def test_sums_are_the_stated_sequence_of_roundings():
    rng = np.random.default_rng(7)
    T, C, B = 37, 3, 2
    x = (rng.standard_normal((T, C, B)) * np.exp2(rng.integers(-20, 21, size=(T, C, B)))).astype(np.float32)  # a wide range per sum
    got = spectra_sums(x)
    inexact = 0
    for c in range(C):
        for b in range(B):
            s1 = s2 = 0.0
            for t in range(T):
                f = Fraction(float(x[t, c, b]))
                n1, n2 = rn64(Fraction(s1) + f), rn64(Fraction(s2) + f * f)
                inexact += (Fraction(n1) != Fraction(s1) + f) + (Fraction(n2) != Fraction(s2) + f * f)
                s1, s2 = n1, n2
            assert struct.pack("<2d", s1, s2) == got[c, b].tobytes(), (c, b)
    assert inexact > T  # the roundings are exercised
    # accumulate: three parts from the running sums are one pass over the joined spectra
    part = spectra_sums(x[25:], prior=spectra_sums(x[10:25], prior=spectra_sums(x[:10])))
    assert same_bits(part, got) is None


def test_float32_sums_are_a_different_function():
    x = np.array([2.0 ** 24, 1.0, 1.0], np.float32).reshape(3, 1, 1)
    s = spectra_sums(x)
    assert s[0, 0, 0] == 2.0 ** 24 + 2
    f = np.float32(0)
    for v in x.ravel():
        f = np.float32(f + v)
    assert float(f) == 2.0 ** 24  # through floats both ones are lost


def test_scales_against_exact_rationals():
    rng = np.random.default_rng(11)
    T, C, B = 50, 4, 3
    x = (np.exp2(rng.integers(-20, 21, size=(1, C, B))) * (1 + 0.25 * rng.standard_normal((T, C, B)))).astype(np.float32)
    sums = spectra_sums(x)
    got = scales(sums, T, 24.0)
    for c in range(C):
        for b in range(B):
            s1, s2 = (Fraction(float(v)) for v in sums[c, b])
            m = rn64(s1 / T)
            var = rn64(Fraction(rn64(s2 / T)) - Fraction(rn64(Fraction(m) * Fraction(m))))
            assert var > 0
            sd = math.sqrt(var)  # correctly rounded: checked on the next line
            lo, hi = Fraction(np.nextafter(sd, 0.0)), Fraction(np.nextafter(sd, np.inf))
            assert ((Fraction(sd) + lo) / 2) ** 2 < Fraction(var) < ((Fraction(sd) + hi) / 2) ** 2
            k = rn64(Fraction(24) / Fraction(sd))
            assert same_bits(got[c, b], np.array([np.float32(m), np.float32(k)], np.float32)) is None, (c, b)
    # a constant channel, a NaN and a negative variance from rounding give k = 0
    const = np.full((9, 1, 1), 0.1, np.float32)
    assert scales(spectra_sums(const), 9, 24.0)[0, 0, 1] == 0
    odd = scales(np.array([[[np.nan, 1.0]], [[3.0, 2.0]], [[np.inf, np.inf]]]), 3, 24.0)
    assert np.isnan(odd[0, 0, 0]) and odd[0, 0, 1] == 0 and odd[1, 0, 1] == 0 and odd[1, 0, 0] == 1 and odd[2, 0, 1] == 0


def py_quantise(x, mu, k, level):
    f = np.float32
    with np.errstate(all="ignore"):
        d = f(f(x) - f(mu))
        y = f(f(d * f(k)) + f(level))
    if math.isnan(y):
        return 0, True
    if math.isinf(y):
        return (255 if y > 0 else 0), True
    r = round(float(y))  # Python's round: ties to even
    return min(max(r, 0), 255), r < 0 or r > 255


def test_quantiser_against_a_plain_loop():
    rng = np.random.default_rng(3)
    T, C, B = 6, 5, 3
    x = (100 * rng.standard_normal((T, C, B))).astype(np.float32)
    x.ravel()[[0, 7, 20, 33, 41, 60]] = [np.nan, np.inf, -np.inf, -0.0, 1e-45, 1e30]
    sc = np.stack([rng.standard_normal((C, B)) * 10, np.abs(rng.standard_normal((C, B))) * 2], axis=-1).astype(np.float32)
    sc[1, 1] = (np.nan, 1.0)
    sc[2, 0] = (0.0, np.inf)
    sc[3, 2] = (0.0, np.nan)
    sc[4, 1] = (5.0, 0.0)
    q, clipped = quantise(x, sc, 128.0)
    assert 0 < clipped.sum() < clipped.size and np.unique(q).size > 20
    for t in range(T):
        for c in range(C):
            for b in range(B):
                assert (int(q[t, c, b]), bool(clipped[t, c, b])) == py_quantise(x[t, c, b], sc[c, b, 0], sc[c, b, 1], 128.0), (t, c, b)
    for desc in (False, True):
        prefill = np.full((B, T + 3, C), 0x5A, np.uint8)
        out, counts = filterbank(x, sc, 128.0, descending=desc, out=prefill, first=2)
        assert np.all(out[:, :2] == 0x5A) and np.all(out[:, 2 + T:] == 0x5A)
        for b in range(B):
            assert counts[b] == clipped[:, :, b].sum()
            for t in range(T):
                row = q[t, :, b][::-1] if desc else q[t, :, b]
                assert np.array_equal(out[b, 2 + t], row)


def test_ties_round_to_even():
    x = np.arange(-3, 260, dtype=np.float32).reshape(-1, 1, 1)  # y = x + 0.5: every one a tie
    sc = np.array([[[0.0, 1.0]]], np.float32)
    q, clipped = quantise(x, sc, 0.5)
    for v, got, cl in zip(x.ravel(), q.ravel(), clipped.ravel()):
        r = int(v) + (int(v) & 1)  # the even neighbour of v + 0.5
        assert r % 2 == 0 and got == min(max(r, 0), 255), v
        assert cl == (r < 0 or r > 255), v
    assert q[2, 0, 0] == 0 and not clipped[2, 0, 0]  # -1 + 0.5 rounds to -0: not below 0
