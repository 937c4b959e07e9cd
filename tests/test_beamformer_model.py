"""The host models of the beamformers' arithmetic (tests/helpers/beamformer_model.py) against exact rational arithmetic
and against the oracle's verifier loop -- no GPU.  tests/test_gpu_beamformer_exact.py holds the kernels to these models
bit for bit; here the models themselves are anchored."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import rand_table
from helpers.beamformer_model import (FIX_SCALE, INV, acc_model, all_pairs_fast, digit_sums, digits, first_difference, fixed,
                                      fused_model, normalise, recombine, weighted_coefficients)

K = FIX_SCALE
U = Fraction(1, 2 ** 24)  # the relative error of one fp32 rounding to nearest (normal range)
ONE_UP = np.nextafter(np.float32(1), np.float32(2))


def rn32(q):
    """A rational rounded to the nearest fp32, ties to even (no double rounding: done on integers)."""
    q = Fraction(q)
    if q == 0:
        return np.float32(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n = round(a / ulp)  # Fraction.__round__: half to even
    v = float(n * ulp)  # exact: n has at most 25 bits
    out = np.float32(v if q > 0 else -v)
    assert float(out) == (v if q > 0 else -v)
    return out


def fixed_exact(w):
    """fixed() of one fp32 value in rational arithmetic."""
    p = Fraction(float(rn32(Fraction(float(w)) * K)))
    p = max(Fraction(-K), min(Fraction(K), p))
    return round(p)


def test_rn32_is_round_to_nearest_even():
    one = Fraction(1)
    assert rn32(one + Fraction(1, 2 ** 24)) == np.float32(1)  # tie: even
    assert rn32(one + Fraction(3, 2 ** 24)) == np.float32(1) + np.float32(2 ** -22)  # tie: even (up)
    assert rn32(one + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == ONE_UP
    assert rn32(Fraction(1, K)) == INV
    assert rn32(Fraction(-16777217)) == np.float32(-16777216)


def test_fixed_edge_cases():
    f = np.float32
    assert fixed(f(1)) == K and fixed(f(-1)) == -K
    assert fixed(ONE_UP) == K and fixed(-ONE_UP) == -K  # one ulp above 1: clamped, no fourth digit
    assert fixed(f(0.0)) == 0 and fixed(f(-0.0)) == 0
    assert fixed(f(0.5)) == 4177856 and fixed(f(-0.5)) == -4177856  # 4177855.5: tie to even
    assert fixed(np.nextafter(f(1), f(0))) == K - 1  # K - 0.498 -> RN32: K - 0.5 -> the tie goes to the even 8355710
    # every value against the rational evaluation
    rng = np.random.default_rng(1)
    w = np.concatenate([rng.uniform(-1, 1, 2000).astype(f), f([1, -1, 0.5, -0.5, 0.25, 2 ** -24, 2 ** -23, 3e-8, -6e-8]), [ONE_UP, -ONE_UP]])
    got = fixed(w)
    for wi, gi in zip(w, got):
        assert int(gi) == fixed_exact(wi), float(wi)
    # the digits of +-1 and 0
    assert [int(d) for d in digits(fixed(f(1)))] == [127, 127, 127]
    assert [int(d) for d in digits(fixed(f(-1)))] == [-127, -127, -127]
    assert [int(d) for d in digits(fixed(f(0)))] == [0, 0, 0]


def test_digits_round_trip_at_the_carry_neighbours():
    edge = [0, 1, -1, 126, 127, 128, 129, -127, -128, -129, -130, 255, 256, 257, 32511, 32512, 32639, 32640, 32641, 32767, 32768,
            32769, -32767, -32768, -32769, -32896, -32897, 65535, 65536, 65537, 8323072, 8355710, K, -K, -8355710, 8388607 - 32897]
    F = np.array([v for v in edge if abs(v) <= K] + list(np.random.default_rng(2).integers(-K, K + 1, 5000)), dtype=np.int64)
    d1, d2, d3 = digits(F)  # asserts the digit range and d1 * 65536 + d2 * 256 + d3 == F
    # the device's form of the same digits: bytes of (F + 0x808080) ^ 0x808080, read as signed
    word = ((F + 0x808080) ^ 0x808080) & 0xFFFFFF
    for shift, d in ((16, d1), (8, d2), (0, d3)):
        byte = (word >> shift) & 0xFF
        assert np.array_equal(np.where(byte >= 128, byte - 256, byte), d)
    assert np.array_equal(np.stack(digits(np.int64(128))), [0, 1, -128])
    assert np.array_equal(np.stack(digits(np.int64(-129))), [0, -1, 127])
    assert np.array_equal(np.stack(digits(np.int64(32768))), [1, -128, 0])
    with pytest.raises(AssertionError):
        digits(np.int64(K + 1))  # 127, 127, 128: no such digit


def _coefficients(kind, rng, C, A, B):
    f = np.float32
    if kind == "trig":
        rot = rng.uniform(-200, 200, (C, A, B)).astype(f).astype(np.float64)
        return np.stack([np.cos(rot), np.sin(rot)], axis=-1).astype(f)
    if kind == "special":
        return rng.choice(np.array([1, -1, 0, 0.5, -0.5, ONE_UP], dtype=f), size=(C, A, B, 2))
    assert kind == "halfway"  # RN32((n + 1/2) / K): w * K lands on, or a hair beside, a tie of rint
    n = rng.integers(-K, K, size=(C, A, B, 2))
    return ((n + 0.5) / K).astype(f)


def _samples(kind, rng, C, nT16, A):
    if kind == "special":
        return rng.choice(np.array([-128, 127], dtype=np.int8), size=(C, nT16, A, 16, 2))
    x = rng.integers(-128, 128, size=(C, nT16, A, 16, 2), dtype=np.int8)
    x[:, :, :, 0, :] = -128  # a full-scale column in every case
    x[:, :, :, 1, :] = 127
    return x


@pytest.mark.parametrize("kind", ["trig", "special", "halfway"])
@pytest.mark.parametrize("A", [1, 3, 64, 65, 200, 256])
def test_acc_model_against_rational_arithmetic_and_the_derived_bound(A, kind):
    """acc_model, per output element, against Python integers and fractions.

    (1) The integer part: 65536 * s1 + 256 * s2 + s3 == S := sum_a F_a * x_a with F_a = fixed(w_a) evaluated in rational
    arithmetic, and the fp32 tail is exactly RN32(RN32(65536 * s1 + RN32(256 * s2 + s3)) * RN32(1 / K)), K = 8355711:
    three roundings (conversion of the low part, the fma, the product) applied to a constant that carries a fourth.

    (2) The distance from the exact sum E = sum_a w_a * x_a of the fp32 coefficients, term by term (u = 2^-24):
      * quantisation, |F_a - w_a K| <= q_a: for |w_a| <= 1, |w_a K| < 2^23 where fp32 is spaced 1/2 at most, so
        RN32(w_a K) is within 1/4, the clamp to +-K does nothing (K is an fp32 number and rounding is monotone), and rint
        adds at most 1/2: q_a = 3/4.  For |w_a| > 1 (one ulp above 1 is what a 1-ULP sine can give) F_a = +-K and
        q_a = K (|w_a| - 1) = 0.996.  So |S / K - E| <= sum_a q_a |x_a| / K;
      * L = 256 * s2 + s3 converts as L (1 + e0), f = (65536 * s1 + L (1 + e0)) (1 + e1), inv = (1 + e2) / K, and the
        result is r = f * inv * (1 + e3), every |e| <= u (all values are normal fp32 numbers or zero: f is an integer):
            r = (S + L e0) (1 + e1) (1 + e2) (1 + e3) / K
            |r - S / K| <= |S| / K * ((1 + u)^3 - 1) + |L| * u * (1 + u)^3 / K.
    bound = sum_a q_a |x_a| / K + |L| u (1 + u)^3 / K + |S| ((1 + u)^3 - 1) / K, asserted in rational arithmetic with no
    factor on top.  In closed form, for |w_a| <= 1: |L| <= 128 * 257 * sum_a |x_a| and |S| / K <= |E| + 0.75 / K * sum|x|, so
    bound <= 9e-8 * sum_a |x_a| + 1.8e-7 * |E| (0.75 / K = 8.976e-8, + 2^-24 * 32896 / K = 2.3e-10; 3 u = 1.788e-7): the
    figure include/dcs_beamformer.h quotes.  The three roundings are up to 3 ulp of the result, not 1.5: u |r| is a whole
    ulp when r sits just below a power of two."""
    rng = np.random.default_rng(1000 * A + len(kind))
    C, B, nT16 = 1, 3, 1
    coef = _coefficients(kind, rng, C, A, B)
    x = _samples(kind, rng, C, nT16, A)
    s1, s2, s3 = digit_sums(coef, x)
    got = acc_model(coef, x)
    assert got.dtype == np.float32 and got.shape == (C, nT16, B, 16, 2)
    assert first_difference(got, recombine(s1, s2, s3)) is None
    w_q = [[[Fraction(float(coef[0, a, b, k])) for a in range(A)] for k in range(2)] for b in range(B)]
    F_q = [[[fixed_exact(coef[0, a, b, k]) for a in range(A)] for k in range(2)] for b in range(B)]
    q_q = [[[Fraction(3, 4) if abs(w) <= 1 else K * (abs(w) - 1) for w in w_q[b][k]] for k in range(2)] for b in range(B)]
    inv = Fraction(float(INV))
    assert INV == rn32(Fraction(1, K))
    growth = (1 + U) ** 3
    worst = Fraction(0)
    for b in range(B):
        for i in range(16):
            for k in range(2):
                xs = [int(v) for v in x[0, 0, :, i, k]]
                S = sum(F * v for F, v in zip(F_q[b][k], xs))
                i1, i2, i3 = int(s1[0, 0, b, i, k]), int(s2[0, 0, b, i, k]), int(s3[0, 0, b, i, k])
                assert 65536 * i1 + 256 * i2 + i3 == S
                L = 256 * i2 + i3
                f = rn32(65536 * i1 + Fraction(float(rn32(L))))
                r = rn32(Fraction(float(f)) * inv)
                assert r.view(np.uint32) == got[0, 0, b, i, k].view(np.uint32), (b, i, k)
                E = sum(w * v for w, v in zip(w_q[b][k], xs))
                mag = sum(abs(v) for v in xs)
                bound = (sum(q * abs(v) for q, v in zip(q_q[b][k], xs)) + abs(L) * U * growth + abs(S) * (growth - 1)) / K
                err = abs(Fraction(float(r)) - E)
                assert err <= bound, (b, i, k, float(err), float(bound))
                if kind != "special":  # |w| <= 1: the header's closed form
                    assert bound <= Fraction(9, 10 ** 8) * mag + Fraction(18, 10 ** 8) * abs(E)
                if mag:
                    worst = max(worst, err / mag)
    if A == 1:  # the inputs do reach the quantisation term (and the rounded "9e-8 * sum|x| + 1.5 ulp" the header used to quote)
        assert worst > Fraction(9, 10 ** 8), float(worst)


def test_acc_model_weighted_scale_is_one_more_rounding():
    rng = np.random.default_rng(7)
    C, A, B = 2, 37, 5
    coef = _coefficients("trig", rng, C, A, B)
    x = _samples("trig", rng, C, 2, A)
    w = (rng.choice([-1.0, 1.0], size=(B, A)) * 10.0 ** rng.uniform(-3, 3, size=(B, A))).astype(np.float32)
    w[2] = 0
    s, gh = normalise(w)
    assert s[2] == 0 and np.all(gh[2] == 0) and np.all(np.abs(gh) <= 1) and np.all(np.abs(gh).max(axis=1)[s > 0] == 1)
    wc = weighted_coefficients(coef, gh)
    got = acc_model(wc, x, scale=s)
    s1, s2, s3 = digit_sums(wc, x)
    inv = Fraction(float(INV))
    for b in range(B):
        fac = rn32(Fraction(float(s[b])) * inv)
        for idx in ((0, 0, b, 0, 0), (1, 1, b, 7, 1), (0, 1, b, 15, 0)):
            L = 256 * int(s2[idx]) + int(s3[idx])
            f = rn32(65536 * int(s1[idx]) + Fraction(float(rn32(L))))
            assert rn32(Fraction(float(f)) * Fraction(float(fac))).view(np.uint32) == got[idx].view(np.uint32)
    assert np.all(got[:, :, 2] == 0)
    # unit weights: the unweighted model's bits; 2^k weights: exactly scaled
    ones = np.ones((B, A), np.float32)
    s, gh = normalise(ones)
    assert first_difference(acc_model(weighted_coefficients(coef, gh), x, scale=s), acc_model(coef, x)) is None
    s, gh = normalise(ones * np.float32(8))
    assert first_difference(acc_model(weighted_coefficients(coef, gh), x, scale=s), acc_model(coef, x) * np.float32(8)) is None


def test_largest_integer_sums_fit():
    """All samples -128 against coefficients -1 (digits -127) and against low digits of -128: |s| <= 128 * 128 * A = 2^22 at
    256 antennas, |256 * s2 + s3| < 2^31 (recombine asserts it)."""
    A = 256
    x = np.full((1, 1, A, 16, 2), -128, dtype=np.int8)
    coef = np.full((1, A, 1, 2), -1, dtype=np.float32)
    s1, s2, s3 = digit_sums(coef, x)
    assert np.all(s1 == 127 * 128 * A) and np.all(s2 == s1) and np.all(s3 == s1)
    assert np.all(acc_model(coef, x) == np.float32(128 * A))
    # low digits of -128 (a high digit of -128 would be beyond -K: the clamp excludes it): F = -126 * 65536 - 128 * 256 - 128
    F = -126 * 65536 - 128 * 256 - 128
    w0 = np.float32(F / K)
    cands = [w for w in (w0, np.nextafter(w0, np.float32(0)), np.nextafter(w0, np.float32(-2))) if fixed(w) == F]
    assert cands
    coef[:] = cands[0]
    assert [int(d) for d in digits(fixed(cands[0]))] == [-126, -128, -128]
    s1, s2, s3 = digit_sums(coef, x)
    assert np.all(s1 == 126 * 128 * A) and np.all(s2 == 2 ** 22) and np.all(s3 == 2 ** 22)  # (-128) * (-128) = 2^14 per antenna
    got = recombine(s1, s2, s3)
    assert np.all(got == rn32(Fraction(float(rn32(Fraction(-F * 128 * A)))) * Fraction(float(INV))))


@pytest.mark.parametrize("A,B,C,nt", [(5, 3, 4, 32), (130, 2, 3, 16)])
def test_fused_model_is_the_verifiers_loop(oracle, A, B, C, nt):
    """fused_model over the oracle's own coefficients gives the bits of oracle.beamform (BCT.cu:363-414: sum += coeff *
    sample with separate roundings, antennas in order): the model restates the verifier."""
    op = oracle.params(nr_channels=C, nr_stations=A, nr_beams=B)
    table = rand_table(A * B, seed=A + B)  # [b * A + a]
    ant = np.random.default_rng(A).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    coef = oracle.generate(op, np.ascontiguousarray(table.reshape(B, A).T).ravel(), 0, nt)  # [t][c][a][b][2]
    diff = first_difference(fused_model(coef, ant), oracle.beamform(op, table, nt, ant))
    assert diff is None, diff
    # weighted with unit weights: the same bits
    s, gh = normalise(np.ones((B, A), np.float32))
    assert first_difference(fused_model(coef, ant, ghat=gh, scale=s), fused_model(coef, ant)) is None


def test_fast_class_precondition_notices_a_slow_pair():
    table = rand_table(40, seed=3)
    dts = np.float32([0.0, 0.5, 1.6])
    assert all_pairs_fast(table, dts, 64, 1e-7)
    slow = table.copy()
    slow["fDelayRate_sps"][5] = 1e-2  # |fRotation| ~ 3e5 rad
    assert not all_pairs_fast(slow, dts, 64, 1e-7)
    tiny = table.copy()
    tiny["fDelayRate_sps"][7] = 1e-30  # outside the constant divide's range
    assert not all_pairs_fast(tiny, dts, 64, 1e-7)
    nan = table.copy()
    nan["fPhase_rad"][0] = np.nan
    assert not all_pairs_fast(nan, dts, 64, 1e-7)
    zero = np.zeros(6, dtype=table.dtype)  # a zero table is fast: rate term 0
    assert all_pairs_fast(zero, dts, 64, 1e-7)


def test_depth_bound_of_the_gpu_tests_is_the_pigeonhole_quotient():
    """helpers/bacc_case.py: blocks_on_some_wave, the guard of the GPU tests' DEEP_SHAPES, on geometries worked by hand."""
    from helpers.bacc_case import DEEP_SHAPES, MIN_DEPTH, blocks_on_some_wave

    one, four = (1, 1), (256, 1, 1)
    # 640 channels x 1 tile x 17 blocks = 10880 units: on 1280 four-wave workgroups 2.125 per wave, so some wave has 3; on
    # 2720 (a wave per block and more) nothing is proven beyond 1
    assert blocks_on_some_wave(16, 640, 272, (1280,) + one, four) == 3
    assert blocks_on_some_wave(16, 640, 272, (2720,) + one, four) == 1
    assert blocks_on_some_wave(16, 640, 272, (2719,) + one, four) == 2
    assert blocks_on_some_wave(17, 640, 272, (1280,) + one, four) == 5  # a ragged second tile counts as a tile
    assert blocks_on_some_wave(72, 640, 256, (1280,) + one, four) == 10
    assert blocks_on_some_wave(72, 640, 256, (1280,) + one, (512, 1, 1)) == 5  # eight waves per workgroup
    with pytest.raises(AssertionError):
        blocks_on_some_wave(16, 640, 272, (640, 2, 1), four)  # a grid that is not one-dimensional is not this kernel's
    assert all(depth >= MIN_DEPTH == 3 and nt % 16 == 0 for _, _, _, nt, depth in DEEP_SHAPES)
