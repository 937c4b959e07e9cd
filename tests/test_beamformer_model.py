"""The host models of the beamformers' arithmetic (tests/helpers/beamformer_model.py) against exact rational arithmetic
and against the oracle's verifier loop -- no GPU.  tests/test_gpu_beamformer_exact.py holds the kernels to these models
bit for bit; here the models themselves are anchored."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import rand_table
from helpers import slow_tables
from helpers.beamformer_model import (FAST_HIGH, FAST_LOW, FILLER_PHASE_HIGH, FIX_SCALE, INV, SLOW, UNCLEAR, acc_model, acc_model_nonfinite, all_pairs_fast,
                                      digit_sums, digits, first_difference, first_difference_or_nan, fixed, flagged_table, fused_model,
                                      interleave_with_filler, normalise, pair_classes, real_beams, recombine, weighted_coefficients,
                                      zero_weight_coefficients)

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


def test_passes_of_a_fused_launch_read_from_its_geometry():
    """helpers/bacc_case.py: passes_of_fused_launch, what the GPU tests of the fused kernel's 2- and 4-channel passes read
    from a captured launch, on geometries worked by hand."""
    from helpers.bacc_case import passes_of_fused_launch

    # 511 channels in groups of 4 are 128 groups, the last of 3; one beam tile, 16 blocks: 2048 workgroups.  5 antennas are
    # 640 bytes a channel
    assert passes_of_fused_launch(5, 3, 511, 16, 2048, 4 * 640) == (4, 4, 3)
    assert passes_of_fused_launch(5, 3, 511, 16, 2048, 2 * 640) == (4, 2, 1)  # the last group: a pass of 2, a pass of 1
    assert passes_of_fused_launch(5, 3, 511, 16, 2048, 640) == (4, 1, 1)
    assert passes_of_fused_launch(5, 3, 512, 16, 2048, 4 * 640) == (4, 4, 4)  # a whole last pass
    assert passes_of_fused_launch(5, 3, 510, 16, 2048, 2 * 640) == (4, 2, 2)  # a last group of 2: one whole pass of 2
    assert passes_of_fused_launch(5, 3, 511, 16, 4096, 2 * 640) == (2, 2, 1)  # 256 groups: 2 channels each
    assert passes_of_fused_launch(5, 3, 511, 16, 8176, 640) == (1, 1, 1)
    assert passes_of_fused_launch(5, 3, 511, 16, 8176, 2 * 640) == (1, 2, 1)  # a pass wider than the group: one live channel
    assert passes_of_fused_launch(7, 20, 254, 16, 2048, 4 * 7 * 128) == (4, 4, 2)  # two beam tiles, 64 groups
    assert passes_of_fused_launch(7, 20, 254, 3, 2 * 3 * 127, 2 * 7 * 128) == (2, 2, 2)
    # more than 128 antennas are staged 128 at a time: 16 KiB a channel
    assert passes_of_fused_launch(129, 2, 511, 16, 2048, 32768) == (4, 2, 1)
    assert passes_of_fused_launch(300, 2, 511, 16, 2048, 16384) == (4, 1, 1)
    assert passes_of_fused_launch(64, 3, 509, 16, 2048, 32768) == (4, 4, 1)
    with pytest.raises(AssertionError):
        passes_of_fused_launch(5, 3, 2, 16, 16, 2 * 640)  # ambiguous: one group of 2 channels is ceil(2 / 2) and ceil(2 / 4)
    with pytest.raises(AssertionError):
        passes_of_fused_launch(5, 3, 1, 16, 16, 640)  # ambiguous: one channel is one group whatever cpb
    with pytest.raises(AssertionError):
        passes_of_fused_launch(5, 3, 511, 16, 2047, 4 * 640)  # no whole number of channel groups
    with pytest.raises(AssertionError):
        passes_of_fused_launch(7, 20, 254, 16, 2048 + 16, 4 * 7 * 128)  # whole groups of ONE beam tile only
    with pytest.raises(AssertionError):
        passes_of_fused_launch(5, 3, 511, 16, 2048, 3 * 640)  # 3 channels per pass: no form of the kernel
    with pytest.raises(AssertionError):
        passes_of_fused_launch(5, 3, 511, 16, 2048, 4 * 640 + 4)  # no whole number of channels
    with pytest.raises(AssertionError):
        passes_of_fused_launch(129, 2, 511, 16, 2048, 2 * 129 * 128)  # sized for 129 antennas, not for the staged 128
    with pytest.raises(AssertionError):
        passes_of_fused_launch(5, 3, 511, 16, 16 * 100, 4 * 640)  # 100 groups: no cpb of 1, 2, 4


# ---- what tests/test_gpu_beamformer_exact_slow.py stands on
@pytest.fixture(scope="module")
def lab():
    """dc_sand_amd/csrc/bf_math.h compiled for the host (tests/numerics, as tests/test_numerics.py builds it)."""
    import ctypes
    import subprocess
    from pathlib import Path

    lab_dir = Path(__file__).resolve().parent / "numerics"
    res = subprocess.run(["make", "-C", str(lab_dir)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    L = ctypes.CDLL(str(lab_dir / "libnumerics_lab.so"))
    L.lab_generate_fast.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                    ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                    ctypes.POINTER(ctypes.c_uint64)]
    return L


def _class_tables():
    """(name, table, fDeltaTime values, channels) of the tables the slow-class GPU tests use and of the boundaries' far sides."""
    dts = np.float32([0.0, 0.3710937, 9 * 1.5e-3, 1.6])
    A, B = 37, 21
    edge = rand_table(A * B, seed=5)
    edge["fDelayRate_sps"][:] = 0.0  # the zero rate term: fast whatever its exponent field says
    edge["fDelayRate_sps"][3] = 1e-30  # the tiny one: below 2^-60, slow
    edge["fDelayRate_sps"][4] = -1e-30
    edge["fPhase_rad"][7] = 20000.0  # full degree
    return [("rand_table", rand_table(A * B, seed=A + B), dts, 9),
            ("one slow pair", slow_tables.one_slow_pair(A, B), dts, 9),
            ("one slow pair, kChain", slow_tables.one_slow_pair(200, 20), dts, 2),
            ("all slow", slow_tables.all_slow(A, B), dts, 3),
            ("crossing", slow_tables.crossing(A, B), slow_tables.crossing_times(), 3),
            ("tiny and zero rate terms", edge, dts, 64)]


@pytest.mark.parametrize("name,table,dts,C", _class_tables(), ids=[t[0] for t in _class_tables()])
def test_pair_classes_count_what_bf_math_counts(lab, name, table, dts, C):
    """pair_classes against dcs_pair_terms / dcs_pair_class compiled for the host (lab_generate_fast: n_slow_pairs and
    n_low_pairs of one time step), at every time: equal counts, and none of these tables has an unclear pair."""
    import ctypes

    cls = pair_classes(table, dts, C, slow_tables.SAMPLING_PERIOD)
    assert cls.shape == (len(dts), table.size) and not np.any(cls == UNCLEAR)
    d = np.ascontiguousarray(table)
    out = np.empty((1, table.size, 2), dtype=np.float32)
    for i, dt in enumerate(dts):
        slow, low = ctypes.c_uint64(), ctypes.c_uint64()
        lab.lab_generate_fast(0, d.ctypes.data, table.size, C, np.float32(slow_tables.SAMPLING_PERIOD), np.float32(dt), 0, 1,
                              out.ctypes.data, ctypes.byref(slow), ctypes.byref(low))
        assert (int(np.sum(cls[i] == SLOW)), int(np.sum(cls[i] == FAST_LOW))) == (slow.value, low.value), (name, i, float(dt))
    # what each table is meant to be
    if name == "rand_table":
        assert np.all(cls == FAST_LOW) and all_pairs_fast(table, dts, C, slow_tables.SAMPLING_PERIOD)
    elif name.startswith("one slow pair"):
        assert np.all(np.sum(cls == SLOW, axis=1) == 1) and np.all(np.sum(cls == FAST_LOW, axis=1) == table.size - 1)
        assert not all_pairs_fast(table, dts, C, slow_tables.SAMPLING_PERIOD)
    elif name == "all slow":
        assert np.all(cls == SLOW)
    elif name == "crossing":
        assert tuple(slow_tables.block_classes(cls)) == slow_tables.CROSSING_BLOCK_CLASSES
        i = (21 // 2) * 37 + 37 // 2
        assert np.all(cls[:16, i] == FAST_HIGH) and list(cls[16:20, i]) == [FAST_HIGH, FAST_HIGH, FAST_HIGH, SLOW] and np.all(cls[19:, i] == SLOW)
        assert np.all(np.delete(cls, i, axis=1) == FAST_LOW)
    else:
        assert np.all(cls[:, [3, 4]] == SLOW) and np.all(cls[:, 7] == FAST_HIGH) and np.all(np.delete(cls, [3, 4, 7], axis=1) == FAST_LOW)


def test_pair_classes_marks_the_neighbourhood_of_every_boundary_and_non_finite_values_slow():
    t = np.zeros(12, dtype=rand_table(1).dtype)
    t["fPhase_rad"][:6] = [31900.0, 32100.0, 499.0, 501.5, 31000.0, 33000.0]
    t["fDelayRate_sps"][6:10] = [2.0 ** -61, 2.0 ** -60, 1.5 * 2.0 ** 60, 2.0 ** 61]  # (the last two: |fRotation| is huge anyway)
    t["fDelayRate_sps"][10] = np.inf
    t["fDelay_s"][11] = np.nan
    cls = pair_classes(t, np.float32([0.0, 0.5]), 1, 1e-7)  # one channel: the rate term's bound is 0, its exponent still counts
    for row in cls:
        assert list(row) == [UNCLEAR] * 4 + [FAST_HIGH, SLOW] + [UNCLEAR] * 4 + [SLOW, SLOW]
    # a flagged pair is made from zero terms, whatever its delay values are
    w = np.ones((3, 4), np.float32)
    w[2, 2], w[2, 3] = 0.0, -0.0
    assert np.all(pair_classes(flagged_table(t, w), np.float32([0.5]), 1, 1e-7)[0, 10:] == FAST_LOW)
    assert np.array_equal(flagged_table(t, w)[:10], t[:10])


def test_interleaving_with_fillers_and_slicing_back_are_inverse():
    A, B, C = 5, 3, 2
    table_ab = rand_table(A * B, seed=11)
    t2 = interleave_with_filler(table_ab, A, B)
    assert t2.shape == (A * 2 * B,) and t2.dtype == table_ab.dtype
    two = t2.reshape(A, 2 * B)
    assert np.array_equal(two[:, 0::2].ravel(), table_ab)  # a real pair's entry is untouched, at [a * 2 B + 2 b]
    for a in range(A):
        for b in range(B):
            assert t2[a * 2 * B + 2 * b] == table_ab[a * B + b]
            assert tuple(t2[a * 2 * B + 2 * b + 1]) == (0.0, 0.0, 40000.0, 0.0)
    # every filler is plainly slow at any time, so every run of two consecutive pairs holds a slow pair
    cls = pair_classes(t2, np.float32([0.0, 0.37, 1.6]), C, 1e-7)
    assert np.all(cls.reshape(3, A, 2 * B)[:, :, 1::2] == SLOW) and np.all(cls.reshape(3, A, 2 * B)[:, :, 0::2] == FAST_LOW)
    # fillers of the full-degree fast class: the same places, the real pairs untouched
    high = interleave_with_filler(table_ab, A, B, FILLER_PHASE_HIGH)
    assert np.array_equal(high.reshape(A, 2 * B)[:, 0::2].ravel(), table_ab) and np.all(high["fPhase_rad"].reshape(A, 2 * B)[:, 1::2] == 20000.0)
    cls = pair_classes(high, np.float32([0.0, 0.37, 1.6]), C, 1e-7)
    assert np.all(cls.reshape(3, A, 2 * B)[:, :, 1::2] == FAST_HIGH) and np.all(cls.reshape(3, A, 2 * B)[:, :, 0::2] == FAST_LOW)
    # a tensor in the generator's order [t][c][a][2 B][2] that carries its own index comes back as [t][c][a][B][2]
    coef2 = np.arange(3 * C * A * 2 * B * 2, dtype=np.float32).reshape(3, C, A, 2 * B, 2)
    back = real_beams(coef2)
    assert back.shape == (3, C, A, B, 2)
    for b in range(B):
        assert np.array_equal(back[:, :, :, b], coef2[:, :, :, 2 * b])


def test_non_finite_model_against_a_plain_loop():
    """acc_model_nonfinite and first_difference_or_nan at one small case, element by element in Python: the verifier's sum
    with a NaN coefficient is NaN whatever the samples are (NaN * 0 = NaN), the others are acc_model's."""
    rng = np.random.default_rng(3)
    C, A, B, nT16 = 2, 7, 4, 2
    coef = _coefficients("trig", rng, C, A, B)
    x = _samples("trig", rng, C, nT16, A)
    x[:, :, 5] = 0  # the antenna of the NaN coefficient below is silent: its beam is NaN all the same
    bad = coef.copy()
    bad[0, 5, 1, :] = np.nan  # channel 0, beam 1, both planes
    bad[1, 2, 3, 1] = np.inf  # channel 1, beam 3, the im plane only
    got = acc_model_nonfinite(bad, x)
    clean = acc_model(np.where(np.isfinite(bad), bad, np.float32(0)), x)
    for c in range(C):
        for t in range(nT16):
            for b in range(B):
                for i in range(16):
                    for k in range(2):
                        column_bad = any(not np.isfinite(bad[c, a, b, k]) for a in range(A))
                        assert column_bad == ((c, b) == (0, 1) or (c, b, k) == (1, 3, 1))
                        if column_bad:
                            assert np.isnan(got[c, t, b, i, k])
                        else:
                            assert got[c, t, b, i, k].view(np.uint32) == clean[c, t, b, i, k].view(np.uint32)
    assert first_difference(acc_model_nonfinite(coef, x), acc_model(coef, x)) is None  # finite: acc_model itself
    # the comparison: NaN of any payload where the model has NaN, bits elsewhere
    assert first_difference_or_nan(got, got) is None
    other = got.copy()
    other[0, 0, 1, 0, 0] = np.float32(-np.nan)
    assert first_difference_or_nan(other, got) is None
    other[0, 0, 1, 0, 0] = 0.0
    assert "NaN in" in first_difference_or_nan(other, got)
    other = got.copy()
    other[1, 1, 0, 3, 0] = np.nextafter(other[1, 1, 0, 3, 0], np.float32(1e9))
    assert "1 of" in first_difference_or_nan(other, got)
    # weights: a flagged antenna's coefficient is made from zero terms, so its NaN goes; ghat * NaN stays NaN
    w = np.ones((B, A), np.float32)
    w[:, 5] = 0.0
    s, gh = normalise(w)
    z = zero_weight_coefficients(bad, w)
    assert np.all(z[:, 5] == np.float32([1, 0])) and np.array_equal(np.delete(z, 5, axis=1), np.delete(bad, 5, axis=1), equal_nan=True)
    flagged = acc_model_nonfinite(weighted_coefficients(z, gh), x, scale=s)
    assert not np.isnan(flagged[0]).any() and np.isnan(flagged[1, :, 3, :, 1]).all() and np.isnan(flagged).sum() == nT16 * 16
    with np.errstate(invalid="ignore"):
        unflagged = acc_model_nonfinite(weighted_coefficients(bad, normalise(np.ones((B, A), np.float32))[1]), x, scale=s)
    assert first_difference_or_nan(unflagged, got) is None
    # the fused model propagates NaN by itself (a coefficient is a sine or a cosine: NaN, never Inf)
    nans = np.where(np.isfinite(bad), bad, np.float32(np.nan))
    with np.errstate(invalid="ignore"):
        f = fused_model(np.broadcast_to(nans, (16 * nT16,) + bad.shape).copy(), x)
    assert np.array_equal(np.isnan(f), np.isnan(got))


def test_equality_sees_what_the_old_bounds_let_through():
    """(64, 16, 2, 32), the shape tests/test_gpu_class_replay.py holds to 4e-5 * A + 1e-6: ONE unit of the middle digit of
    one antenna's coefficients (256 / 8355711 = 3.1e-5 per unit of sample).  That antenna's samples are drawn within +-64
    here -- at full scale, 128, the unit moves an output by 3.9e-3 and even the bound notices -- and every changed output
    is within the bound of the unchanged one, while first_difference names the first of them."""
    A, B, C, nt = 64, 16, 2, 32
    rng = np.random.default_rng(64)
    coef = _coefficients("trig", rng, C, A, B)
    x = rng.integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    a0 = 29
    x[:, :, a0] = rng.integers(-64, 65, size=(C, nt // 16, 16, 2), dtype=np.int8)
    s1, s2, s3 = digit_sums(coef, x)
    ref = recombine(s1, s2, s3)
    assert first_difference(ref, acc_model(coef, x)) is None
    s2_off = s2 + x[:, :, a0].astype(np.int64)[:, :, None]  # d2 of antenna a0 one higher in every beam: [C][nT16][1][16][2]
    off = recombine(s1, s2_off, s3)
    err = np.abs(off.astype(np.float64) - ref.astype(np.float64))
    assert 1.5e-3 < err.max() <= 4e-5 * A + 1e-6  # the old bound passes it ...
    diff = first_difference(off, ref)
    assert diff is not None and int(diff.split()[0]) > 0.8 * ref.size, diff  # ... equality does not, nearly everywhere
