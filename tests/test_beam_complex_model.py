"""The host model of the complex-product beamformer (tests/helpers/beam_complex_model.py; include/dcs_beam_complex.h)
against Python integers and exact rational arithmetic -- no GPU.  tests/test_gpu_beam_complex.py holds the kernels to the
model bit for bit; here the model itself is anchored, as tests/test_beamformer_model.py anchors the element-wise one."""
from fractions import Fraction

import numpy as np
import pytest

from helpers.beam_complex_model import SUM_BOUND, complex_model, digit_sums, low_part, operands, recombine
from helpers.beamformer_model import FIX_SCALE, INV, digits, first_difference, fixed, normalise, weighted_coefficients
from test_beamformer_model import ONE_UP, U, fixed_exact, rn32

K = FIX_SCALE


def _coefficients(kind, rng, C, A, B):
    f = np.float32
    if kind == "trig":
        rot = rng.uniform(-200, 200, (C, A, B)).astype(f).astype(np.float64)
        return np.stack([np.cos(rot), np.sin(rot)], axis=-1).astype(f)
    if kind == "special":
        return rng.choice(np.array([1, -1, 0, 0.5, -0.5, ONE_UP], dtype=f), size=(C, A, B, 2))
    if kind == "halfway":  # RN32((n + 1/2) / K): w * K lands on, or a hair beside, a tie of rint
        n = rng.integers(-K, K, size=(C, A, B, 2))
        return ((n + 0.5) / K).astype(f)
    assert kind == "low128"  # F with -128 in its low digits: the numbers whose negation has other digits than the negated ones
    d1 = rng.integers(-126, 127, size=(C, A, B, 2))
    d2 = rng.choice([-128, -128, 5, 127], size=(C, A, B, 2))
    d3 = rng.choice([-128, -128, -1, 127], size=(C, A, B, 2))
    F = d1 * 65536 + d2 * 256 + d3
    w = (F / K).astype(f)
    keep = fixed(w) == F  # (RN32(F / K) * K rounds back to F nearly always; where not, the value is as good a coefficient)
    assert keep.mean() > 0.9
    return w


def _samples(rng, C, nT16, A):
    x = rng.integers(-128, 128, size=(C, nT16, A, 16, 2), dtype=np.int8)
    x[:, :, :, 0, :] = -128  # a full-scale column in every case
    x[:, :, :, 1, :] = 127
    x[:, :, :, 2, 0], x[:, :, :, 2, 1] = -128, 127
    return x


def test_digits_of_the_negated_number_are_not_the_negated_digits():
    """F = 128 = (0, 1, -128): -F = -128 = (0, 0, -128), while the negated digits (0, -1, 128) are no digits at all.  The
    model's third operand has the former: with one antenna, x = (0, 1), out_re is digit_d(F_in) itself."""
    assert [int(d) for d in digits(np.int64(128))] == [0, 1, -128]
    assert [int(d) for d in digits(np.int64(-128))] == [0, 0, -128]
    w = np.float32(128 / K)
    assert fixed(w) == 128 and fixed(-w) == -128
    coef = np.zeros((1, 1, 1, 2), np.float32)
    coef[..., 1] = w
    F_re, F_ip, F_in = (int(F.item()) for F in operands(coef))
    assert (F_re, F_ip, F_in) == (0, 128, -128)
    assert [int(d) for d in digits(np.int64(F_in))] != [-int(d) for d in digits(np.int64(F_ip))]
    x = np.zeros((1, 1, 1, 16, 2), np.int8)
    x[..., 1] = 1
    s1, s2, s3 = digit_sums(coef, x)
    assert [int(s[0, 0, 0, 0, 0]) for s in (s1, s2, s3)] == [0, 0, -128]  # digits(-F), not -digits(F) = (0, -1, 128)
    assert [int(s[0, 0, 0, 0, 1]) for s in (s1, s2, s3)] == [0, 0, 0]     # x_re = 0 and w_re = 0
    # ... and conjugated the operands change places
    assert tuple(int(F.item()) for F in operands(coef, conjugate=True)) == (0, -128, 128)
    s1, s2, s3 = digit_sums(coef, x, conjugate=True)
    assert [int(s[0, 0, 0, 0, 0]) for s in (s1, s2, s3)] == [0, 1, -128]
    # rint is odd and the clamp symmetric: fixed(-w) == -fixed(w) for every fp32 w
    rng = np.random.default_rng(3)
    ws = np.concatenate([_coefficients("halfway", rng, 1, 50, 20).ravel(), _coefficients("special", rng, 1, 10, 5).ravel()])
    assert np.array_equal(fixed(-ws), -fixed(ws))


def test_fma_tail_is_the_integer_tail_and_does_not_wrap():
    """low = fmaf((float)s2, 256.0f, (float)s3) against RN32 of the exact integer s2 * 256 + s3 (int64 -> fp32, and the
    rational rounding), on random sums up to the bound 2^23 and at the bound itself, where an int32 would wrap."""
    rng = np.random.default_rng(11)
    s2 = np.concatenate([rng.integers(-SUM_BOUND, SUM_BOUND + 1, 20000), rng.integers(-300, 300, 2000),
                         [SUM_BOUND, -SUM_BOUND, SUM_BOUND, -SUM_BOUND, SUM_BOUND - 1, 2 ** 22, 0]])
    s3 = np.concatenate([rng.integers(-SUM_BOUND, SUM_BOUND + 1, 20000), rng.integers(-SUM_BOUND, SUM_BOUND + 1, 2000),
                         [SUM_BOUND, -SUM_BOUND, -SUM_BOUND, SUM_BOUND, SUM_BOUND - 1, 2 ** 22, 0]])
    got = low_part(s2, s3)
    exact = s2 * 256 + s3  # int64
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exact.astype(np.float32).view(np.uint32))
    for i in list(range(0, 200)) + list(range(len(s2) - 7, len(s2))):
        assert got[i].view(np.uint32) == rn32(Fraction(int(exact[i]))).view(np.uint32), (int(s2[i]), int(s3[i]))
    # where the integer form fits an int32 the two forms are the same expression of the same integer; at the bound it does not
    top = SUM_BOUND * 256 + SUM_BOUND
    assert top == 2 ** 31 + 2 ** 23 and top > np.iinfo(np.int32).max
    with np.errstate(over="ignore"):
        wrapped = np.int32(SUM_BOUND) * np.int32(256) + np.int32(SUM_BOUND)
    assert int(wrapped) != top  # int32 arithmetic wraps here ...
    assert float(low_part(SUM_BOUND, SUM_BOUND)) == float(top) and float(low_part(-SUM_BOUND, -SUM_BOUND)) == -float(top)  # ... the model does not
    # the whole tail at that point, against the rational evaluation
    s1 = np.array([SUM_BOUND, -SUM_BOUND, 12345])
    b = np.array([SUM_BOUND, -SUM_BOUND, SUM_BOUND])
    v = recombine(s1, b, b)
    for i in range(3):
        f = rn32(65536 * int(s1[i]) + Fraction(float(rn32(Fraction(int(b[i]) * 257)))))
        assert v[i].view(np.uint32) == rn32(Fraction(float(f)) * Fraction(float(INV))).view(np.uint32)


def test_largest_sums_are_reached_and_fit():
    """256 antennas, every sample -128 and both products of one sign: |S_d| = 2 * 256 * 128 * 128 = 2^23 in the low digits."""
    A = 256
    F = -126 * 65536 - 128 * 256 - 128
    w0 = np.float32(F / K)
    cands = [w for w in (w0, np.nextafter(w0, np.float32(0)), np.nextafter(w0, np.float32(-2))) if fixed(w) == F]
    assert cands
    coef = np.full((1, A, 1, 2), cands[0], dtype=np.float32)
    x = np.full((1, 1, A, 16, 2), -128, dtype=np.int8)
    s1, s2, s3 = digit_sums(coef, x)  # out_im = sum F_re x_im + F_ip x_re: both products positive
    assert np.all(s2[..., 1] == SUM_BOUND) and np.all(s3[..., 1] == SUM_BOUND) and np.all(s1[..., 1] == 2 * 126 * 128 * A)
    v = complex_model(coef, x)
    exp = rn32(Fraction(float(rn32(Fraction(-F * 128 * 2 * A)))) * Fraction(float(INV)))
    assert np.all(v[..., 1] == exp) and np.all(np.isfinite(v))


def test_conjugate_is_the_model_on_negated_imaginary_parts():
    rng = np.random.default_rng(5)
    for kind in ("trig", "low128", "halfway"):
        coef = _coefficients(kind, rng, 2, 37, 5)
        x = _samples(rng, 2, 2, 37)
        neg = coef.copy()
        neg[..., 1] = -neg[..., 1]
        assert first_difference(complex_model(coef, x, conjugate=True), complex_model(neg, x)) is None
        assert first_difference(complex_model(coef, x, conjugate=True), complex_model(coef, x)) is not None


@pytest.mark.parametrize("kind", ["trig", "special", "halfway", "low128"])
@pytest.mark.parametrize("A", [1, 3, 64, 65, 256])
@pytest.mark.parametrize("conjugate", [False, True])
def test_complex_model_against_rational_arithmetic_and_the_derived_bound(A, kind, conjugate):
    """complex_model, per output element and component, against Python integers and fractions.

    (1) The integer part: 65536 * s1 + 256 * s2 + s3 == S, with
            S_re = sum_a F_re x_re + F_in x_im,   S_im = sum_a F_re x_im + F_ip x_re,
        F_re = fixed(w_re), F_ip = fixed(sigma w_im), F_in = fixed(-sigma w_im) evaluated in rational arithmetic, and the
        fp32 tail is exactly RN32(RN32(65536 * s1 + RN32(256 * s2 + s3)) * RN32(1 / K)).

    (2) The distance from the exact sum E of the fp32 coefficients, E_re = sum_a w_re x_re - sigma w_im x_im, E_im = sum_a
    w_re x_im + sigma w_im x_re -- tests/test_beamformer_model.py's derivation with both sample components in the sum
    (u = 2^-24):
      * quantisation: every product's coefficient is within q of its fixed-point number, q = 3/4 for |w| <= 1 and
        K (|w| - 1) beyond (fixed(-w) = -fixed(w), so the negated operand is as close as the other): a component has two
        products per antenna, |S / K - E| <= sum_a (q_1a |x_1a| + q_2a |x_2a|) / K;
      * the three roundings, as there: |r - S / K| <= |S| / K * ((1 + u)^3 - 1) + |L| u (1 + u)^3 / K, L = 256 s2 + s3.
    bound = sum_a (q_1a |x_1a| + q_2a |x_2a|) / K + |L| u (1 + u)^3 / K + |S| ((1 + u)^3 - 1) / K, asserted in rational
    arithmetic with no factor on top.  In closed form, for |w| <= 1: |L| <= 128 * 257 * sum_a (|x_re| + |x_im|) and
    |S| / K <= |E| + 0.75 / K * sum_a (|x_re| + |x_im|), so bound <= 9e-8 * sum_a (|x_re| + |x_im|) + 1.8e-7 * |E|: the
    figure include/dcs_beam_complex.h quotes."""
    rng = np.random.default_rng(1000 * A + len(kind) + conjugate)
    C, B, nT16 = 1, 2, 1
    sigma = -1 if conjugate else 1
    coef = _coefficients(kind, rng, C, A, B)
    x = _samples(rng, C, nT16, A)
    s1, s2, s3 = digit_sums(coef, x, conjugate)
    got = complex_model(coef, x, conjugate)
    assert got.dtype == np.float32 and got.shape == (C, nT16, B, 16, 2)
    inv = Fraction(float(INV))
    growth = (1 + U) ** 3
    for b in range(B):
        w_re = [Fraction(float(coef[0, a, b, 0])) for a in range(A)]
        w_im = [sigma * Fraction(float(coef[0, a, b, 1])) for a in range(A)]
        F_re = [fixed_exact(float(w)) for w in w_re]
        F_ip = [fixed_exact(float(w)) for w in w_im]
        F_in = [fixed_exact(float(-w)) for w in w_im]
        assert F_in == [-F for F in F_ip]
        q_re = [Fraction(3, 4) if abs(w) <= 1 else K * (abs(w) - 1) for w in w_re]
        q_im = [Fraction(3, 4) if abs(w) <= 1 else K * (abs(w) - 1) for w in w_im]
        for i in range(16):
            xr = [int(v) for v in x[0, 0, :, i, 0]]
            xi = [int(v) for v in x[0, 0, :, i, 1]]
            mag = sum(abs(v) for v in xr) + sum(abs(v) for v in xi)
            for k in range(2):
                if k == 0:
                    S = sum(fr * r + fn * m for fr, fn, r, m in zip(F_re, F_in, xr, xi))
                    E = sum(wr * r - wi * m for wr, wi, r, m in zip(w_re, w_im, xr, xi))
                    quant = sum(qr * abs(r) + qi * abs(m) for qr, qi, r, m in zip(q_re, q_im, xr, xi))
                else:
                    S = sum(fr * m + fp * r for fr, fp, r, m in zip(F_re, F_ip, xr, xi))
                    E = sum(wr * m + wi * r for wr, wi, r, m in zip(w_re, w_im, xr, xi))
                    quant = sum(qr * abs(m) + qi * abs(r) for qr, qi, r, m in zip(q_re, q_im, xr, xi))
                i1, i2, i3 = int(s1[0, 0, b, i, k]), int(s2[0, 0, b, i, k]), int(s3[0, 0, b, i, k])
                assert 65536 * i1 + 256 * i2 + i3 == S
                L = 256 * i2 + i3
                f = rn32(65536 * i1 + Fraction(float(rn32(L))))
                r = rn32(Fraction(float(f)) * inv)
                assert r.view(np.uint32) == got[0, 0, b, i, k].view(np.uint32), (b, i, k)
                bound = (quant + abs(L) * U * growth + abs(S) * (growth - 1)) / K
                err = abs(Fraction(float(r)) - E)
                assert err <= bound, (b, i, k, float(err), float(bound))
                if kind != "special":  # |w| <= 1: the header's closed form
                    assert bound <= Fraction(9, 10 ** 8) * mag + Fraction(18, 10 ** 8) * abs(E)
                    assert err <= Fraction(9, 10 ** 8) * mag + Fraction(18, 10 ** 8) * abs(E)


def test_weighted_scale_and_non_finite_rows():
    rng = np.random.default_rng(7)
    C, A, B = 2, 37, 5
    coef = _coefficients("trig", rng, C, A, B)
    x = _samples(rng, C, 2, A)
    ones = np.ones((B, A), np.float32)
    s, gh = normalise(ones)
    assert first_difference(complex_model(weighted_coefficients(coef, gh), x, scale=s), complex_model(coef, x)) is None
    s, gh = normalise(ones * np.float32(8))
    assert first_difference(complex_model(weighted_coefficients(coef, gh), x, scale=s), complex_model(coef, x) * np.float32(8)) is None
    w = (rng.choice([-1.0, 1.0], size=(B, A)) * 10.0 ** rng.uniform(-3, 3, size=(B, A))).astype(np.float32)
    w[2] = 0
    s, gh = normalise(w)
    wc = weighted_coefficients(coef, gh)
    got = complex_model(wc, x, scale=s)
    assert np.all(got[:, :, 2] == 0) and np.all(np.isfinite(got))
    s1, s2, s3 = digit_sums(wc, x)
    for b in range(B):
        fac = rn32(Fraction(float(s[b])) * Fraction(float(INV)))
        for idx in ((0, 0, b, 0, 0), (1, 1, b, 7, 1)):
            L = 256 * int(s2[idx]) + int(s3[idx])
            f = rn32(65536 * int(s1[idx]) + Fraction(float(rn32(L))))
            assert rn32(Fraction(float(f)) * Fraction(float(fac))).view(np.uint32) == got[idx].view(np.uint32)
    # a non-finite coefficient in EITHER component: NaN in both planes of that beam (and channel), nothing else
    ref = complex_model(coef, x)
    for plane, bad in ((0, np.nan), (1, np.inf)):
        c2 = coef.copy()
        c2[1, 5, 3, plane] = bad
        v = complex_model(c2, x)
        assert np.all(np.isnan(v[1, :, 3])) and not np.isnan(v[0]).any() and not np.isnan(np.delete(v[1], 3, axis=1)).any()
        v[1, :, 3] = ref[1, :, 3]
        assert first_difference(v, ref) is None
