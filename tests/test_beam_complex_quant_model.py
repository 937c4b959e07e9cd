"""The contract of include/dcs_beam_complex_quant.h on the CPU: its expectation is quantise() of helpers/beam_quant_model.py
applied to complex_model() of helpers/beam_complex_model.py -- both anchored against exact arithmetic by their own tests
(tests/test_beam_quant_model.py, tests/test_beam_complex_model.py), so no new model exists.  Here: the composition at its
extremes (the largest sums, NaN rows, the conjugate), the binding's place in the package, and the two-stage use the int8
tensor is laid out for -- quantised beams as the samples of a second complex product -- against rational arithmetic.
No GPU."""
from fractions import Fraction

import numpy as np

from helpers.beam_complex_model import SUM_BOUND, complex_model, digit_sums
from helpers.beam_quant_model import gains_without_clipping, quantise
from helpers.beamformer_model import FIX_SCALE, digits, fixed
from test_beam_complex_model import _coefficients, _samples

K = FIX_SCALE


def _with_fixed(F):
    """An fp32 number whose fixed-point number is F."""
    w0 = np.float32(F / K)
    for w in (w0, np.nextafter(w0, np.float32(0)), np.nextafter(w0, np.float32(-2)), np.nextafter(w0, np.float32(2))):
        if fixed(w) == F:
            return w
    raise AssertionError(F)


def test_largest_sums_saturate_every_component_and_count_them():
    """256 antennas, every sample -128, coefficients whose low digits are all -128 (re) and all -128 / -127 (the negated
    operand of im): the digit sums reach 2^23, the floats stay finite, and with unit gains every component is beyond 127."""
    A, C, nT16 = 256, 2, 2
    F_re = [-126 * 65536 - 128 * 256 - 128, -100 * 65536 - 128 * 256 - 128, -126 * 65536 - 128 * 256 - 128]
    F_im = [-63 * 65536 - 128 * 256 - 128, -31 * 65536 - 128 * 256 - 128, 63 * 65536 + 127 * 256 + 127]
    B = len(F_re)
    coef = np.empty((C, A, B, 2), np.float32)
    for b in range(B):
        coef[:, :, b, 0], coef[:, :, b, 1] = _with_fixed(F_re[b]), _with_fixed(F_im[b])
    assert [int(d) for d in digits(np.int64(-F_im[0]))] == [64, -127, -128]  # the negated NUMBER's digits
    x = np.full((C, nT16, A, 16, 2), -128, np.int8)
    for conj in (False, True):
        s1, s2, s3 = digit_sums(coef, x, conj)
        assert max(int(np.abs(s).max()) for s in (s2, s3)) == SUM_BOUND  # the bound is reached ...
        v = complex_model(coef, x, conj)
        assert np.all(np.isfinite(v)) and np.abs(v).min() > 127.5        # ... the floats are finite, and all beyond the range
        q, n = quantise(v, np.ones(B, np.float32))
        assert np.all(np.abs(q.astype(np.int16)) == 127) and np.array_equal(q > 0, v > 0)
        assert np.all(n == C * nT16 * 16 * 2), n
        # the same with gains large enough to overflow the product: +-Inf clamps to +-127 as well
        q2, n2 = quantise(v, np.full(B, 3e38, np.float32))
        assert np.array_equal(q2, q) and np.array_equal(n2, n)


def test_a_non_finite_coefficient_component_is_minus_128_in_both_planes():
    rng = np.random.default_rng(21)
    C, A, B = 2, 37, 5
    coef = _coefficients("trig", rng, C, A, B)
    x = _samples(rng, C, 2, A)
    ref = complex_model(coef, x)
    k = gains_without_clipping(ref)
    q_ref, n_ref = quantise(ref, k)
    assert n_ref.sum() == 0 and not np.any(q_ref == -128)
    for plane, bad in ((0, np.nan), (1, np.inf), (1, np.nan)):
        c2 = coef.copy()
        c2[:, 5, 3, plane] = bad
        q, n = quantise(complex_model(c2, x), k)
        assert np.all(q[:, :, 3] == -128), (plane, bad)  # both planes, every sample
        assert n[3] == C * 2 * 16 * 2 and np.all(np.delete(n, 3) == 0)
        others = [b for b in range(B) if b != 3]
        assert np.array_equal(q[:, :, others], q_ref[:, :, others])


def test_the_conjugate_changes_both_planes_of_the_bytes():
    rng = np.random.default_rng(22)
    coef = _coefficients("trig", rng, 2, 64, 7)
    x = _samples(rng, 2, 2, 64)
    v, vc = complex_model(coef, x), complex_model(coef, x, conjugate=True)
    k = gains_without_clipping(np.concatenate([v, vc], axis=1))
    q, _ = quantise(v, k)
    qc, _ = quantise(vc, k)
    assert np.mean(q[..., 0] != qc[..., 0]) > 0.5 and np.mean(q[..., 1] != qc[..., 1]) > 0.5


def test_two_stages_beams_of_quantised_beams_against_rational_arithmetic():
    """Stage 1: 64 antennas -> 32 conjugate beams, quantised with gains that cannot clip.  Those bytes are, as they lie, the
    sample tensor [C][nt / 16][A2 = 32][16][2] of stage 2 (32 inputs -> 5 beams).  Stage 2's model output against the exact
    rational sum_a conj(w_a) x_a of its fp32 coefficients on the same bytes, within the bound include/dcs_beam_complex.h
    states: 9e-8 * sum_a (|x_re| + |x_im|) + 1.8e-7 * |exact| per component."""
    rng = np.random.default_rng(23)
    C, nT16, A1, B1, B2 = 2, 1, 64, 32, 5
    x1 = _samples(rng, C, nT16, A1)
    v1 = complex_model(_coefficients("trig", rng, C, A1, B1), x1, conjugate=True)
    q1, n1 = quantise(v1, gains_without_clipping(v1))
    assert n1.sum() == 0 and q1.dtype == np.int8 and q1.shape == (C, nT16, B1, 16, 2) and np.unique(q1).size >= 100
    coef2 = _coefficients("trig", rng, C, B1, B2)
    v2 = complex_model(coef2, q1, conjugate=True)
    assert v2.shape == (C, nT16, B2, 16, 2) and np.all(np.isfinite(v2))
    worst = Fraction(0)
    for c in range(C):
        for b in range(B2):
            w = [(Fraction(float(coef2[c, a, b, 0])), -Fraction(float(coef2[c, a, b, 1]))) for a in range(B1)]  # conj(w)
            for i in range(16):
                xs = [(int(q1[c, 0, a, i, 0]), int(q1[c, 0, a, i, 1])) for a in range(B1)]
                mag = sum(abs(r) + abs(m) for r, m in xs)
                E = (sum(wr * r - wi * m for (wr, wi), (r, m) in zip(w, xs)), sum(wr * m + wi * r for (wr, wi), (r, m) in zip(w, xs)))
                for k in range(2):
                    err = abs(Fraction(float(v2[c, 0, b, i, k])) - E[k])
                    bound = Fraction(9, 10 ** 8) * mag + Fraction(18, 10 ** 8) * abs(E[k])
                    assert err <= bound, (c, b, i, k, float(err), float(bound))
                    worst = max(worst, err / bound)
    assert worst > 0  # (the model is not the exact sum: something was compared)


def test_the_binding_and_the_table_row_exist_without_a_built_library():
    from dc_sand_amd.companions import COMPANIONS
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    row = COMPANIONS["beam_complex_quant"]
    assert (row.header, row.source, row.lib) == ("dcs_beam_complex_quant.h", "bf_beam_complex_quant.cpp", "libdcs_beam_complex_quant.so")
    assert [s[0] for s in row.signatures] == ["dcs_bf_beamform_accumulated_complex_q8", "dcs_bf_beamform_accumulated_complex_q8_dt"]
    assert callable(SteeringCoefficientGenerator.beamform_accumulated_complex_q8)
