"""The inputs of tests/test_gpu_beam_complex_edges.py, checked without a GPU (tests/helpers/complex_edges.py): the weighted
construction takes the model's S2 * 256 + S3 beyond int32, where the fma low part of include/dcs_beam_complex.h and the
integer form differ -- also on coefficients one ULP off, which is what a generator within 1 ULP may return -- and no
unweighted input can."""
import numpy as np
import pytest

from helpers import complex_edges as ce
from helpers.beam_complex_model import SUM_BOUND, complex_model, digit_sums
from helpers.beamformer_model import F32, digits, first_difference, fixed, normalise, weighted_coefficients

C, A, B = 2, 256, 17
DRIVEN = (3, 16)


def one_ulp_off(coef, kind):
    """The stand-in coefficients with one component of every pair moved one ULP up or down, or each component by a seeded
    -1 / 0 / +1 ULP of its own."""
    bits = coef.view(np.int32).copy()  # positive numbers: the next fp32 is the next integer
    assert np.all(coef > 0)
    if kind == "seeded":
        bits += np.random.default_rng(8).integers(-1, 2, size=bits.shape, dtype=np.int32)
    elif kind is not None:
        plane, step = kind
        bits[..., plane] += step
    return bits.view(F32)


def samples():
    """Block 0 all -128, block 1 seeded random."""
    x = np.random.default_rng(2).integers(-128, 128, size=(C, 2, A, 16, 2), dtype=np.int8)
    x[:, 0] = -128
    return x


@pytest.mark.parametrize("kind", [None, (0, 1), (0, -1), (1, 1), (1, -1), "seeded"], ids=str)
def test_weighted_construction_leaves_int32_and_the_two_low_parts_differ_there(kind):
    coef = one_ulp_off(ce.standin_coefficients(C, A, B), kind)
    gains = ce.wrap_gains(coef, DRIVEN)
    w = ce.wrap_weights(coef, DRIVEN)
    s, gh = normalise(w)
    assert np.all(s == 1) and np.array_equal(gh, w) and all(w[b, 0] == 1 and np.all(w[b, 1:] == g) for b, g in gains.items())
    wc = weighted_coefficients(coef, gh)
    x = samples()
    for conj in (False, True):
        s1, s2, s3 = digit_sums(wc, x, conj)
        assert max(int(np.abs(v).max()) for v in (s1, s2, s3)) <= SUM_BOUND
        low = ce.exact_low(s2, s3)
        fits = np.abs(low) <= ce.INT32_MAX
        v, v32 = complex_model(wc, x, conj, scale=s), ce.int32_model(wc, x, conj, scale=s)
        assert np.all(np.isfinite(v))
        plane = 0 if conj else 1
        for b in DRIVEN:
            assert np.all(low[:, 0, b, :, plane] > ce.INT32_MAX), (kind, conj, b, int(low[:, 0, b].max()))
            assert np.all(v[:, 0, b, :, plane] != v32[:, 0, b, :, plane]) and np.all(v[:, 0, b, :, plane] < -40000)
        # nothing else leaves int32 (the other plane of the driven beams stays just inside), and there the two forms agree
        others = np.ones(B, dtype=bool)
        others[list(DRIVEN)] = False
        assert np.all(fits[:, :, others]) and np.all(fits[:, 1]) and np.all(fits[:, 0, :, :, 1 - plane])
        assert np.array_equal(v.view(np.uint32)[fits], v32.view(np.uint32)[fits]) and not np.any(v.view(np.uint32)[~fits] == v32.view(np.uint32)[~fits])
        assert low.min() >= -2 ** 31
        print(f"{kind}, conjugate {conj}: g = {float(gains[3])!r}, largest exact low {int(low.max())} = 2^31 + {int(low.max()) - 2 ** 31}, "
              f"value {float(v[0, 0, 3, 0, plane])!r}, with the int32 form {float(v32[0, 0, 3, 0, plane])!r}")
    # the driven weights negated: the same integers negated, and no low part below int32
    wn = ce.wrap_weights(coef, DRIVEN, sign=-1.0)
    sn, ghn = normalise(wn)
    assert np.all(sn == 1) and np.array_equal(ghn, wn)
    wcn = weighted_coefficients(coef, ghn)
    for conj in (False, True):
        p = digit_sums(wc, x, conj)
        n = digit_sums(wcn, x, conj)
        total = lambda q: q[0] * 65536 + q[1] * 256 + q[2]
        assert np.array_equal(total(n)[:, :, list(DRIVEN)], -total(p)[:, :, list(DRIVEN)])
        assert ce.exact_low(n[1], n[2]).min() >= -2 ** 31
        # ... in fact none outside int32 on either side, so that pass tells the two forms apart nowhere
        assert np.abs(ce.exact_low(n[1], n[2])).max() <= ce.INT32_MAX
        assert first_difference(complex_model(wcn, x, conj, scale=sn), ce.int32_model(wcn, x, conj, scale=sn)) is None


def test_construction_names_the_condition_that_fails():
    coef = ce.standin_coefficients(1, 8, 2)
    bad = coef.copy()
    bad[:, 0] = coef[:, 1]
    with pytest.raises(ValueError, match="antenna 0.*change the inputs"):
        ce.wrap_gains(bad, (1,))
    bad = coef.copy()
    bad[:, 1:, :, 0] = np.linspace(0.1, 0.9, 7, dtype=F32)[None, :, None]
    with pytest.raises(ValueError, match="none of the|share a few"):
        ce.wrap_gains(bad, (0,))
    rng = np.random.default_rng(0)
    bad[:, 1:] = rng.uniform(0.1, 0.9, size=bad[:, 1:].shape).astype(F32)
    with pytest.raises(ValueError, match="change the inputs"):
        ce.wrap_gains(bad, (0,))


def test_int32_low_part_wraps_as_int32_does():
    s2 = np.array([SUM_BOUND, -SUM_BOUND, 8387456, 5, -7, 2 ** 23 - 1])
    s3 = np.array([SUM_BOUND, -SUM_BOUND, 7197312, -3, 100, 255])
    with np.errstate(over="ignore"):
        exp = (s2.astype(np.int32) * np.int32(256) + s3.astype(np.int32)).astype(F32)
    got = ce.int32_low_part(s2, s3)
    assert got.dtype == F32 and np.array_equal(got, exp)
    assert got[2] == -2140581248.0 and ce.exact_low(s2, s3)[2] == 2154386048


def test_no_unweighted_input_leaves_int32():
    """Over 10^7 seeded fp32 phases: no unit-modulus coefficient has the middle digit -128 in both components, and 256
    antennas of the worst coefficient found, with the worst samples for it, keep |S2 * 256 + S3| below 2^31.  Per antenna
    and plane the low part is x_1 * l(F_re) + x_2 * l(F_ip or F_in), l = 256 * d2 + d3, x in [-128, 127]: its largest value
    of either sign is h(l_1) + h(l_2) resp. h(-l_1) + h(-l_2), h(l) = max(127 * l, -128 * l)."""
    rng = np.random.default_rng(20261019)
    joint, worst = 0, 0
    h = lambda l: np.maximum(127 * l, -128 * l)
    for _ in range(10):
        p = rng.uniform(-np.pi, np.pi, 10 ** 6).astype(F32).astype(np.float64)
        F_re, F_im = fixed(np.cos(p).astype(F32)), fixed(np.sin(p).astype(F32))
        low, mid = {}, {}
        for name, F in (("re", F_re), ("im", F_im), ("-im", -F_im)):
            _, mid[name], d3 = digits(F)
            low[name] = 256 * mid[name] + d3
        joint += int(np.count_nonzero((mid["re"] == -128) & ((mid["im"] == -128) | (mid["-im"] == -128))))
        for other in ("im", "-im"):  # F_ip and F_in, whichever the conjugate flag makes them
            worst = max(worst, int(np.maximum(h(low["re"]) + h(low[other]), h(-low["re"]) + h(-low[other])).max()))
    print(f"largest unweighted |S2 * 256 + S3| at 256 antennas: {256 * worst} = 2^31 - {2 ** 31 - 256 * worst}")
    assert joint == 0
    assert 256 * worst < 2 ** 31
