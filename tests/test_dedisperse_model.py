"""The numpy model of the dedispersion (helpers/dedisperse_model.py) anchored without a device: the delays against exact
rational arithmetic of the header's formula, rounded once per operation, and the plane against a triple Python loop."""
from fractions import Fraction

import numpy as np
import pytest

from helpers.dedisperse_model import (BAND_ASCENDING_100, BAND_DESCENDING_64, DMS_40, INT32_MAX, INT32_MIN, K_DM, dedisperse,
                                      dm_delays, smooth_table, takes_part)


def rn(x):
    """The double nearest to a rational, ties to even: int / int true division is correctly rounded."""
    return float(x)


def exact_delay(C, first, step, ts, dm, j):
    """include/dcs_dedisperse.h, one Fraction operation and one rounding per line."""
    def f_of(i):
        return rn(Fraction(first) + Fraction(rn(Fraction(i) * Fraction(step))))

    f = f_of(j)
    f_ref = first if step <= 0 else f_of(C - 1)
    a = rn(1 / Fraction(rn(Fraction(f) * Fraction(f))))
    b = rn(1 / Fraction(rn(Fraction(f_ref) * Fraction(f_ref))))
    if dm != dm:
        return INT32_MAX
    if dm in (float("inf"), float("-inf")):
        pytest.fail("the rational check takes finite DMs only")
    k = rn(Fraction(K_DM) * Fraction(dm))
    diff = rn(Fraction(a) - Fraction(b))
    q = Fraction(rn(Fraction(k) * Fraction(diff))) / Fraction(ts)
    if abs(q) > Fraction(2) ** 1000:  # RN would be an infinity
        return INT32_MAX if q > 0 else INT32_MIN
    s = rn(q)
    if s > 2147483647:
        return INT32_MAX
    if s < -2147483648:
        return INT32_MIN
    return round(s)  # a float's round() goes to the nearest integer, ties to even


BANDS = [(64,) + BAND_DESCENDING_64, (100,) + BAND_ASCENDING_100, (5, 1400.0, 0.0, 64e-6), (1, 600.0, -1.0, 1e-3),
         (3, 0.1, 0.3, 1e-6)]
DMS = [0.0, 2.5, 97.5, 1.0 / 3.0, -7.25, float("nan"), 1e300, -1e300, 5e12, 4.9e-324]


@pytest.mark.parametrize("C,first,step,ts", BANDS)
def test_delays_are_the_formula_rounded_once_per_operation(C, first, step, ts):
    got = dm_delays(C, first, step, ts, DMS)
    assert got.dtype == np.int32 and got.shape == (len(DMS), C)
    for m, dm in enumerate(DMS):
        for j in range(C):
            assert int(got[m, j]) == exact_delay(C, first, step, ts, dm, j), (m, j)


def test_delay_edges():
    for C, first, step, ts in BANDS:
        got = dm_delays(C, first, step, ts, DMS)
        ref = 0 if step <= 0 else C - 1
        assert np.all(got[0] == 0), "DM 0"
        assert np.all(got[5] == INT32_MAX), "a NaN DM"
        finite = [m for m, dm in enumerate(DMS) if dm == dm and abs(dm) < 1e200]
        assert np.all(got[finite, ref] == 0), "the reference column"
        assert np.all(got[[1, 2, 3]] >= 0) and np.all(got[4] <= 0)
        if step != 0.0 and C > 1:
            other = np.arange(C) != ref
            assert np.all(got[6][other] == INT32_MAX) and np.all(got[7][other] == INT32_MIN)
    # a zero-step band: every column is the reference
    assert not dm_delays(5, 1400.0, 0.0, 64e-6, [0.0, 50.0, -3.0]).any()


@pytest.mark.parametrize("C,band", [(64, BAND_DESCENDING_64), (100, BAND_ASCENDING_100)])
def test_the_two_bands_of_the_gpu_tests(C, band):
    d = dm_delays(C, *band, DMS_40)
    assert d.min() == 0 and 1300 <= d.max() <= 1340, d.max()
    assert np.all(np.diff(d, axis=0) >= 0), "monotone in the DM"
    assert {int(r) for r in np.unique(d % 4)} == {0, 1, 2, 3}
    low = 0 if band[1] > 0 else C - 1  # the lowest frequency has the largest delay
    assert d[-1, low] == d.max()


def loops(fb, delays, first, T, max_delay, mask):
    B, _, C = fb.shape
    out = [[[0] * T for _ in range(delays.shape[0])] for _ in range(B)]
    for b in range(B):
        for m in range(delays.shape[0]):
            for t in range(T):
                total = 0
                for c in range(C):
                    d = int(delays[m, c])
                    if (mask is None or mask[c] != 0) and 0 <= d <= max_delay:
                        total += int(fb[b, first + t + d, c])
                out[b][m][t] = total % 2**32
    return np.array(out, dtype=np.uint32)


def test_plane_is_the_triple_loop():
    rng = np.random.default_rng(5)
    B, C, T, first, max_delay = 2, 5, 7, 2, 9
    fb = rng.integers(0, 256, size=(B, first + T + max_delay, C), dtype=np.uint8)
    delays = rng.integers(0, max_delay + 1, size=(6, C)).astype(np.int32)
    delays[1, 2], delays[2, 0], delays[3, 4], delays[4, 1] = -1, INT32_MIN, max_delay + 1, INT32_MAX
    delays[5] = [-1, INT32_MAX, max_delay + 1, INT32_MIN, -5]  # a DM whose every term drops
    for mask in (None, np.array([1, 0, 255, 1, 0], np.uint8), np.zeros(C, np.uint8)):
        got = dedisperse(fb, delays, first, T, max_delay, mask)
        exp = loops(fb, delays, first, T, max_delay, mask)
        assert got.dtype == np.uint32 and np.array_equal(got, exp)
        assert not got[:, 5].any()
        if mask is not None and not mask.any():
            assert not got.any()
    assert takes_part(delays, max_delay).sum() == 6 * C - 4 - C
    # into a prefilled plane at an offset: no other word changes
    pre = np.full((B, 6, T + 5), 0xDEADBEEF, np.uint32)
    got = dedisperse(fb, delays, first, T, max_delay, out=pre, first_out=3)
    assert np.array_equal(got[:, :, 3:3 + T], loops(fb, delays, first, T, max_delay, None))
    assert np.all(got[:, :, :3] == 0xDEADBEEF) and np.all(got[:, :, 3 + T:] == 0xDEADBEEF)


def test_smooth_tables():
    for C in (1, 3, 17, 257):
        t = smooth_table(C, 7, 600, seed=C)
        assert t.dtype == np.int32 and t.min() == 0 and t.max() == 600 and np.all(np.diff(t, axis=0) >= 0)
        if C > 1:
            assert np.all(np.diff(t, axis=1) <= 0) and np.all(t[:, -1] == 0)
