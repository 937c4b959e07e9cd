"""The numpy model of the RFI flagger (helpers/rfi_model.py; include/dcs_rfi.h) anchored on plain Python integers: sums with
int, medians with sorted(), the limit compared through fractions.Fraction, so that no float rounding of the test's own can
agree with the model's by accident.  Then the seeded recipe and what the model makes of it, stated as facts.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import rfi_model as rm


def lmed(values):
    s = sorted(int(v) for v in values)
    return s[(len(s) - 1) >> 1]


def outliers_exact(values, thr, floor):
    """The header's test in exact arithmetic: RN64(thr * mad) is the one rounding, made by Python's float multiply of two
    doubles; the compare is between exact rationals."""
    v = [int(x) for x in values]
    med = lmed(v)
    d = [abs(x - med) for x in v]
    mad = lmed(d)
    assert mad < 1 << 53 and all(x < 1 << 53 for x in d)
    prod = float(thr) * float(mad)
    limit = max(prod, float(floor))
    if limit == float("inf"):
        return [False] * len(v)
    return [Fraction(x) > Fraction(limit) for x in d]


@pytest.mark.parametrize("K", [1, 2, 3, 4, 7, 8, 31, 32])
@pytest.mark.parametrize("thr,floor", [(0.0, 0.0), (0.0, 2.5), (1.0, 0.0), (2.0, 0.0), (6.0, 0.0), (6.0, 40.0), (1e300, 0.0), (1.4826, 0.0)])
def test_outliers_against_python_integers(K, thr, floor):
    rng = np.random.default_rng(1000 * K + int(thr * 10) + int(floor))
    for hi in (2, 3, 256, 1 << 24, 1 << 49):  # two values only: ties; then wider and wider
        v = rng.integers(0, hi, size=K, dtype=np.uint64)
        assert rm.lower_median(v)[0] == lmed(v)
        assert rm.outliers(v, thr, floor).tolist() == outliers_exact(v, thr, floor), (K, hi, v)


def test_lower_median_of_even_and_odd_counts():
    assert rm.lower_median(np.array([5, 1, 9, 3], np.uint64))[0] == 3      # rank 1 of 1 3 5 9
    assert rm.lower_median(np.array([5, 1, 9, 3, 7], np.uint64))[0] == 5   # rank 2 of 1 3 5 7 9
    assert rm.lower_median(np.array([4], np.uint64))[0] == 4
    assert rm.lower_median(np.array([2, 1], np.uint64))[0] == 1
    assert rm.lower_median(np.array([[2, 1], [7, 9]], np.uint64)).tolist() == [[1], [7]]


def test_mad_zero_and_thr_zero():
    v = np.array([10, 10, 10, 10, 11, 3], np.uint64)  # med 10, d = 0 0 0 0 1 7, mad 0
    assert rm.outliers(v, 6.0, 0.0).tolist() == [False, False, False, False, True, True]   # limit 0: every d > 0
    assert rm.outliers(v, 6.0, 1.0).tolist() == [False, False, False, False, False, True]  # the floor holds: 1 > 1 is false
    assert rm.outliers(v, 6.0, 7.0).tolist() == [False] * 6
    w = np.array([0, 4, 8, 12, 16], np.uint64)  # med 8, d = 8 4 0 4 8, mad 4
    assert rm.outliers(w, 0.0, 0.0).tolist() == [True, True, False, True, True]
    assert rm.outliers(np.array([9], np.uint64), 0.0, 0.0).tolist() == [False]  # K = 1: d = 0


def test_the_compare_is_strict():
    v = np.array([0, 4, 8, 12, 16], np.uint64)  # mad 4: thr 2 gives the limit 8 = d of both ends
    assert rm.outliers(v, 2.0, 0.0).tolist() == [False] * 5
    assert rm.outliers(v, np.nextafter(2.0, 0.0), 0.0).tolist() == [True, False, False, False, True]
    assert outliers_exact(v, 2.0, 0.0) == [False] * 5


def test_moments_of_small_blocks_against_python_integers():
    rng = np.random.default_rng(5)
    fb = rng.integers(0, 256, size=(2, 11, 5), dtype=np.uint8)
    cs, z = rm.moments(fb, 2, 3, 3)
    assert cs.shape == (2, 3, 5, 2) and cs.dtype == np.uint32 and z.shape == (2, 9) and z.dtype == np.uint32
    for b in range(2):
        for k in range(3):
            for c in range(5):
                col = [int(x) for x in fb[b, 2 + 3 * k:5 + 3 * k, c]]
                assert cs[b, k, c].tolist() == [sum(col), sum(x * x for x in col)]
        for t in range(9):
            assert z[b, t] == sum(int(x) for x in fb[b, 2 + t])


def test_extremes_of_a_block_of_65536():
    n = 65536
    full = np.full((1, n, 2), 255, np.uint8)
    cs, z = rm.moments(full, 0, 1, n)
    assert cs[0, 0, 0].tolist() == [n * 255, 4_261_478_400] and 4_261_478_400 < 1 << 32 and np.all(z == 510)
    s1, s2 = int(cs[0, 0, 0, 0]), int(cs[0, 0, 0, 1])
    assert n * s2 - s1 * s1 == 0 and n * s2 < 1 << 49 and s1 * s1 < 1 << 48
    half = np.zeros((1, n, 2), np.uint8)
    half[0, ::2] = 255
    cs, _ = rm.moments(half, 0, 1, n)
    s1, s2 = int(cs[0, 0, 0, 0]), int(cs[0, 0, 0, 1])
    q = n * s2 - s1 * s1
    assert (s1, s2) == (n // 2 * 255, n // 2 * 255 * 255) and q == (n * 255 // 2) ** 2 and q < 1 << 49  # the largest q there is
    # the model's q is this integer: both channels equal, so neither is an outlier, and with a dead one beside it is
    cell, mask, spectrum, counts = rm.flags(cs, None, n, rm.Thresholds())
    assert not cell.any() and mask.all() and spectrum is None and counts.tolist() == [[0, 0, 0]]
    cs3 = np.concatenate([cs, np.array([[[[128 * n, 128 * 128 * n]]]], np.uint32)], axis=2)
    assert cs3.shape == (1, 1, 3, 2)
    cell, mask, _, counts = rm.flags(cs3, None, n, rm.Thresholds(mean_floor=1e300, var_floor=1e300))
    assert not cell.any()
    cell, mask, _, counts = rm.flags(cs3, None, n, rm.Thresholds())  # two of three alike: mad 0, the third is out on both
    assert cell.tolist() == [[[0, 0, 3]]] and mask.tolist() == [[1, 1, 0]] and counts.tolist() == [[1, 1, 0]]


def test_flags_against_python_integers():
    rng = np.random.default_rng(6)
    B, nb, n, C = 2, 3, 8, 9
    fb = rng.integers(100, 140, size=(B, nb * n, C), dtype=np.uint8)
    fb[0, :, 4] = 120
    fb[1, 5] = 255
    cs, z = rm.moments(fb, 0, nb, n)
    thr = rm.Thresholds(mean_thr=3.0, var_thr=2.0, var_floor=100.0, zero_dm_thr=4.0, max_bad_blocks=1)
    cell, mask, spectrum, counts = rm.flags(cs, z, n, thr)
    for b in range(B):
        bad = [0] * C
        for k in range(nb):
            m = [int(cs[b, k, c, 0]) for c in range(C)]
            q = [n * int(cs[b, k, c, 1]) - int(cs[b, k, c, 0]) ** 2 for c in range(C)]
            assert min(q) >= 0
            fm, fq = outliers_exact(m, 3.0, 0.0), outliers_exact(q, 2.0, 100.0)
            assert cell[b, k].tolist() == [int(x) | (int(y) << 1) for x, y in zip(fm, fq)]
            bad = [x + (1 if f else 0) for x, f in zip(bad, cell[b, k])]
        assert mask[b].tolist() == [0 if x > 1 else 1 for x in bad]
        assert spectrum[b].tolist() == [int(x) for x in outliers_exact(z[b], 4.0, 0.0)]
        assert counts[b].tolist() == [sum(bad), sum(1 for x in bad if x > 1), int(spectrum[b].sum())]
    assert cell.any() and spectrum[1, 5] == 1 and (mask == 0).any()


def test_clean_replaces_exactly_the_flagged_bytes():
    rng = np.random.default_rng(7)
    B, nb, n, C = 2, 2, 3, 4
    fb = rng.integers(0, 256, size=(B, 8, C), dtype=np.uint8)
    cell = np.zeros((B, nb, C), np.uint8)
    cell[0, 1, 2] = 2
    mask = np.ones((B, C), np.uint8)
    mask[1, 0] = 0
    spec = np.zeros((B, nb * n), np.uint8)
    spec[1, 4] = 1
    pre = np.full((B, 9, C), 0x3C, np.uint8)
    out, replaced = rm.clean(fb, 1, nb, n, 77, cell, mask, spec, out=pre, first_out=2)
    exp = pre.copy()
    count = [0, 0]
    for b in range(B):
        for t in range(nb * n):
            for c in range(C):
                rep = mask[b, c] == 0 or cell[b, t // n, c] != 0 or spec[b, t] != 0
                exp[b, 2 + t, c] = 77 if rep else fb[b, 1 + t, c]
                count[b] += int(rep)
    assert np.array_equal(out, exp) and replaced.tolist() == count == [3, 6 + 4 - 1]
    assert np.all(out[:, :2] == 0x3C) and np.all(out[:, 8:] == 0x3C)
    copy, none = rm.clean(fb, 1, nb, n, 77)
    assert np.array_equal(copy, fb[:, 1:7]) and none.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------- the recipe

@pytest.fixture(scope="module")
def recipe_flags():
    fb = rm.recipe()
    B, nb, n, C = rm.RECIPE_SHAPE
    cs, z = rm.moments(fb, 0, nb, n)
    return rm.flags(cs, z, n, rm.Thresholds(max_bad_blocks=2))


def test_recipe_is_what_the_model_flags(recipe_flags):
    B, nb, n, C = rm.RECIPE_SHAPE
    cell, mask, spectrum, counts = recipe_flags
    bad = cell != 0
    assert bad.size == 8192 and bad.sum() == 40
    assert bad[0, :, 37].all() and bad[1, :, 90].all()
    assert np.flatnonzero(bad[0, :, 200]).tolist() == [3, 4, 5]
    planted = np.zeros((B, C), bool)
    planted[0, 37] = planted[0, 200] = planted[1, 90] = True
    elsewhere = bad & ~planted[:, None, :]
    assert elsewhere.sum() == 5 and elsewhere.sum(axis=1).max() == 1
    beam, lo, hi = rm.RECIPE_BURST
    assert np.argwhere(spectrum).tolist() == [[beam, t] for t in range(lo, hi)]
    assert np.flatnonzero(mask[0] == 0).tolist() == [37, 200] and np.flatnonzero(mask[1] == 0).tolist() == [90]
    assert counts.tolist() == [[int(bad[0].sum()), 2, 0], [int(bad[1].sum()), 1, 4]]
    # the doubled noise shows in the variance, the raised blocks in the mean, the dead channel in the variance
    assert np.all(cell[0, :, 37] & 2) and np.all(cell[0, 3:6, 200] & 1) and np.all(cell[1, :, 90] & 2)


def test_recipe_false_alarm_caps(recipe_flags):
    """Conditions on the noise's false-alarm rate: at most 0.2 % of the cells outside the three planted channels, and no
    spectrum outside the burst."""
    B, nb, n, C = rm.RECIPE_SHAPE
    cell, _, spectrum, _ = recipe_flags
    bad = cell != 0
    bad[0, :, 37] = bad[0, :, 200] = bad[1, :, 90] = False
    assert bad.sum() <= 0.002 * (bad.size - 3 * nb)
    beam, lo, hi = rm.RECIPE_BURST
    outside = spectrum.copy()
    outside[beam, lo:hi] = 0
    assert not outside.any()
