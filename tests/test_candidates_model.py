"""Anchors of the model of the candidate sifter (helpers/candidates_model.py; include/dcs_candidates.h): the vectorised
implementation against the naive one on seeded planes with NaN, +-inf, +-0, plateaus and duplicate maxima across widths,
the rules on planes built by hand, and the Python side's constants against the C header's.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest

from helpers.candidates_model import (CANDIDATE, NO_WIDTH, collapse, expected_buffer, find_candidates, find_candidates_naive,
                                      same_bits, seeded_planes)

ROOT = Path(__file__).resolve().parents[1]


def plane_of(s):
    """A collapsed plane float [nr_dm][nr_blocks] as (snr, peaks) of one beam and one width."""
    s = np.asarray(s, np.float32)
    snr = s[None, :, None, :].copy()
    n = snr.size
    peaks = np.stack([np.arange(n, dtype=np.uint32) + 1000, np.arange(n, dtype=np.uint32) + 5000], axis=-1)
    return snr, peaks.reshape(snr.shape + (2,))


@pytest.mark.parametrize("seed,shape,first_block,nr_blocks,radii,special", [
    (0, (2, 9, 3, 20), 3, 14, (1, 1), 0.0),
    (1, (2, 9, 3, 20), 0, 20, (2, 3), 0.15),
    (2, (1, 12, 4, 17), 2, 15, (8, 8), 0.15),
    (3, (3, 5, 2, 11), 1, 9, (0, 0), 0.3),
    (4, (1, 7, 5, 13), 0, 13, (8, 0), 0.1),
    (5, (1, 7, 5, 13), 4, 9, (0, 8), 0.1),
    (6, (2, 6, 0, 8), 0, 8, (1, 1), 0.0),
    (7, (1, 1, 2, 1), 0, 1, (3, 3), 0.0),
])
def test_the_two_implementations_agree(seed, shape, first_block, nr_blocks, radii, special):
    snr, peaks = seeded_planes(*shape, seed=seed, special=special)
    if special:
        assert np.isnan(snr).any() and np.isposinf(snr).any() and np.isneginf(snr).any() and np.signbit(snr[snr == 0]).any()
    for threshold in (-3.0, 0.0, 6.25, 11.5, 100.0):
        for max_candidates in (0, 3, 10**6):
            got, count = find_candidates(snr, peaks, first_block, nr_blocks, threshold, *radii, max_candidates)
            exp, exp_count = find_candidates_naive(snr, peaks, first_block, nr_blocks, threshold, *radii, max_candidates)
            assert same_bits(got, exp) and np.array_equal(count, exp_count), (threshold, max_candidates)
            assert count[0] == len(got) and count[1] == min(len(got), max_candidates)
            key = [(int(r["beam"]), int(r["dm"]), int(r["block"])) for r in got]
            assert key == sorted(set(key))  # ascending (b, m, k), no cell twice


def test_seeded_planes_have_duplicate_maxima_and_plateaus():
    snr, _ = seeded_planes(2, 9, 3, 20, seed=0)
    s, best = collapse(snr, 0, 20)
    assert ((snr == s[:, :, None, :]).sum(axis=2) > 1).any()  # the same maximum at two widths: the lower index is taken
    assert np.all(s[:, 1:4, 2:6] == np.float32(11.5)) and np.all(best[:, 1:4, 2:6] == 0)


def test_collapse_skips_nan_and_keeps_the_first_of_equals():
    snr = np.array([[np.nan, 2.0, 2.0], [np.nan, np.nan, np.nan], [-np.inf, -np.inf, 1.0], [-0.0, 0.0, -1.0]], np.float32)
    s, best = collapse(snr.T[None, None].copy().reshape(1, 1, 3, 4), 0, 4)
    assert best[0, 0].tolist() == [1, NO_WIDTH, 2, 0]
    assert s[0, 0].tolist()[:3] == [2.0, -np.inf, 1.0] and np.signbit(s[0, 0, 3])
    none, none_best = collapse(np.zeros((1, 2, 0, 5), np.float32), 1, 3)
    assert np.all(none == -np.inf) and np.all(none_best == NO_WIDTH)


def test_a_plateau_gives_one_candidate_the_first():
    s = np.zeros((9, 12), np.float32)
    s[2:6, 3:8] = 7.0
    snr, peaks = plane_of(s)
    for radii in ((1, 1), (2, 3), (8, 8), (1, 0), (0, 1)):
        rec, count = find_candidates(snr, peaks, 0, 12, 5.0, *radii, 100)
        if 0 in radii:  # the plateau is connected through one axis only: one candidate per row or per column of it
            n = 5 if radii[0] else 4
            assert count.tolist() == [n, n]
            continue
        assert count.tolist() == [1, 1] and (rec[0]["dm"], rec[0]["block"]) == (2, 3)
        assert rec[0]["members"] == (radii[0] + 1) * (radii[1] + 1) if radii != (8, 8) else rec[0]["members"] == 20
    # +0 and -0 are one plateau
    s = np.full((3, 3), -1.0, np.float32)
    s[1, 1], s[1, 2] = 0.0, -0.0
    rec, count = find_candidates(*plane_of(s), 0, 3, -0.5, 1, 1, 10)
    assert count[0] == 1 and (rec[0]["dm"], rec[0]["block"]) == (1, 1)


def test_radius_zero_gives_every_cell_at_or_above_threshold():
    snr, peaks = seeded_planes(2, 6, 3, 10, seed=9, special=0.2)
    s, best = collapse(snr, 2, 7)
    rec, count = find_candidates(snr, peaks, 2, 7, 3.0, 0, 0, 1000)
    at = np.argwhere(s >= np.float32(3.0))
    assert count[0] == len(at) > 10 and np.all(rec["members"] == 1)
    assert np.array_equal(np.stack([rec["beam"], rec["dm"], rec["block"] - 2], axis=1), at)
    assert np.array_equal(rec["width_index"], best[s >= np.float32(3.0)])
    assert np.array_equal(rec["snr"].view(np.uint32), s[s >= np.float32(3.0)].view(np.uint32))
    for r in rec[:20]:
        assert (r["value"], r["time"]) == tuple(peaks[r["beam"], r["dm"], r["width_index"], r["block"]])


def test_members_at_the_four_edges():
    """Every cell is above threshold and strictly ordered, the corners highest: the window is cut at the rectangle."""
    D, K, first_block = 7, 9, 4
    s = np.ones((D, K), np.float32)
    s[0, 0], s[0, K - 1], s[D - 1, 0], s[D - 1, K - 1], s[3, 4] = 10.0, 11.0, 12.0, 13.0, 14.0
    snr = np.full((1, D, 1, first_block + K + 2), 99.0, np.float32)  # blocks outside the call: higher, and not there
    snr[0, :, 0, first_block:first_block + K] = s
    peaks = np.zeros(snr.shape + (2,), np.uint32)
    rec, count = find_candidates(snr, peaks, first_block, K, 5.0, 2, 3, 100)
    got = {(int(r["dm"]), int(r["block"]) - first_block): int(r["members"]) for r in rec}
    assert got == {(0, 0): 1, (0, K - 1): 1, (D - 1, 0): 1, (D - 1, K - 1): 1, (3, 4): 1}
    rec, _ = find_candidates(snr, peaks, first_block, K, 0.5, 2, 3, 100)
    got = {(int(r["dm"]), int(r["block"]) - first_block): int(r["members"]) for r in rec}
    assert got == {(0, 0): 3 * 4, (0, K - 1): 3 * 4, (D - 1, 0): 3 * 4, (D - 1, K - 1): 3 * 4, (3, 4): 5 * 7}
    exp, _ = find_candidates_naive(snr, peaks, first_block, K, 0.5, 2, 3, 100)
    assert same_bits(rec, exp)


def test_overflow_truncates_in_order():
    snr, peaks = seeded_planes(2, 6, 3, 10, seed=10)
    rec, count = find_candidates(snr, peaks, 0, 10, 2.0, 1, 1, 10**6)
    found = len(rec)
    assert found > 6
    prefill = np.zeros(found + 2, CANDIDATE)
    prefill.view(np.uint32)[:] = 0x3C3C3C3C
    for max_candidates in (0, 1, found - 1, found, found + 2):
        again, count = find_candidates(snr, peaks, 0, 10, 2.0, 1, 1, max_candidates)
        assert same_bits(again, rec) and count.tolist() == [found, min(found, max_candidates)]
        buf = expected_buffer(again, count, prefill[:max_candidates])
        assert same_bits(buf[:count[1]], rec[:count[1]]) and np.all(buf[count[1]:].view(np.uint32) == 0x3C3C3C3C)


def test_python_constants_are_the_headers():
    from dc_sand_amd import generator as gen

    text = (ROOT / "dc_sand_amd" / "csrc" / "bf_arg_checks.h").read_text()
    m = re.search(r"kCandTileDms = (\d+)u, kCandTileBlocks = (\d+)u, kCandMaxRadius = (\d+)u;", text)
    assert tuple(map(int, m.groups())) == (gen.CANDIDATES_TILE_DMS, gen.CANDIDATES_TILE_BLOCKS, gen.CANDIDATES_MAX_RADIUS)
    hip = (ROOT / "dc_sand_amd" / "csrc" / "bf_candidates.hip").read_text()
    threads = int(re.search(r"kScanThreads = (\d+);", hip).group(1))
    items = int(re.search(r"kScanItems = (\d+);", hip).group(1))
    assert threads * items == gen.CANDIDATES_SCAN_SPAN
    assert gen.candidate_dtype == CANDIDATE and gen.candidate_dtype.itemsize == 32 == gen.candidates_bytes(1)
