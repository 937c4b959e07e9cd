"""The CPU model of the forms the RFI flagger's kernels take (helpers/rfi_forms.py; DESIGN.md section 5.23, "The forms"): its
constants and rules against the kernel's source text, a census of what the tables of tests/test_gpu_rfi.py present to the
launcher (helpers/rfi_cases.py; printed with pytest -s), and the bar: every form that can exist is run against the model, by
a moments case and by a clean case, and the hand-made sums of the flags tests are what they were made to be.  The last are
conditions on the inputs, asserted on the numpy model alone: if a builder misses one, the builder is wrong."""
import re
from pathlib import Path

import numpy as np

from helpers import rfi_cases as rc
from helpers import rfi_forms as rf
from helpers import rfi_model as rm

SOURCE = Path(__file__).resolve().parent.parent / "dc_sand_amd" / "csrc" / "bf_rfi.hip"


# ---------------------------------------------------------------------------------------------------------------- constants

def kernel_constants():
    return {name: int(value, 0) for name, value in re.findall(r"^constexpr uint32_t (k\w+) = (\w+?)u?;", SOURCE.read_text(), flags=re.M)}


def test_the_models_constants_and_rules_are_the_kernels():
    k = kernel_constants()
    assert (k["kThreads"], k["kLaneChannels"], k["kMaxLanes"]) == (rf.THREADS, rf.LANE_CHANNELS, rf.MAX_LANES) == (256, 16, 64)
    assert (k["kCellCache"], k["kBeamThreads"], k["kBeamWords"]) == (rf.CELL_CACHE, rf.BEAM_THREADS, rf.BEAM_WORDS) == (4096, 1024, 16)
    assert rf.ON_CHIP_SPECTRA == 16384 and rf.BEAM_UNROLL == 8 and (rf.M_BITS, rf.Q_BITS) == (24, 49)
    text = SOURCE.read_text()
    once = ["const uint32_t need = (C + kLaneChannels - 1u) / kLaneChannels;",
            "while (lanes < need && lanes < kMaxLanes) lanes <<= 1;",
            "tiles = (C - 1u) / (kLaneChannels * lanes) + 1u;",
            "t.R = kThreads >> __builtin_ctz(lanes);",
            "t.width = C - t.c0 < kLaneChannels * lanes ? C - t.c0 : kLaneChannels * lanes;",
            "return U == 16u ? kLaneChannels * j + i : U == 4u ? 4u * ((i >> 2) * L + j) + (i & 3u) : i * L + j;",
            "if (t.L >= 4u) {",
            "for (uint32_t x = 4u; x < t.L; x <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x);",
            "for (uint32_t x = 1u; x < t.L; x <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x);",
            "const bool cached = C <= kCellCache; // the same in every thread",
            "if (W <= kBeamThreads * kBeamWords) {",
            "for (; k + 8u <= a.nr_blocks; k += 8u) {",
            "for (; k < a.nr_blocks; k++) bad += f[(size_t)k * C] != 0u ? 1u : 0u;",
            "const uint32_t keep = bad > a.max_bad_blocks ? 0u : 1u;",
            "for (int bit = (bits - 1) & ~1; bit >= 0; bit -= 2) {",
            "select_rank<kThreads>(m, C, rank, 24, s_part, pass);",
            "select_rank<kThreads>(q, C, rank, 49, s_part, pass);"]
    for line in once:
        assert text.count(line) == 1, line
    twice = ["const bool lane_on = at_of<U>(0u, t.j, t.L) < t.width;",  # the moments and the clean kernel
             "if (a.C % 16u == 0u)", "else if (a.C % 4u == 0u)",         # their launchers
             "(reinterpret_cast<uintptr_t>(p) & (U - 1u)) == 0u, f);"]   # the clean kernel's two flag tensors
    for line in twice:
        assert text.count(line) == 2, line
    # the largest m and q there are fit the bits the bisections walk
    n = 65536
    assert 255 * n < 1 << rf.M_BITS and 65025 * (n // 2) ** 2 == 65025 << 30 < 1 << rf.Q_BITS


def test_the_model_on_shapes_worked_out_by_hand():
    assert [rf.lanes_of(C) for C in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 4100)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64]
    assert [rf.unit_of(C) for C in (1, 4, 16, 20, 48, 1030)] == [1, 4, 16, 4, 16, 1]
    f = rf.hot_form(144)
    assert (f.U, f.L, f.R, f.tiles, f.zero_dm, set(f.kinds)) == (16, 16, 16, 1, ("quads", 2), {"lanes off"})
    assert rf.tiles_of(144) == [rf.Tile(144, 9, "lanes off")]
    assert rf.tiles_of(200) == [rf.Tile(200, 16, "partial")] and rf.hot_form(200).U == 4
    assert rf.tiles_of(257) == [rf.Tile(257, 32, "partial")] and rf.hot_form(257).zero_dm == ("quads", 3)
    assert rf.tiles_of(512) == [rf.Tile(512, 32, "full")]
    assert rf.tiles_of(1030) == [rf.Tile(1024, 64, "full"), rf.Tile(6, 6, "lanes off")]
    assert rf.tiles_of(4100)[-1] == rf.Tile(4, 1, "lanes off") and rf.hot_form(4100).tiles == 5
    assert rf.hot_form(20).zero_dm == ("rows", 1) and rf.hot_form(3).zero_dm == ("rows", 0) and rf.hot_form(64).zero_dm == ("quads", 0)
    # every lane's every channel lies inside the tile, each place once, in all three units
    for U in rf.ALL_UNITS:
        for L in rf.ALL_LANES:
            assert sorted(rf.at_of(U, i, j, L) for j in range(L) for i in range(16)) == list(range(16 * L))
    assert [rf.beam_unroll(nb) for nb in (1, 7, 8, 9, 16, 17)] == [(0, 1), (0, 7), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert rf.on_chip(4096, 4, 4096) == (True, True) and rf.on_chip(4097, 1, 16385) == (False, False)


# ------------------------------------------------------------------------------------------------------------------- census

PAIRS, KINDS = rf.hot_forms_that_exist()
LANES_OFF = {(U, L) for U, L, kind in KINDS if kind == "lanes off"}
ZERO_DM = {rf.zero_dm_form(L) for L in rf.ALL_LANES}
UNROLL = {(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)}  # (trips of eight, capped at 2; a tail or none)

OLD_MOMENTS = rc.CHANNELS + rc.MORE_CHANNELS
OLD_CLEAN = rc.CLEAN_CHANNELS


def test_the_forms_that_can_exist():
    assert PAIRS == {(U, L) for U in rf.ALL_UNITS for L in rf.ALL_LANES}
    # whole lanes are off in a single tile only where 16-byte lanes go unused; narrower units only behind a full tile
    assert LANES_OFF == {(16, 4), (16, 8), (16, 16), (16, 32), (16, 64), (4, 64), (1, 64)}
    assert ZERO_DM == {("rows", 0), ("rows", 1), ("quads", 0), ("quads", 1), ("quads", 2), ("quads", 3), ("quads", 4)}


def test_census_of_the_older_tables():
    """Facts about the tables as they were, printed and written into DESIGN.md section 5.23 and the profiles/ note: what the
    new cases are for.  The tables stay, so the facts do."""
    m, c = rf.census(OLD_MOMENTS), rf.census(OLD_CLEAN)
    print("\n" + rf.format_census("moments, older tables", m) + "\n" + rf.format_census("clean, older tables", c))
    assert {L for _, L in m["pairs"]} == {1, 2, 4, 8, 64} == {L for _, L in c["pairs"]} | {2}
    assert len(m["pairs"]) == 8 and len(c["pairs"]) == 6
    assert m["lanes off"] == {(16, 64), (4, 64), (1, 64)} == c["lanes off"]
    assert {t for kind, t in m["zero-DM"] if kind == "quads"} == {0, 1, 4}
    f = rf.flags_census(rc.flags_calls())
    print(f"flags, older tables: unroll {sorted(f['unroll'])}, of those at C >= 64 {sorted(f['unroll at C >= 64'])}")
    assert f["unroll at C >= 64"] == {(0, 1), (2, 0)}  # no call with a tail behind an unrolled trip


def test_every_form_is_run_against_the_model():
    """The bar.  It fails on the older tables alone: that is what helpers/rfi_cases.FORM_CHANNELS and the hand-made flags
    cases are for."""
    m, c = rf.census(OLD_MOMENTS + rc.FORM_CHANNELS), rf.census(OLD_CLEAN + rc.FORM_CHANNELS)
    print("\n" + rf.format_census("moments", m) + "\n" + rf.format_census("clean", c))
    for name, seen in (("moments", m), ("clean", c)):
        assert seen["pairs"] == PAIRS, (name, sorted(PAIRS - seen["pairs"]))
        assert seen["lanes off"] == LANES_OFF, (name, sorted(LANES_OFF - seen["lanes off"]))
        assert seen["zero-DM"] == ZERO_DM, (name, sorted(ZERO_DM - seen["zero-DM"]))
    # the byte path of the clean kernel's flag loads: both vector units, every offset class
    assert {rf.unit_of(C) for C in rc.OFFSET_CASES} == {16, 4}
    for C, offsets in rc.OFFSET_CASES.items():
        U = rf.unit_of(C)
        assert all(o % U for o in offsets) and {o % 4 for o in offsets} >= ({1, 0} if U == 16 else {1, 2, 3})
    f = rf.flags_census(list(rc.flags_calls()) + list(rc.new_flags_calls()))
    print(f"flags: unroll {sorted(f['unroll at C >= 64'])}; cells {sorted(f['cells on chip'])}; window {sorted(f['window on chip'])}")
    assert f["unroll at C >= 64"] == UNROLL, sorted(UNROLL - f["unroll at C >= 64"])
    assert f["cells on chip"] >= {(True, 4096), (False, 4097)} and f["window on chip"] >= {(True, 16384), (False, 16385)}


def test_form_cases_are_what_the_tables_say():
    cases = rc.form_cases()
    assert sorted(cases) == sorted(rc.FORM_CHANNELS) and len(set(rc.FORM_CHANNELS)) == len(rc.FORM_CHANNELS)
    assert not set(rc.FORM_CHANNELS) & set(OLD_MOMENTS) - {16, 20}  # 16 and 20 are new to the clean table only
    for C, rows in cases.items():
        assert [r[0] for r in rows] == rc.FORM_BLOCK_LENS == [1, 5, 258]
        assert {r[1] for r in rows} == {1, 2, 3} == {r[2] for r in rows} and sorted(r[3] for r in rows) == [0, 0, 3]
        assert max(r[0] * r[1] * r[2] * C for r in rows) < 2 << 20
    f = {C: rf.hot_form(C) for C in rc.FORM_CHANNELS[:4]}
    assert [(f[C].U, f[C].L, sorted(f[C].kinds)) for C in (144, 200, 257, 512)] == \
        [(16, 16, ["lanes off"]), (4, 16, ["partial"]), (1, 32, ["partial"]), (16, 32, ["full"])]
    assert rf.tiles_of(144)[0].lanes_on == 9
    # 258 rows: more than one trip of the moments' loop over groups of four rows at every L, and a last group of two rows
    assert all(-(-258 // 4) > 2 * (256 // L) or L < 8 for L in rf.ALL_LANES) and 258 % 4 == 2


# ----------------------------------------------------------------------------------------------- hand-made sums: the unroll

def test_unroll_cases_put_channels_on_both_sides_of_max_bad_blocks():
    for nb in rc.UNROLL_NR_BLOCKS:
        U = 8 * (nb // 8)
        fb = rc.unroll_filterbank(nb)
        cs, z = rm.moments(fb, 0, nb, rc.UNROLL_LEN)
        cell = rm.flags(cs, None, rc.UNROLL_LEN, rm.Thresholds())[0]
        bad = (cell != 0).sum(axis=1)
        assert np.array_equal(bad, rc.unroll_expected_bad(nb)) and set(np.unique(cell)) == {0, 1}
        where = {"unrolled": set(), "tail": set(), "both": set()}
        for c, blocks in rc.unroll_bad_cells(nb).items():
            assert all(0 <= k < nb for k in blocks) and len(set(blocks)) == len(blocks)
            assert all(cell[0, k, c] for k in blocks) and all(cell[1, k, (c + 1) % rc.UNROLL_C] for k in blocks)
            part = "unrolled" if max(blocks) < U else "tail" if min(blocks) >= U else "both"
            where[part].add(len(blocks))
        # exactly max_bad_blocks and one more, for max_bad_blocks 0, 1 and 2, wherever the part has the blocks for it
        assert where["unrolled"] >= {1, 2, 3}
        if nb > U:
            assert where["tail"] >= {1} and where["both"] >= {2, 3}
            assert any(sorted(b)[-2:] == [U - 1, U] for b in rc.unroll_bad_cells(nb).values())  # across the boundary
        for M in rc.UNROLL_MAX_BAD:
            mask = rm.flags(cs, None, rc.UNROLL_LEN, rm.Thresholds(max_bad_blocks=M))[1]
            assert np.array_equal(mask, (bad <= M).astype(np.uint8)) and 0 < (mask == 0).sum() < mask.size
            assert (bad == M).any() and (bad == M + 1).any()


# --------------------------------------------------------------------------------------------- hand-made sums: the top bits

TOP_THRESHOLDS, m_and_q = rc.TOP_THRESHOLDS, rc.m_and_q


def test_top_bit_sums_are_consistent_and_sit_on_both_sides():
    n = rc.TOP_BITS_LEN
    cs = rc.top_bits_sums()
    assert cs.shape == (1, 6, 70, 2) and cs.dtype == np.uint32 and np.array_equal(cs, rc.top_bits_sums())
    m, q = m_and_q(cs, n)
    # sums that bytes can have: s1 <= 255 n, s1^2 <= n s2 (Cauchy-Schwarz) and s2 <= 255 s1
    assert m.max() == 255 * n and m.min() == 0 and np.all(cs[..., 1].astype(np.uint64) <= 255 * m)
    assert np.all(np.uint64(n) * cs[..., 1].astype(np.uint64) >= m * m)
    assert q.max() == 65025 << 30 and (q == 65025 << 30).sum() == 2  # half 0 and half 255, in the blocks 0 and 4
    med = rm.lower_median(m)[0, :, 0]
    mad = rm.lower_median(np.where(m > rm.lower_median(m), m - rm.lower_median(m), rm.lower_median(m) - m))[0, :, 0]
    print(f"\nmedians of m {med.tolist()}\nMADs of m {mad.tolist()}\nmedians of q {rm.lower_median(q)[0, :, 0].tolist()}")
    # bit 23 decides the medians of the blocks 1 and 5, bit 22 those of the blocks 0, 2 and 4, neither that of block 3
    assert [int(x) >> 22 for x in med] == [1, 2, 1, 0, 1, 2]
    assert mad[5] == (1 << 22) + 8 and med[5] == (1 << 23) + 100  # bit 22 decides a MAD
    assert rm.lower_median(q).max() >= 1 << 45 and rm.lower_median(q).min() < 1 << 44
    cell = rm.flags(cs, None, n, TOP_THRESHOLDS)[0]
    for lo, hi in ((0, 1 << 22), (1 << 22, 1 << 23), (1 << 23, 1 << 24)):  # flagged and unflagged cells on each side
        inside = (m >= lo) & (m < hi)
        assert (cell[inside] & 1).any() and not (cell[inside] & 1).all(), (lo, hi)
    for lo, hi in ((0, 1 << 40), (1 << 40, 1 << 45), (1 << 45, 1 << 46)):
        inside = (q >= lo) & (q < hi)
        assert (cell[inside] & 2).any() and not (cell[inside] & 2).all(), (lo, hi)
    # block 5: the limit lies ON the cell at 2 d with thr = 2, and ON the cell at 1.5 d with thr = 1.5 (both exact); the
    # cell of all 255 lies between them
    d = (1 << 22) + 8
    for thr, flagged in ((2.0, 0), (float(np.nextafter(2.0, 0.0)), 1), (1.5, 2), (1.4999, 3)):
        got = rm.flags(cs[:, 5:], None, n, rm.Thresholds(thr, 0.0, 1e300, 0.0))[0]
        far = np.abs(m[0, 5].astype(np.int64) - ((1 << 23) + 100)) >= d + d // 2
        assert far.sum() == 3 and got[0, 0][far].sum() == flagged and not got[0, 0][~far].any(), thr
    # the floor as the limit, ON the distance of block 0's largest m and of its largest q (the cell of half 0 and half 255): the
    # cell is kept there and flagged one step below
    for which, values in (("m", m), ("q", q)):
        at, floor = rc.top_cell_and_its_distance(values[0, 0])
        assert (values[0, 0] == values[0, 0][at]).sum() == 1 and int(floor) == int(values[0, 0][at]) - int(rm.lower_median(values[0, 0])[0]) > 1 << 22
        for f, flagged in ((floor, False), (float(np.nextafter(floor, 0.0)), True)):
            thr = rm.Thresholds(0.0, f, 0.0, 1e300) if which == "m" else rm.Thresholds(0.0, 1e300, 0.0, f)
            got = rm.flags(cs[:, :1], None, n, thr)[0][0, 0]
            assert bool(got[at]) == flagged and (got != 0).sum() < 70, (which, f)


def test_the_gpu_tests_thresholds_are_the_ones_held_above():
    thr = rc.top_bits_thresholds(rc.top_bits_sums())
    assert len(thr) == 10 and thr[0] == TOP_THRESHOLDS and {t.mean_thr for t in thr} >= {2.0, 1.5, 1.4999, float(np.nextafter(2.0, 0.0))}
    cs = rc.top_bits_sums()
    seen = [rm.flags(cs, None, rc.TOP_BITS_LEN, t) for t in thr]
    assert all(0 < (s[0] != 0).sum() < s[0].size for s in seen[:6])  # no trivial expectation
    assert len({s[0].tobytes() for s in seen}) == len(seen)         # and no two alike
