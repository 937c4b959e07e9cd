"""The CPU model of the form bf_dedisperse_kernel takes per chunk (helpers/dedisperse_paths.py): its
constants against the kernel's source text, the model on hand-made chunks, a census of what the older GPU tests present to
the rule, and the conditions a-i that the edge tables of tests/test_gpu_dedisperse.py must meet.  Those are conditions on
the inputs, asserted on the model alone: if a builder misses one, the builder is wrong."""
import re
from pathlib import Path

import numpy as np
import pytest

from helpers import dedisperse_cases
from helpers import dedisperse_paths as dp
from helpers.dedisperse_model import INT32_MAX, INT32_MIN

SOURCE = Path(__file__).resolve().parent.parent / "dc_sand_amd" / "csrc" / "bf_dedisperse.hip"


# ---------------------------------------------------------------------------------------------------------------- constants

def kernel_constants():
    """The ``constexpr uint32_t`` lines of the kernel's file, evaluated in order."""
    names = {}
    for name, expr in re.findall(r"^constexpr uint32_t (k\w+) = ([^;]+);", SOURCE.read_text(), flags=re.M):
        expr = re.sub(r"\b(\d+)u\b", r"\1", expr).replace("/", "//")
        assert re.fullmatch(r"[\w\s*+\-/<>()]+", expr), expr
        names[name] = eval(expr, {"__builtins__": {}}, dict(names))
    return names


def test_the_models_constants_are_the_kernels():
    k = kernel_constants()
    assert (k["kTileT"], k["kTileD"], k["kChunk"], k["kWinBytes"], k["kZero"], k["kSlack"]) == (512, 16, 32, 36 << 10, 528, 16)
    assert (dp.TILE_T, dp.TILE_D, dp.CHUNK, dp.WIN_BYTES, dp.ZERO, dp.SLACK) == (512, 16, 32, 36 << 10, 528, 16)
    assert k["kThreads"] == 256 and k["kMaxPitch"] == dp.MAX_PITCH == 1152 and dp.MAX_SPREAD == 620
    # the rule itself, as the kernel writes it: the model restates these three lines
    text = SOURCE.read_text()
    for line in ("uint32_t pitch = (kTileT + spread + kSlack) & ~3u;",
                 "pitch |= 4u;",
                 "const uint32_t rows = (uint32_t)(rhi - rlo) + nt;",
                 "const bool staged = spread <= kMaxPitch - kTileT - kSlack - 4u && rows <= 2u * pitch + 64u;",
                 "const int32_t wl = lo - ((lo - rlo) & 3);"):
        assert text.count(line) == 1, line
    # both roundings of the pitch, and what they are for: a whole, odd number of dwords; a lane's three dwords -- 516 bytes
    # from the dword of the term's first byte, which lies at most spread + ((lo - rlo) & 3) into the window -- stay inside
    # the column's window, and the staged windows inside their LDS
    assert [dp.pitch_of(s) for s in (0, 1, 3, 4, 7, 8, 617, 620, 621)] == [532, 532, 532, 532, 532, 540, 1148, 1148, 1148]
    assert k["kTimesPerLane"] * 63 + 12 == 516 <= dp.ZERO
    for s in range(0, 1300):
        p = dp.pitch_of(s)
        assert p % 4 == 0 and (p // 4) % 2 == 1 and all(((s + r) & ~3) + 516 <= p for r in range(4))
        assert s > dp.MAX_SPREAD or dp.CHUNK * p <= dp.WIN_BYTES
    assert dp.rows_limit(620) == 2360 and dp.at_limit(620, 512) == 1848


# ---------------------------------------------------------------------------------------------------------- hand-made chunks

def paths(table, T, max_delay, mask=None):
    return list(dp.chunk_paths(np.asarray(table, dtype=np.int32), T, max_delay, mask))


def test_one_column_one_dm():
    (p,) = paths([[7]], 512, 7)
    assert (p.kind, p.spread, p.pitch, p.rows, p.nt, p.nd, p.cc) == ("staged", 0, 532, 512, 512, 1, 1)
    assert p.lo_residues == {0} and p.shifts == {0} and (p.widest, p.widest_residue, p.dead) == (0, 0, ())
    # one column, many DMs: the spread alone decides
    for top, kind in ((620, "staged"), (621, "direct")):
        (p,) = paths([[0], [5], [top]], 100, 1000)
        assert (p.kind, p.spread, p.rows, p.nd, p.shifts) == (kind, top, top + 100, 3, {0, 1, top & 3})
    # one DM, many columns: no spread, the rows alone decide; the limit is 2 * 532 + 64 = 1128 rows
    for top, kind in ((616, "staged"), (617, "direct")):
        (p,) = paths([[0, 1, 2, 3, top]], 512, 1000)
        assert (p.kind, p.spread, p.pitch, p.rows) == (kind, 0, 532, top + 512)
        assert p.lo_residues == {0, 1, 2, 3} == p.shifts and p.widest == 4 and p.widest_residue == top & 3


def test_tiles_and_chunks_are_counted_as_the_kernel_counts_them():
    table = np.zeros((33, 65), np.int32)
    ps = paths(table, 1025, 0)
    assert len(ps) == 3 * 3 * 3 and [p.nd for p in ps[::9]] == [16, 16, 1]
    assert [p.nt for p in ps[:9:3]] == [512, 512, 1] and [p.cc for p in ps[:3]] == [32, 32, 1]
    assert [(p.dm_tile, p.t_tile, p.chunk) for p in ps[:4]] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0)]
    assert {p.kind for p in ps} == {"staged"}
    assert dp.workgroups(ps)[2, 2] == ["staged"] * 3 and dp.orders(ps) == {("staged", "staged")}


def test_terms_that_drop():
    max_delay = 900
    outside = [-1, INT32_MIN, max_delay + 1, INT32_MAX]
    # all terms dropped, by their value or by the mask
    (p,) = paths([outside, outside[::-1]], 10, max_delay)
    assert (p.kind, p.spread, p.rows, p.widest, p.dead) == ("none", 0, 0, None, (0, 1, 2, 3)) and not p.lo_residues and not p.shifts
    (p,) = paths([[0, 5], [900, 7]], 10, max_delay, mask=[0, 0])
    assert p.kind == "none"
    # entries at 0 and at max_delay take part; one past it does not
    (p,) = paths([[0, 5], [900, 7]], 10, max_delay)
    assert (p.kind, p.spread, p.rows) == ("direct", 900, 910)
    (p,) = paths([[0, 5], [901, 7]], 10, max_delay)
    assert (p.kind, p.spread, p.rows, p.dead) == ("staged", 2, 17, ())
    # a masked column inside a chunk that is otherwise staged: its entries do not count, whatever they are
    table = [[10, 0, 13], [14, 900, 19]]
    assert paths(table, 512, max_delay)[0].kind == "direct"
    (p,) = paths(table, 512, max_delay, mask=[1, 0, 0x80])
    assert (p.kind, p.spread, p.rows, p.dead, p.widest, p.widest_residue) == ("staged", 6, 9 + 512, (1,), 2, 3)
    assert p.lo_residues == {0, 3} and p.shifts == {0, 3, 1}  # wl = 10 and 10: 10, 14 -> 0; 13, 19 -> 3, 1
    # a DM whose every entry drops does not count either, and the second tile starts at DM 16
    table = np.zeros((17, 2), np.int32)
    table[3] = -5
    table[16] = [30, 700]
    a, b = paths(table, 5, max_delay)
    assert (a.kind, a.spread, a.nd, b.kind, b.spread, b.rows, b.nd) == ("staged", 0, 16, "staged", 0, 675, 1)


# ------------------------------------------------------------------------------------------------------------------ census

def census_of(calls):
    total = None
    for table, T, max_delay, mask in calls:
        total = dp.merge_census(total, dp.census(dp.chunk_paths(table, T, max_delay, mask)))
    return total


def format_census(c):
    short = {"staged": "S", "direct": "D", "none": "N"}
    lines = [f"chunks {c['chunks']}"]
    for key in sorted(c["spread"]):
        lines.append(f"spread of {key[0]} chunks on {key[1]} tiles: {c['spread'][key][0]} .. {c['spread'][key][1]}")
    lines.append(f"nearest staged chunk: {c['rows_inside']} rows inside rows <= 2 pitch + 64")
    lines.append(f"nearest chunk that is direct by its rows: {c['rows_outside']} rows outside")
    lines.append("orders: " + " ".join(sorted(short[a] + short[b] for a, b in c["orders"])))
    lines.append("nd: " + " ".join(str(n) for n in sorted(c["nd"])))
    return "\n".join(lines)


def test_census_of_the_older_gpu_tests():
    """Facts about the older tests, printed (pytest -s) and written into DESIGN.md section 5.16 and the profiles/ note.
    They are no bar: all that is asserted is that the model ran over those tables."""
    c = census_of(dedisperse_cases.calls())
    print("\n" + format_census(c))
    assert c["chunks"] > 400 and c["nd"] and c["orders"]


# ------------------------------------------------------------------------------------------------------ coverage conditions

def records(case):
    table, mask, T, max_delay = case
    return list(dp.chunk_paths(table, T, max_delay, mask))


@pytest.fixture(scope="module")
def edge_records():
    """{(nt, part, C): records} of every edge case of the GPU tests."""
    return {(nt, part, C): records(dp.edge_case(nt, part, C)) for nt in dp.EDGE_NT for part in range(dp.EDGE_PARTS) for C in dp.EDGE_C}


def is_a(p, spread=620):
    """Condition (a) but for the kind and the tile: the widest window is the last one in LDS, at residue 3."""
    return (p.spread == spread and p.cc == 32 and p.widest == 31 and p.widest_residue == 3 and p.lo_residues == {0, 1, 2, 3}
            and p.shifts == {0, 1, 2, 3})


def at_edge(p):
    return p.kind == "staged" and p.rows == 2 * p.pitch + 64


def past_edge(p):
    return p.kind == "direct" and p.spread <= 620 and p.rows == 2 * p.pitch + 65


def test_edge_tables_fit_their_shapes():
    for nt in dp.EDGE_NT:
        for C in dp.EDGE_C:
            table, mask, T, max_delay = dp.edge_case(nt, 2, C)
            assert table.shape == (16, C) and table.dtype == np.int32 and mask.shape == (C,) and T % 512 == nt % 512
            assert max_delay == dp.MAX_DELAY <= 2500 and T in (512, 513, 999, 1024, 1025)
            again = dp.edge_case(nt, 2, C)
            assert np.array_equal(table, again[0]) and np.array_equal(mask, again[1])  # seeded
    assert 487 % 8 != 0 and 1000 % 512 % 8 == 0  # why 999 spectra and not 1000: the last tile's times are no multiple of 8


@pytest.mark.parametrize("C", dp.EDGE_C)
def test_conditions_a_b_c_on_full_tiles(edge_records, C):
    full = [p for (nt, part, c), ps in edge_records.items() if c == C and nt == 512 for p in ps if p.nt == 512]
    a = [p for p in full if p.kind == "staged" and is_a(p)]
    assert a and any(p.rows < 2 * p.pitch + 64 for p in a)                                     # a
    assert any(at_edge(p) and p.rows == 2360 and p.pitch == 1148 for p in a)                   # b: rhi - rlo = 1848
    assert any(p.kind == "direct" and is_a(p, 621) and p.rows <= 2 * p.pitch + 64 for p in full)  # c: direct by its spread alone


@pytest.mark.parametrize("C", dp.EDGE_C)
@pytest.mark.parametrize("nt", dp.EDGE_NT)
def test_conditions_d_e(edge_records, C, nt):
    """For every spread of the two pitch roundings a staged chunk at the limit on the rows and a direct one a row past it,
    in tiles of nt times: 512 (d), and 487 and 1 (e), where the rows count the tile's own times.  (a) in those tiles too."""
    tile = [p for (n, part, c), ps in edge_records.items() if c == C and n == nt for p in ps if p.nt == nt]
    assert {(p.pitch, (p.spread + 512 + 16) & 3, p.pitch - (p.spread + 512 + 16)) for p in tile if p.spread in dp.D_SPREADS} >= {
        (532, 0, 4), (532, 1, 3), (532, 2, 2), (532, 3, 1), (532, 0, 0), (532, 1, -1), (532, 2, -2), (532, 3, -3),
        (1148, 1, 3), (1148, 2, 2), (1148, 3, 1), (1148, 0, 0)}
    for s in dp.D_SPREADS:
        assert any(at_edge(p) and p.spread == s and p.widest == 31 and p.widest_residue == 3 for p in tile), s
        assert any(past_edge(p) and p.spread == s and p.widest == 31 and p.widest_residue == 3 for p in tile), s
    assert any(p.kind == "staged" and is_a(p) for p in tile)
    if nt != 512:  # the same chunks in the full tile beside it span more rows: direct
        full = [p for (n, part, c), ps in edge_records.items() if c == C and n == nt for p in ps if p.nt == 512]
        assert full and sum(p.kind == "direct" for p in full) >= 2 * len(dp.D_SPREADS)


def test_condition_h_ragged_last_chunk(edge_records):
    """C = 320 stages dwords; C = 317 stages bytes, its rows start at any byte, and its last chunk has 29 columns."""
    assert dp.EDGE_C[0] % 4 == 0 and dp.EDGE_C[1] % 4 == 1 and dp.ORDER_C == dp.EDGE_C
    for (nt, part, C), ps in edge_records.items():
        last = [p for p in ps if p.chunk == 9]
        assert last and all(p.cc == (32 if C == 320 else 29) and p.kind == "staged" for p in last if p.nt == nt)


@pytest.mark.parametrize("C", dp.EDGE_C)
def test_condition_i_masked_and_dead_columns(edge_records, C):
    for nt in dp.EDGE_NT:
        table, mask, T, max_delay = dp.edge_case(nt, 2, C)
        hit = [p for p in edge_records[nt, 2, C] if p.nt == nt and at_edge(p) and p.spread == 620 and p.dead == (5, 9)]
        assert hit and len({p.chunk for p in hit}) == 1, nt
        c0 = 32 * hit[0].chunk
        assert mask[c0 + 5] == 0 and mask[c0 + 9] != 0 and np.count_nonzero(mask) == C - 1
        assert not ((table[:, c0 + 9] >= 0) & (table[:, c0 + 9] <= max_delay)).any()
        # the masked column's entries would count otherwise: the chunk is direct without the mask
        bare = [p for p in dp.chunk_paths(table, T, max_delay) if p.nt == nt and p.chunk == hit[0].chunk][0]
        assert bare.kind == "direct" and bare.spread > 620 and bare.dead == (9,)


ALL_ORDERS = {(a, b) for a in ("staged", "direct", "none") for b in ("staged", "direct", "none")}


@pytest.mark.parametrize("C", dp.ORDER_C)
def test_condition_f_orders(C):
    ps = records(dp.order_case(C))
    assert len(dp.workgroups(ps)) == 1 and dp.orders(ps) == ALL_ORDERS
    kinds = dp.workgroups(ps)[0, 0]
    assert "".join(k[0].upper() for k in kinds) == dp.ORDER_KINDS
    staged = [p for p in ps if p.kind == "staged" and p.cc == 32]
    assert all(is_a(p) for p in staged) and any(at_edge(p) for p in staged)
    direct = [p for p in ps if p.kind == "direct"]
    assert {p.spread for p in direct} == {620, 621} and any(past_edge(p) for p in direct)
    # two DM tiles and two time tiles: every workgroup has all nine orders but for what the tile of 512 times turns direct,
    # and at some chunk the four workgroups that run side by side take all three forms
    ps = records(dp.order_case_tiles(C))
    groups = dp.workgroups(ps)
    assert sorted(groups) == [(0, 0), (0, 1), (1, 0), (1, 1)] and {p.nd for p in ps} == {16, 13} and {p.nt for p in ps} == {512, 1}
    assert dp.orders(p for p in ps if p.t_tile == 1 and p.dm_tile == 0) == ALL_ORDERS
    assert dp.orders(p for p in ps if p.t_tile == 1 and p.dm_tile == 1) == ALL_ORDERS
    assert any({g[i] for g in groups.values()} == {"staged", "direct", "none"} for i in range(10))
    assert any(groups[0, 0][i] == "direct" and groups[0, 1][i] == "staged" for i in range(10))


def test_condition_g_nd_and_nr_dm():
    """Every nd at a wave's boundary (4, 5, 8, 12, 13, 16) in a staged chunk like (a)'s; nd = 1 has no spread, so its chunks
    sit on the other edge, the limit on the rows; nr_dm = 17 and 33 put a tile of one DM second and third."""
    assert {17, 33} <= set(dp.SWEEP_NR_DM)
    seen, behind = set(), set()
    for nr_dm in dp.SWEEP_NR_DM:
        ps = records(dp.sweep_case(nr_dm))
        assert {p.kind for p in ps} == {"staged", "direct"}
        for p in ps:
            if p.nd > 1 and p.kind == "staged" and is_a(p):
                seen.add(p.nd)
            if p.nd == 1 and at_edge(p) and p.lo_residues == {0, 1, 2, 3} == p.shifts:
                seen.add(1)
                behind.add(p.dm_tile)
            if p.nd == 1:
                assert p.spread == 0
        for k in range(-(-nr_dm // 16)):
            tile = [p for p in ps if p.dm_tile == k]
            assert any(at_edge(p) for p in tile) and any(past_edge(p) for p in tile) and tile[0].nt == 512
    assert seen == {1, 4, 5, 8, 12, 13, 16} and behind == {1, 2}


def test_replay_tables_change_the_form_of_the_same_chunks():
    (staged, direct, none), T, max_delay = dp.replay_tables()
    assert staged.shape == direct.shape == none.shape == (16, dp.REPLAY_C) and T == 513
    for table, kind in ((staged, "staged"), (direct, "direct"), (none, "none")):
        ps = list(dp.chunk_paths(table, T, max_delay))
        assert len(ps) == 6 and {p.kind for p in ps} == {kind}
    ps = list(dp.chunk_paths(staged, T, max_delay))
    assert any(is_a(p) and p.nt == 512 for p in ps) and sum(at_edge(p) for p in ps) == 2
    assert sum(past_edge(p) for p in dp.chunk_paths(direct, T, max_delay)) == 2


def test_the_new_cases_close_what_the_census_found_open():
    calls = [dp.edge_case(nt, part, C) for nt in dp.EDGE_NT for part in range(dp.EDGE_PARTS) for C in dp.EDGE_C]
    calls += [dp.order_case(C) for C in dp.ORDER_C] + [dp.order_case_tiles(C) for C in dp.ORDER_C]
    calls += [dp.sweep_case(n) for n in dp.SWEEP_NR_DM]
    c = census_of((table, T, max_delay, mask) for table, mask, T, max_delay in calls)
    print("\n" + format_census(c))
    assert c["spread"]["staged", "full"] == (0, 620) == c["spread"]["staged", "partial"]
    assert c["spread"]["direct by spread", "full"] == (621, 621) == c["spread"]["direct by spread", "partial"]
    assert c["spread"]["direct by rows", "full"] == (0, 620) == c["spread"]["direct by rows", "partial"]
    assert (c["rows_inside"], c["rows_outside"]) == (0, 1) and c["orders"] == ALL_ORDERS
    assert c["nd"] == {1, 4, 5, 8, 12, 13, 16}
