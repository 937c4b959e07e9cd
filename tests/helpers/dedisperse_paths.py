"""Which form bf_dedisperse_kernel takes per chunk ("The choice"), restated on the CPU from that
text, and seeded builders of tables whose chunks sit on the edges of the rule.  The kernel decides on the device, from the
table's contents, so no launch geometry tells a test which form ran: this model does.  Plain loops, no attempt at speed --
the tables are tiny.  tests/test_dedisperse_paths.py holds the constants to the kernel's source text and the builders to
the conditions the GPU tests rely on."""
from dataclasses import dataclass

import numpy as np

from helpers.dedisperse_model import INT32_MAX, INT32_MIN, takes_part

TILE_T = 512           # output times of a workgroup
TILE_D = 16            # DMs of a workgroup
CHUNK = 32             # columns of a chunk
WIN_BYTES = 36 << 10   # LDS of a chunk's windows
ZERO = 528             # zero bytes in front of the windows
SLACK = 16             # window bytes beyond 512 + hi - lo
MAX_PITCH = WIN_BYTES // CHUNK
MAX_SPREAD = MAX_PITCH - TILE_T - SLACK - 4  # 620


def pitch_of(spread):
    """Bytes of one column's window: 512 + spread + 16 rounded down to a dword, then made an odd number of dwords."""
    return ((TILE_T + spread + SLACK) & ~3) | 4


def rows_limit(spread):
    """The most rows rhi - rlo + nt that a staged chunk spans."""
    return 2 * pitch_of(spread) + 64


@dataclass(frozen=True)
class ChunkPath:
    dm_tile: int
    t_tile: int
    chunk: int
    kind: str              # "staged", "direct" or "none"
    spread: int            # max over the chunk's columns of hi - lo; 0 where kind is "none"
    pitch: int
    rows: int              # rhi - rlo + nt; 0 where kind is "none"
    nt: int
    nd: int
    cc: int                # the chunk's columns
    lo_residues: frozenset  # (lo - rlo) & 3 over the columns that some DM of the tile takes
    shifts: frozenset      # (d - wl) & 3 over the terms, wl = lo - ((lo - rlo) & 3)
    widest: object         # the last column of the chunk whose hi - lo is the spread; None where kind is "none"
    widest_residue: object  # its (lo - rlo) & 3
    dead: tuple            # the columns no DM of the tile takes


def chunk_paths(table, nr_spectra, max_delay, mask=None):
    """A ChunkPath per (DM tile, time tile, chunk of 32 columns), DM tiles outermost, chunks innermost: consecutive
    records of one (dm_tile, t_tile) are consecutive chunks of one workgroup."""
    table = np.asarray(table)
    on = takes_part(table, max_delay, mask)
    nr_dm, C = table.shape
    for dm0 in range(0, nr_dm, TILE_D):
        nd = min(TILE_D, nr_dm - dm0)
        for t0 in range(0, nr_spectra, TILE_T):
            nt = min(TILE_T, nr_spectra - t0)
            for c0 in range(0, C, CHUNK):
                cc = min(CHUNK, C - c0)
                where = dict(dm_tile=dm0 // TILE_D, t_tile=t0 // TILE_T, chunk=c0 // CHUNK, nt=nt, nd=nd, cc=cc)
                lo, hi = {}, {}
                for j in range(cc):
                    d = [int(table[dm0 + m, c0 + j]) for m in range(nd) if on[dm0 + m, c0 + j]]
                    if d:
                        lo[j], hi[j] = min(d), max(d)
                dead = tuple(j for j in range(cc) if j not in lo)
                if not lo:
                    yield ChunkPath(kind="none", spread=0, pitch=pitch_of(0), rows=0, lo_residues=frozenset(), shifts=frozenset(),
                                    widest=None, widest_residue=None, dead=dead, **where)
                    continue
                rlo, rhi = min(lo.values()), max(hi.values())
                spread = max(hi[j] - lo[j] for j in lo)
                pitch = pitch_of(spread)
                rows = rhi - rlo + nt
                staged = spread <= MAX_SPREAD and rows <= 2 * pitch + 64
                shifts = set()
                for j in lo:
                    wl = lo[j] - ((lo[j] - rlo) & 3)
                    shifts |= {(int(table[dm0 + m, c0 + j]) - wl) & 3 for m in range(nd) if on[dm0 + m, c0 + j]}
                widest = max(j for j in lo if hi[j] - lo[j] == spread)
                yield ChunkPath(kind="staged" if staged else "direct", spread=spread, pitch=pitch, rows=rows,
                                lo_residues=frozenset((lo[j] - rlo) & 3 for j in lo), shifts=frozenset(shifts), widest=widest,
                                widest_residue=(lo[widest] - rlo) & 3, dead=dead, **where)


def workgroups(paths):
    """{(dm_tile, t_tile): [kind per chunk]} of the records of one table."""
    out = {}
    for p in paths:
        out.setdefault((p.dm_tile, p.t_tile), []).append(p.kind)
    return out


def orders(paths):
    """The ordered pairs of kinds that consecutive chunks of one workgroup take."""
    return {(a, b) for kinds in workgroups(paths).values() for a, b in zip(kinds, kinds[1:])}


def census(paths):
    """What a set of records presents to the rule: per form (staged, direct because the spread is past 620, direct because
    of the rows alone) the smallest and the largest spread, over full and over partial tiles; the nearest approach to the
    limit on the rows from either side (limit - rows of the staged chunks, rows - limit of the chunks that are direct
    although their spread would fit); the orders of kinds; the nd seen."""
    out = {"spread": {}, "rows_inside": None, "rows_outside": None, "orders": set(), "nd": set(), "chunks": 0}
    paths = list(paths)
    out["orders"] = orders(paths)
    for p in paths:
        out["chunks"] += 1
        out["nd"].add(p.nd)
        if p.kind == "none":
            continue
        form = p.kind if p.kind == "staged" else "direct by spread" if p.spread > MAX_SPREAD else "direct by rows"
        key = (form, "full" if p.nt == TILE_T else "partial")
        lo, hi = out["spread"].get(key, (p.spread, p.spread))
        out["spread"][key] = (min(lo, p.spread), max(hi, p.spread))
        gap = 2 * p.pitch + 64 - p.rows
        if p.kind == "staged":
            out["rows_inside"] = gap if out["rows_inside"] is None else min(out["rows_inside"], gap)
        elif p.spread <= MAX_SPREAD:
            out["rows_outside"] = -gap if out["rows_outside"] is None else min(out["rows_outside"], -gap)
    return out


def merge_census(a, b):
    """The census of two sets of records taken together."""
    if a is None:
        return b
    out = {"spread": dict(a["spread"]), "orders": a["orders"] | b["orders"], "nd": a["nd"] | b["nd"], "chunks": a["chunks"] + b["chunks"]}
    for key, (lo, hi) in b["spread"].items():
        l0, h0 = out["spread"].get(key, (lo, hi))
        out["spread"][key] = (min(l0, lo), max(h0, hi))
    for key in ("rows_inside", "rows_outside"):
        both = [v for v in (a[key], b[key]) if v is not None]
        out[key] = min(both) if both else None
    return out


# ------------------------------------------------------------------------------------------------------------- edge tables
#
# A table is described per DM tile as a list of chunk templates, one per 32 columns:
#   ("edge", spread, span)            entries that take part: the widest window is `spread`, and rhi - rlo is `span`
#   ("edge", spread, span, options)   options: masked=(columns,), dead=(columns,)
#   ("none",)                         every entry outside [0, max_delay]
# An "edge" chunk of cc >= 5 columns and nd DMs is built so that, whatever the seed,
#   * its last column alone carries the widest window, lo = rlo + 3 (the last window in LDS, at the largest residue);
#   * columns 0, 1 and 2 start at rlo, rlo + 1 and rlo + 2, so all four residues of (lo - rlo) & 3 occur;
#   * column 3 ends at rhi = rlo + span;
#   * the other columns lie anywhere inside [rlo, rhi] with windows narrower than `spread`;
#   * a masked column holds entries over all of [0, max_delay], which would make the chunk direct if they counted, and a
#     dead column only entries outside [0, max_delay].
# With one DM (nd = 1) every window is one row, so `spread` must be 0.

_OUTSIDE = (-1, INT32_MIN, None, INT32_MAX)  # None: max_delay + 1


def _outside(n, max_delay, start=0):
    return [max_delay + 1 if _OUTSIDE[(start + i) % 4] is None else _OUTSIDE[(start + i) % 4] for i in range(n)]


def _column(rng, nd, lo, hi):
    """nd entries in [lo, hi] with both ends present (nd >= 2), in a seeded order."""
    if nd == 1:
        assert lo == hi
        return [lo]
    d = [lo, hi] + [int(x) for x in rng.integers(lo, hi + 1, size=nd - 2)]
    return [d[i] for i in rng.permutation(nd)]


def edge_chunk(rng, nd, cc, spread, span, max_delay, masked=(), dead=()):
    """int64 [nd][cc], as described above; rlo is seeded in [0, max_delay - span]."""
    assert cc >= 5 and span >= spread + 3 and span <= max_delay and (nd > 1 or spread == 0)
    assert not set(masked) & set(dead) and all(4 <= j < cc - 1 for j in tuple(masked) + tuple(dead))
    rlo = int(rng.integers(0, max_delay - span + 1))
    out = np.empty((nd, cc), np.int64)
    narrower = max(spread - 1, 0)
    for j in range(cc):
        if j in dead:
            out[:, j] = _outside(nd, max_delay, start=j)
        elif j in masked:
            out[:, j] = _column(rng, nd, 0, max_delay) if nd > 1 else [max_delay]
        elif j == cc - 1:
            out[:, j] = _column(rng, nd, rlo + 3, rlo + 3 + spread)
        elif j < 3:
            out[:, j] = _column(rng, nd, rlo + j, rlo + j + int(rng.integers(0, narrower + 1)))
        elif j == 3:
            out[:, j] = _column(rng, nd, rlo + span - narrower, rlo + span)
        else:
            w = int(rng.integers(0, narrower + 1))
            lo = rlo + int(rng.integers(0, span - w + 1))
            out[:, j] = _column(rng, nd, lo, lo + w)
    return out


def build_table(C, nr_dm, templates, max_delay, seed):
    """(int32 [nr_dm][C], mask uint8 [C] or None) from ``templates``: one list of chunk templates per DM tile, or one list
    for all of them.  A column is masked where any tile's template asks for it."""
    rng = np.random.default_rng(seed)
    chunks = -(-C // CHUNK)
    tiles = -(-nr_dm // TILE_D)
    if templates and isinstance(templates[0], tuple):
        templates = [templates] * tiles
    assert len(templates) == tiles and all(len(t) == chunks for t in templates)
    table = np.empty((nr_dm, C), np.int64)
    mask = np.ones(C, np.uint8)
    for k in range(tiles):
        nd = min(TILE_D, nr_dm - k * TILE_D)
        for i, tpl in enumerate(templates[k]):
            c0, cc = i * CHUNK, min(CHUNK, C - i * CHUNK)
            block = table[k * TILE_D:k * TILE_D + nd, c0:c0 + cc]
            if tpl[0] == "none":
                for j in range(cc):
                    block[:, j] = _outside(nd, max_delay, start=i + j)
                continue
            assert tpl[0] == "edge"
            options = tpl[3] if len(tpl) > 3 else {}
            block[:] = edge_chunk(rng, nd, cc, tpl[1], tpl[2], max_delay, **options)
            for j in options.get("masked", ()):
                mask[c0 + j] = 0
    return table.astype(np.int32), (None if mask.all() else mask)


MAX_DELAY = 2400           # of every edge table: a chunk of one time at the limit on the rows spans 2359 rows
D_SPREADS = tuple(range(8)) + (617, 618, 619, 620)  # every case of the pitch's two roundings, at both ends of the range
EDGE_NT = (512, 487, 1)    # a full tile; a partial one whose times are no multiple of 8; a single time
EDGE_C = (320, 317)        # ten whole chunks (dword staging); nine and one of 29 columns (byte staging)
EDGE_PARTS = 3
EDGE_T = {(512, 320): 512, (512, 317): 1024, (487, 320): 999, (487, 317): 999, (1, 320): 513, (1, 317): 1025}
PLAIN_SPAN = 700           # rhi - rlo of an edge chunk that is nowhere near the limit on the rows


def at_limit(spread, nt):
    """rhi - rlo with which a chunk of that spread spans exactly the most rows a staged chunk may, in a tile of nt times."""
    return rows_limit(spread) - nt


def edge_templates(nt, part):
    """The chunk templates of one of the EDGE_PARTS edge tables for tiles of nt times: ten chunks.  Over the parts: the
    chunk of condition (a), its direct twin at spread 621 (c), and for every spread of D_SPREADS a chunk exactly at the limit
    on the rows and one a row past it (b, d); the staged chunk at spread 620 and the limit also has a masked and a dead
    column (i).  The tenth chunk of every part, which a ragged C cuts short, is a filler far from every edge."""
    need = [("edge", 620, PLAIN_SPAN), ("edge", 621, PLAIN_SPAN)]
    for s in D_SPREADS:
        options = ({"masked": (5,), "dead": (9,)},) if s == 620 else ()
        need += [("edge", s, at_limit(s, nt)) + options, ("edge", s, at_limit(s, nt) + 1)]
    need.append(("edge", 620, 1000))
    assert len(need) == 9 * EDGE_PARTS
    return need[9 * part:9 * part + 9] + [("edge", 300, 500)]


def edge_case(nt, part, C):
    """(table, mask, T, max_delay) of one edge case: 16 DMs."""
    table, mask = build_table(C, 16, edge_templates(nt, part), MAX_DELAY, seed=1000 * nt + 10 * part + C % 2)
    return table, mask, EDGE_T[nt, C], MAX_DELAY


# staged, direct and none so that every ordered pair occurs between consecutive chunks: nine pairs in ten chunks
ORDER_KINDS = "SSDDNNSNDS"
ORDER_C = (320, 317)


def order_templates(nt, shift=0):
    """ORDER_KINDS rotated left by ``shift``, as templates: the staged chunks alternate between condition (a)'s and the
    limit on the rows, the direct ones between spread 621 and one row past that limit."""
    staged = [("edge", 620, PLAIN_SPAN), ("edge", 620, at_limit(620, nt))]
    direct = [("edge", 621, PLAIN_SPAN), ("edge", 620, at_limit(620, nt) + 1)]
    kinds = ORDER_KINDS[shift:] + ORDER_KINDS[:shift]
    out, seen = [], {"S": 0, "D": 0}
    for k in kinds:
        if k == "N":
            out.append(("none",))
        else:
            out.append((staged if k == "S" else direct)[seen[k] % 2])
            seen[k] += 1
    return out


def order_case(C):
    """One workgroup's row of chunks per beam: 16 DMs, 512 times."""
    table, mask = build_table(C, 16, order_templates(512), MAX_DELAY, seed=900 + C)
    return table, mask, 512, MAX_DELAY


def order_case_tiles(C):
    """Two DM tiles (16 and 13 DMs) and two time tiles (512 times and 1): the second DM tile's kinds are rotated by one
    chunk (which keeps all nine orders: the pair it parts and the pair it joins are both staged to staged), and the chunks
    at the limit on the rows are built for the tile of one time, so they are staged there and direct in the full tile
    beside it."""
    table, mask = build_table(C, 29, [order_templates(1), order_templates(1, shift=1)], MAX_DELAY, seed=950 + C)
    return table, mask, 513, MAX_DELAY


SWEEP_C = 128
SWEEP_NR_DM = (4, 5, 8, 12, 13, 16, 17, 20, 29, 33)  # nd 4, 5, 8, 12, 13, 16 alone; 1, 4, 13 behind a full tile; 1 behind two


def sweep_case(nr_dm):
    """Four chunks: condition (a)'s, its direct twin, and spread 0 at and past the limit on the rows.  A tile of one DM has
    no spread, so its first two chunks are at and past the limit as well."""
    many = [("edge", 620, PLAIN_SPAN), ("edge", 621, PLAIN_SPAN), ("edge", 0, at_limit(0, 512)), ("edge", 0, at_limit(0, 512) + 1)]
    one = [("edge", 0, at_limit(0, 512)), ("edge", 0, at_limit(0, 512) + 1), ("edge", 0, PLAIN_SPAN), ("edge", 0, at_limit(0, 512))]
    tiles = -(-nr_dm // TILE_D)
    templates = [one if min(TILE_D, nr_dm - k * TILE_D) == 1 else many for k in range(tiles)]
    table, mask = build_table(SWEEP_C, nr_dm, templates, MAX_DELAY, seed=700 + nr_dm)
    return table, mask, 512, MAX_DELAY


REPLAY_C = 96


def replay_tables():
    """Three tables of 16 DMs x 96 columns for one captured call of 513 times: every chunk staged in both time tiles
    (condition (a)'s, and two at the limit on the rows of the full tile), the same chunks direct in both (spread 621, and a
    row past the limit of the tile of one time), and no term at all.  ([staged, direct, none], nr_spectra, max_delay)."""
    staged = [("edge", 620, PLAIN_SPAN), ("edge", 620, at_limit(620, 512)), ("edge", 3, at_limit(3, 512))]
    direct = [("edge", 621, PLAIN_SPAN), ("edge", 620, at_limit(620, 1) + 1), ("edge", 3, at_limit(3, 1) + 1)]
    templates = (staged, direct, [("none",)] * 3)
    return [build_table(REPLAY_C, 16, t, MAX_DELAY, seed=800 + i)[0] for i, t in enumerate(templates)], 513, MAX_DELAY
