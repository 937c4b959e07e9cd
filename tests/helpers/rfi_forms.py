"""Which form the RFI flagger's kernels take for a shape (dc_sand_amd/csrc/bf_rfi.hip; DESIGN.md section 5.23, "The forms"),
restated on the CPU.  The launcher picks the two hot kernels' unit U and lanes L from C alone, and the flags kernels pick
theirs from C, nr_blocks and the window, so a shape names its forms.  tests/test_rfi_forms.py holds these constants and rules
to the kernel's source text and takes the census of the GPU tests' tables with them."""
from dataclasses import dataclass

THREADS = 256          # of a workgroup of the two hot kernels
LANE_CHANNELS = 16     # channels a lane holds
MAX_LANES = 64         # lanes of one row in a workgroup
CELL_CACHE = 4096      # channels whose m and q bf_rfi_cell_flags_kernel keeps in LDS
BEAM_THREADS = 1024
BEAM_WORDS = 16        # zero-DM words a thread of bf_rfi_beam_kernel keeps in registers
BEAM_UNROLL = 8        # blocks its bad-block loop takes at a time
ON_CHIP_SPECTRA = BEAM_THREADS * BEAM_WORDS
M_BITS, Q_BITS = 24, 49  # of select_rank's bisections, two bits a pass

ALL_UNITS = (16, 4, 1)
ALL_LANES = (1, 2, 4, 8, 16, 32, 64)


def lanes_of(C):
    """Lanes of 16 channels that a row of C channels needs, as a power of two <= 64."""
    need = (C + LANE_CHANNELS - 1) // LANE_CHANNELS
    lanes = 1
    while lanes < need and lanes < MAX_LANES:
        lanes <<= 1
    return lanes


def unit_of(C):
    """Bytes of one row access: the kernel template's U."""
    return 16 if C % 16 == 0 else 4 if C % 4 == 0 else 1


def at_of(U, i, j, L):
    """Where channel i = 0 .. 15 of lane j lies in the tile."""
    return LANE_CHANNELS * j + i if U == 16 else 4 * ((i >> 2) * L + j) + (i & 3) if U == 4 else i * L + j


def zero_dm_form(L):
    """("rows", trips) below four lanes: every row is summed on its own, in log2 L exchanges; ("quads", trips) from four
    lanes on: four rows in 2 + 1 exchanges and then `trips` plain halvings, x = 4 .. L / 2."""
    log2 = L.bit_length() - 1
    return ("rows", log2) if L < 4 else ("quads", log2 - 2)


@dataclass(frozen=True)
class Tile:
    width: int      # the tile's channels that exist, 1 .. 16 L
    lanes_on: int   # lanes that have a channel at all
    kind: str       # "full", "partial" (every lane on, some without all 16 channels) or "lanes off"


@dataclass(frozen=True)
class HotForm:
    U: int
    L: int
    R: int          # rows a workgroup takes side by side
    tiles: int
    zero_dm: tuple
    kinds: frozenset  # of its tiles


def tiles_of(C):
    U, L = unit_of(C), lanes_of(C)
    span = LANE_CHANNELS * L
    out = []
    for c0 in range(0, C, span):
        width = min(span, C - c0)
        on = sum(at_of(U, 0, j, L) < width for j in range(L))
        out.append(Tile(width, on, "full" if width == span else "partial" if on == L else "lanes off"))
    assert len(out) == (C - 1) // span + 1
    return out


def hot_form(C):
    L = lanes_of(C)
    tiles = tiles_of(C)
    return HotForm(unit_of(C), L, THREADS // L, len(tiles), zero_dm_form(L), frozenset(t.kind for t in tiles))


def hot_forms_that_exist(top=8192):
    """Every (U, L) pair, and every (U, L, kind of tile), that some C up to ``top`` has."""
    pairs, kinds = set(), set()
    for C in range(1, top + 1):
        f = hot_form(C)
        pairs.add((f.U, f.L))
        kinds |= {(f.U, f.L, k) for k in f.kinds}
    return pairs, kinds


def beam_unroll(nr_blocks):
    """(trips of the loop that takes eight blocks, blocks of its tail)."""
    return nr_blocks // BEAM_UNROLL, nr_blocks % BEAM_UNROLL


def on_chip(C, nr_blocks, block_len):
    """(the cell kernel keeps m and q in LDS, the beam kernel keeps the zero-DM series in registers)."""
    return C <= CELL_CACHE, nr_blocks * block_len <= ON_CHIP_SPECTRA


def census(channels):
    """What a list of C presents to the two hot kernels: the (U, L) pairs, the (U, L) pairs met with lanes off, the zero-DM
    forms."""
    forms = [hot_form(C) for C in channels]
    return {"pairs": {(f.U, f.L) for f in forms}, "lanes off": {(f.U, f.L) for f in forms if "lanes off" in f.kinds},
            "zero-DM": {f.zero_dm for f in forms}}


def flags_census(calls):
    """What (C, nr_blocks, block_len) calls present to the two flags kernels."""
    calls = list(calls)
    return {"unroll": {(min(t, 2), min(tail, 1)) for t, tail in (beam_unroll(nb) for _, nb, _ in calls)},
            "unroll at C >= 64": {(min(t, 2), min(tail, 1)) for t, tail in (beam_unroll(nb) for C, nb, _ in calls if C >= 64)},
            "cells on chip": {(C <= CELL_CACHE, C) for C, _, _ in calls if abs(C - CELL_CACHE) <= 1},
            "window on chip": {(nb * n <= ON_CHIP_SPECTRA, nb * n) for _, nb, n in calls if abs(nb * n - ON_CHIP_SPECTRA) <= 1}}


def format_census(name, c):
    lines = [f"{name}:"]
    for U in ALL_UNITS:
        lines.append(f"  U {U:2}: L " + " ".join(f"{L}{'*' if (U, L) in c['lanes off'] else ''}" for L in ALL_LANES if (U, L) in c["pairs"]))
    lines.append("  (* with whole lanes off)   zero-DM: " + " ".join(f"{k}/{t}" for k, t in sorted(c["zero-DM"])))
    return "\n".join(lines)
