"""The case tables of the RFI flagger's GPU tests (tests/test_gpu_rfi.py), kept here so that tests/test_rfi_forms.py can take
a census of the forms they present to the kernels without a GPU, and the hand-made cell sums of the flags tests, which are
conditions on the model alone before a GPU sees them."""
import numpy as np

from helpers import rfi_model as rm

# ------------------------------------------------------------------------------------------------------------------ moments

CHANNELS = [1, 3, 16, 64, 100, 1000, 4100]
MORE_CHANNELS = [1040, 1030, 20]  # two tiles of channels, the second a part of one: rows in 16-byte units, and in single bytes; two lanes a row
BLOCK_LENS = [1, 2, 5, 16, 257, 258, 1000]
LIMIT = 12 << 20


def moments_cases():
    """Every C with every block_len, while nr_blocks, B and first_spectrum rotate at different periods; the largest are cut
    to one beam and at most two blocks, so that the model stays quick: C -> [(block_len, nr_blocks, B, first)]."""
    out = {}
    for ci, C in enumerate(CHANNELS + MORE_CHANNELS):
        out[C] = []
        for i, n in enumerate(BLOCK_LENS):
            nb, B, first = (1, 2, 7)[(i + ci) % 3], (1, 3)[(i + ci // 2) % 2], (0, 5)[(i // 2 + ci) % 2]
            if B * nb * n * C > LIMIT:
                nb, B = min(nb, 2), 1
            out[C].append((n, nb, B, first))
    return out


# -------------------------------------------------------------------------------------------------------------------- clean

CLEAN_CHANNELS = [3, 64, 100, 1030, 1040, 4100]


def clean_shape(C):
    """(B, nr_blocks, block_len, first, first_out) of test_clean_is_the_model."""
    return (3, 7, 5, 2, 4) if C < 4100 else (2, 2, 37, 1, 0)


# ---------------------------------------------------------------------------------------------- the forms the census found open
#
# The (U, L) pairs -- the unit of a row access and the lanes of a row -- that the tables above leave out, for the moments and
# for the clean kernel, and the partial tiles with whole lanes off at every L that has them.  The first four: L = 16 with lanes
# 9 .. 15 off (U 16), L = 16 partial (U 4), L = 32 partial (U 1), L = 32 full (U 16).

FORM_CHANNELS = [144, 200, 257, 512,
                 16, 32, 128,        # U 16: L 1, 2, 8
                 4, 20, 36, 260,     # U 4: L 1, 2, 4, 32
                 17, 33, 65, 129,    # U 1: L 2, 4, 8, 16
                 48, 80, 272]        # U 16 with lanes off at L 4, 8, 32
FORM_BLOCK_LENS = [1, 5, 258]


def form_cases():
    """C -> [(block_len, nr_blocks, B, first)]: every block length, nr_blocks and B rotating through 1, 2, 3, and
    first_spectrum != 0 once per C."""
    out = {}
    for ci, C in enumerate(FORM_CHANNELS):
        out[C] = [(n, (1, 2, 3)[(i + ci) % 3], (3, 1, 2)[(i + 2 * ci) % 3], 3 if i == ci % 3 else 0) for i, n in enumerate(FORM_BLOCK_LENS)]
    return out


# clean with the flag tensors at byte offsets inside larger allocations: C -> offsets (U 16, and U 4)
OFFSET_CASES = {64: (1, 4, 8), 100: (1, 2, 3)}
OFFSET_SHAPE = (2, 3, 5, 1)  # B, nr_blocks, block_len, first

# -------------------------------------------------------------------------------------------------------------------- flags

FLAGS_CHANNELS = CHANNELS
ONE_AND_TWO_CHANNELS = (4, 10)  # nr_blocks, block_len of test_flags_of_one_and_two_channels


def own_sums_shapes(C):
    """(block_len, nr_blocks, B) of test_flags_of_the_devices_own_sums."""
    return ((16, 7, 3), (257, 2, 1)) if C < 4100 else ((16, 7, 1), (5, 2, 3))


ON_CHIP_CASES = [(4096, 4, 4096), (4100, 5, 3277), (4100, 3, 3000), (4097, 1, 16385)]  # C, nr_blocks, block_len

UNROLL_C, UNROLL_B, UNROLL_LEN = 70, 2, 16
UNROLL_NR_BLOCKS = (8, 9, 17)
UNROLL_MAX_BAD = (0, 1, 2)

TOP_BITS_C, TOP_BITS_LEN = 70, 65536


def flags_calls():
    """(C, nr_blocks, block_len) of every dcs_bf_rfi_flags call of the tables above and of the hand-made cases."""
    for C in FLAGS_CHANNELS:
        for n, nb, _ in own_sums_shapes(C):
            yield C, nb, n
    yield from ((5, 1, 1), (5, 1, 3), (5, 1, 2), (5, 8, 1), (5, 5, 1))  # test_flags_of_hand_made_sums
    yield from ((C, *ONE_AND_TWO_CHANNELS) for C in (1, 2))
    yield from ON_CHIP_CASES
    yield 16, 2, 65536      # test_moments_of_the_longest_block_at_full_scale
    yield 256, 16, 64       # the recipe
    yield 100, 5, 24        # the captured chain
    yield 64, 7, 32         # filterbank_q8 into rfi into dedisperse (nr_blocks from its delays)


def new_flags_calls():
    for nb in UNROLL_NR_BLOCKS:
        yield UNROLL_C, nb, UNROLL_LEN
    yield TOP_BITS_C, len(top_bits_blocks()), TOP_BITS_LEN


# ------------------------------------------------------------------------------------- hand-made sums: the beam kernel's unroll

def unroll_bad_cells(nr_blocks):
    """{channel: [bad blocks]} of beam 0 (beam 1 has the same a channel further on): 1, 2 and 3 bad cells in the part of
    the blocks that the beam kernel's loop takes eight at a time (blocks below U = 8 (nr_blocks // 8)), in its tail, and in
    both, the last unrolled and the first tail block among them."""
    U = 8 * (nr_blocks // 8)
    bad = {3: [0], 5: [0, 7], 9: [1, 4, U - 1], 69: [U - 1]}
    if U > 8:
        bad.update({50: [8, 15], 51: [7, 8, U - 1], 52: [6, 9]})
    if nr_blocks > U:
        bad.update({12: [U], 20: [0, U], 33: [2, 5, U], 40: [U - 1, U], 41: [nr_blocks - 1, 3, U - 8]})
    return bad


def unroll_filterbank(nr_blocks):
    """uint8 [2][nr_blocks * 16][70]: channel c holds the byte 100 + c % 7 in every row, 60 more in its bad cells.  Every
    q is 0, so only the means flag: a block's m are 16 (100 .. 106), MAD 32, and a bad cell lies 16 * 54 or more away."""
    C, B, n = UNROLL_C, UNROLL_B, UNROLL_LEN
    fb = np.empty((B, nr_blocks * n, C), np.uint8)
    fb[:] = 100 + np.arange(C) % 7
    for c, blocks in unroll_bad_cells(nr_blocks).items():
        for beam in range(B):
            for k in blocks:
                fb[beam, k * n:(k + 1) * n, (c + beam) % C] += 60
    return fb


def unroll_expected_bad(nr_blocks):
    """uint [2][70]: the bad cells per channel that unroll_filterbank was made for."""
    bad = np.zeros((UNROLL_B, UNROLL_C), np.int64)
    for c, blocks in unroll_bad_cells(nr_blocks).items():
        for beam in range(UNROLL_B):
            bad[beam, (c + beam) % UNROLL_C] = len(blocks)
    return bad


# --------------------------------------------------------------------------------- hand-made sums: the top bits of m and of q

def cell_of(counts):
    """{s1, s2} of a block whose bytes are ``counts``: {value: how many}, block_len of them in all."""
    assert sum(counts.values()) == TOP_BITS_LEN and all(0 <= v <= 255 and k >= 0 for v, k in counts.items())
    s1, s2 = sum(v * k for v, k in counts.items()), sum(v * v * k for v, k in counts.items())
    assert s2 < 1 << 32
    return s1, s2


def cell_of_mean(m):
    """A cell of sum m from bytes 255, one byte of the remainder, and zeros."""
    k, r = divmod(m, 255)
    counts = {255: k, 0: TOP_BITS_LEN - k}
    if r:
        counts[0] -= 1
        counts[r] = 1
    return cell_of(counts)


def cell_of_halves(a, b):
    """Half the bytes a, half b: q = (a - b)^2 2^30."""
    return cell_of({a: TOP_BITS_LEN // 2, b: TOP_BITS_LEN // 2} if a != b else {a: TOP_BITS_LEN})


def top_bits_blocks():
    """Blocks of 70 cells each, as lists of {s1, s2}, block_len 65536:
    0  m spread evenly over [0, 255 * 65536], the cell of half 0 and half 255 -- the largest q there is -- among them;
    1  m clustered at 150 * 65536 (above 2^23), with cells below 2^22, between 2^22 and 2^23 and at the top far out;
    2  the same around 100 * 65536 (between 2^22 and 2^23);
    3  the same around 40 * 65536 (below 2^22);
    4  cells of half a, half b with a - b spread over 0 .. 255: q = (a - b)^2 2^30 up to 65025 * 2^30, m near 2^23;
    5  a cluster at 2^23 + 100 whose distances 0, d, 1.5 d and 2 d have d = 2^22 + 8: the limit ON a cell at thr = 2."""
    C, n = TOP_BITS_C, TOP_BITS_LEN
    rng = np.random.default_rng(65536)
    top = 255 * n
    spread = [cell_of_mean(round(c * top / (C - 1))) for c in range(C)]
    spread[35] = cell_of_halves(0, 255)
    blocks = [spread]
    far = [1000, 3_000_000, (1 << 22) - 1, 1 << 22, 5_000_000, (1 << 23) - 1, 1 << 23, 12_000_000, top - 1, top]
    for centre in (150, 100, 40):
        near = [int(x) for x in centre * n + rng.integers(-40_000, 40_001, size=C - len(far))]
        blocks.append([cell_of_mean(m) for m in near + far])
    halves = []
    for c in range(C):
        d = round(c * 255 / (C - 1))
        b = (255 - d) // 2
        halves.append(cell_of_halves(b + d, b))
    blocks.append(halves)
    med, d = (1 << 23) + 100, (1 << 22) + 8
    edge = [med - 2 * d] + [med - d] * 17 + [med] * 17 + [med + d] * 33 + [med + d + d // 2, top]
    blocks.append([cell_of_mean(m) for m in edge])
    out = np.array(blocks, np.uint64)                     # [blocks][C][2]
    for k in range(len(blocks)):                          # a seeded order of the channels per block
        out[k] = out[k][rng.permutation(C)]
    return out


def top_bits_sums():
    """Cell sums uint32 [1][6][70][2]."""
    return top_bits_blocks()[None].astype(np.uint32)


TOP_THRESHOLDS = rm.Thresholds(3.0, 0.0, 3.0, 0.0)


def m_and_q(cs, n):
    """(m, q) as uint64 of cell sums uint32 [...][2]."""
    s = cs.astype(np.uint64)
    return s[..., 0], np.uint64(n) * s[..., 1] - s[..., 0] * s[..., 0]


def top_bits_thresholds(cs):
    """The thresholds the GPU test runs the top-bit sums with: the ones held to their conditions above."""
    n = TOP_BITS_LEN
    m, q = m_and_q(cs, n)
    out = [TOP_THRESHOLDS, rm.Thresholds(), rm.Thresholds(2.0, 0.0, 2.0, 0.0, max_bad_blocks=2),
           rm.Thresholds(float(np.nextafter(2.0, 0.0)), 0.0, 1e300, 0.0), rm.Thresholds(1.5, 0.0, 1.5, 0.0), rm.Thresholds(1.4999, 0.0, 1e300, 0.0)]
    for values, which in ((m, "m"), (q, "q")):
        _, top = top_cell_and_its_distance(values[0, 0])
        for floor in (top, float(np.nextafter(top, 0.0))):
            out.append(rm.Thresholds(0.0, floor, 0.0, 1e300) if which == "m" else rm.Thresholds(0.0, 1e300, 0.0, floor))
    return out


def top_cell_and_its_distance(values):
    """(the channel of the largest of a block's values, its distance from their lower median as a float64, exact)."""
    at = int(np.argmax(values))
    d = int(values[at]) - int(rm.lower_median(values)[0])
    assert float(d) == d
    return at, float(d)
