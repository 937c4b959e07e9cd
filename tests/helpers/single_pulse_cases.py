"""The width lists and shapes of the boxcar-peak calls of tests/test_gpu_single_pulse.py, kept here so that
tests/test_launch_forms.py can take a census of the (batch, block) walks they present to the kernel without a GPU."""
from helpers.single_pulse_model import CHAIN, NO_TIME

WIDTHS_5 = [3, 7, 1, 100, 7]
EDGE_T = (1, 63, 64, 65, 1000)                       # test_block_and_window_edges, block_len 64
RUNS = [(5000, 64, 33), (5000, 4096, 4096), (9000, 192, 2000), (4097, 1024, 1)]  # T, block_len, max_width
POWERS = [1 << k for k in range(13)]
MIXED = [0, 3, 7, 101, 1, NO_TIME, 100, 7, 4096]
NONE = [0, 101]


def run_widths(max_width):
    return sorted({1, 2, max_width // 3 + 1, max_width})


def old_peaks_calls():
    """(nr_widths, T, block_len) of every dcs_bf_boxcar_peaks call of the tests as they were."""
    for T in EDGE_T:
        yield len(WIDTHS_5), T, 64
    yield len(WIDTHS_5), 100, 4096
    yield len(WIDTHS_5), 300, 128
    for T, block_len, max_width in RUNS:
        yield len(run_widths(max_width)), T, block_len
    yield 1, 130, 64
    yield len(POWERS), 130, 64
    for widths in (WIDTHS_5, MIXED, NONE):
        yield len(widths), 300, 64
    yield 2, 700, 256      # ties
    yield 2, 256, 256
    yield 3, 200, 64       # wraps
    yield 4, 2000, 128
    yield 4, 200, 64       # refusals
    yield 4, 700, 128      # the captured calls
    yield len(CHAIN["widths"]), CHAIN["outputs"] - CHAIN["max_width"] + 1, CHAIN["block_len"]


# ------------------------------------------------------------------------------------------- batches and blocks in every order
#
# One to five batches of eight widths (a last batch of one, of eight) against runs of one to five blocks and of seven: where
# the run is shorter than the four waves a wave skips batches, and from five batches on it does so more than once; eight
# batches, so that with a single block every wave still takes two pairs.
WALK_NR_WIDTHS = (8, 9, 16, 17, 25, 33, 40, 57)
WALK_NB = (1, 2, 3, 4, 5, 7)
WALK_BLOCK_LEN = 64
WALK_MAX_WIDTH = 64
WALK_LONG_T = 4096 + 100       # a run of 64 blocks and a second workgroup with two
WALK_LONG_NR_WIDTHS = (17, 40)


def walk_T(nb):
    """Times of nb blocks of 64, the last one ragged."""
    return WALK_BLOCK_LEN * nb - 5


def walk_widths(nr_widths):
    """Widths in [1, 64], no two neighbours alike, with widths that take no part in the second batch (0, its first) and in
    the last (max_width + 1, its last)."""
    widths = [1 + (7 * i) % WALK_MAX_WIDTH for i in range(nr_widths)]
    if nr_widths > 8:
        widths[8] = 0
    if nr_widths > 9:
        widths[nr_widths - 1] = WALK_MAX_WIDTH + 1
    return widths


def walk_calls():
    """(nr_widths, T, block_len) of test_batches_and_blocks_in_every_order."""
    for nw in WALK_NR_WIDTHS:
        for nb in WALK_NB:
            yield nw, walk_T(nb), WALK_BLOCK_LEN
    for nw in WALK_LONG_NR_WIDTHS:
        yield nw, WALK_LONG_T, WALK_BLOCK_LEN
