"""The shapes of the candidate sifter's GPU tests (tests/test_gpu_candidates.py) that decide which take_widths calls a cell
makes, kept here so that tests/test_launch_forms.py can take a census of them without a GPU, and the planes of the test of
every unrolled chain, whose conditions are asserted on the numpy model before a GPU sees them."""
import numpy as np

from helpers.candidates_model import seeded_planes

RAGGED = (2, 37, 3, 200)       # B, nr_dm, nr_widths, peak_blocks of ragged_planes
BORDER_WIDTHS = 2              # test_equal_maxima_across_tile_borders_and_halo_corners
SCAN = (2, 600, 2, 1100)       # B, nr_dm, nr_widths, nr_blocks of test_more_segments_than_two_rounds_of_the_scan
FLAT_WIDTHS = 1                # the plateau of test_every_cell_a_candidate_and_none
BEST_WIDTHS = [4, 1, 33, 16, 0, 4, 32]  # test_width_index_is_the_best_width_of_peak_snr
SHORT = (2, 20, 3, 80)         # test_short_buffers_are_refused_and_nothing_is_enqueued
CAPTURE = (2, 37, 3, 140)      # test_captured_on_first_use_and_replayed_with_new_contents
CHAIN_WIDTHS = 6               # helpers/single_pulse_model.CHAIN, and the example


def old_nr_widths():
    """nr_widths of every find_candidates call of the tests as they were."""
    return sorted({RAGGED[2], BORDER_WIDTHS, SCAN[2], FLAT_WIDTHS, 0, len(BEST_WIDTHS), SHORT[2], CAPTURE[2], CHAIN_WIDTHS})


# -------------------------------------------------------------------------------------------------- every unrolled chain
#
# One, two and three eights alone and with a one behind; an eight with three ones, with the four, with the four and a one.
FORM_NR_WIDTHS = (8, 9, 11, 12, 13, 16, 17, 24, 25)
FORM_SHAPE = (1, 20, 70)       # B, nr_dm, blocks
FORM_RADII = ((0, 0), (1, 1))
FORM_THRESHOLD = 6.0
TIE_PAIRS = ((7, 8), (11, 12), (3, 15))  # equal maxima at two width indices: across the first eight's end, the four's, far apart


def hand_cells(nr_widths):
    """{(dm, block): (the values of the cell {width index: value}, -inf elsewhere; the width index that must win)}: equal
    maxima at two indices (the lower wins), the same with a NaN at one of the two (the other wins), and a cell that is
    -infinity in all widths but the last.  Every value is above everything else in the plane, and the cells are three blocks
    apart: each is a candidate at both radii."""
    cells, k = {}, 30
    pairs = [p for p in TIE_PAIRS if p[1] < nr_widths] + [(0, nr_widths - 1)]
    for lo, hi in pairs:
        cells[(5, k)] = ({lo: 50.0, hi: 50.0}, lo)
        cells[(9, k)] = ({lo: np.nan, hi: 51.0}, hi)
        cells[(13, k)] = ({lo: 52.0, hi: np.nan}, lo)
        k += 3
    cells[(17, 30)] = ({nr_widths - 1: 53.0}, nr_widths - 1)
    return cells


def form_planes(nr_widths):
    """(snr, peaks) of FORM_SHAPE: seeded values below 10 with few ties; width index i alone holds 20 + i at cell
    (2 (i % 10), 2 + 4 (i // 10)) -- a local maximum at both radii, so every width index wins somewhere -- and the hand-made
    cells."""
    B, nr_dm, blocks = FORM_SHAPE
    snr, peaks = seeded_planes(B, nr_dm, nr_widths, blocks, seed=700 + nr_widths, plateau=False, step=1024)
    for i in range(nr_widths):
        snr[0, 2 * (i % 10), i, 2 + 4 * (i // 10)] = 20.0 + i
    for (m, k), (values, _) in hand_cells(nr_widths).items():
        snr[0, m, :, k] = -np.inf
        for i, v in values.items():
            snr[0, m, i, k] = v
    return snr, peaks
