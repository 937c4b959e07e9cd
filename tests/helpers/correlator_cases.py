"""The case tables of the correlator's GPU tests (tests/test_gpu_correlator.py), kept here so that tests/test_launch_forms.py
can take a census of the forms they present to the kernel without a GPU."""

# one antenna; a few; one tile; a tile and one row; one unit of four tiles; ragged tiles in a second unit; every unit of the
# tile-group split.  n: one block (three zero operands), a pair, three (a ragged K group), one group and a block, two groups
STATIONS = (1, 3, 16, 17, 64, 100, 256)
BLOCKS = (1, 2, 3, 5, 8)
CHANNELS = 3

# ------------------------------------------------------------------------------------------------ the forms the census found open
#
# One A (and more) per tile count 1 .. 16, so that every (diag, sa, NA) that exists up to A = 256 is run: A % 16 is 0, 1 and
# other.  n: a masked last step, a whole last step, two steps.
FORM_STATIONS = (9, 32, 33, 50, 65, 80, 81, 96, 97, 128, 129, 150, 161, 192, 200, 224, 225, 241)
FORM_BLOCKS = (3, 4, 5)
FORM_CHANNELS = 2
NR_VIS = (1, 3)

# the walk of the waves over the items beyond the grid: A = 2, n = 1, C * nr_vis a little above 4 * 2^20 (one unit each)
WALK = dict(A=2, C=1025, nr_vis=4093, n=1)


def shape_of(A):
    """(C, the n of test_visibilities_are_the_model) of a station count of either table."""
    return (CHANNELS, BLOCKS) if A in STATIONS else (FORM_CHANNELS, FORM_BLOCKS)
