"""The shapes of the down-converter's GPU tests (tests/test_gpu_ddc.py), kept here so that tests/test_launch_forms.py can take
a census of the grids they present to the kernel without a GPU."""

# one output; a tile less one; a tile; a tile and one (the second tile of a pair holds one output); two tiles and one (a second
# pair).  T: every number of K steps.  One input and several; one band and two
NR_BANDS = (1, 2)
NR_INPUTS = (1, 3)
NR_TAPS = (64, 128, 192, 256)
NR_OUT = (1, 15, 16, 17, 33)

SPANS_NR_OUT = (511, 512, 513, 1100)  # test_several_spans_and_every_wave_of_a_workgroup: two inputs
SPANS_NR_INPUTS = 2


def old_calls():
    """(nr_inputs, nr_out) of the calls of the two tables."""
    for ni in NR_INPUTS:
        for nr_out in NR_OUT:
            yield ni, nr_out
    for nr_out in SPANS_NR_OUT:
        yield SPANS_NR_INPUTS, nr_out


# the workgroups' walk over the items beyond the grid: 37 workgroups take a second row
WALK = dict(T=64, nr_out=3, in_stride=96, nr_inputs=(1 << 20) + 37)
