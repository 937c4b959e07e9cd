"""The case tables of the incoherent beam's GPU tests (tests/test_gpu_incoherent_beam.py), kept here so that
tests/test_launch_forms.py can take a census of the forms they present to the kernel without a GPU."""

# a single row; rows that could share a wave's load; both sides of a wave-load boundary (32 antennas); a last partial
# load; every loads-per-row count's neighbourhood; row counts odd and no multiple of any rows-per-wave choice
SHAPES = [(1, 1, 16), (3, 5, 48), (8, 4, 32), (31, 3, 48), (32, 3, 48), (33, 3, 48), (64, 7, 64), (65, 2, 48), (130, 4, 16),
          (255, 2, 32), (256, 3, 80), (64, 1, 1600)]

# both sides of every other wave-load boundary: loads per row 3 to 8, each whole and with a ragged last load; 5 to 15 rows, an
# odd count that is no multiple of the two rows a wave carries at 3 and 4 loads
FORM_SHAPES = [(96, 3, 48), (97, 5, 48), (128, 3, 80), (129, 3, 48), (160, 1, 112), (161, 3, 48), (192, 5, 16), (193, 3, 48),
               (224, 7, 16), (225, 3, 48)]

# SHAPES have 25 groups of rows at the most, and the kernel's grid holds 2048 workgroups x 4 waves: no wave takes a second
# trip of its loop over the row groups.  These have 1.25 to 1.35 times 8192 groups, and an odd row count that is no multiple of the rows a
# wave carries per trip (A, C, nt, those rows: 8 / loads per row, a load being 32 antennas): (1 load, 8 rows), (3 loads, 2
# rows, ragged), (8 loads, 1 row, ragged)
LOOPING_SHAPES = [(32, 1283, 1040, 8), (65, 1283, 272, 2), (255, 643, 256, 1)]

# (4 loads, 2 rows, ragged): two rows of four loads, all eight in flight -- the form no older shape of either table has
FORM_LOOPING_SHAPES = [(97, 1283, 272, 2)]
