"""The blocks-per-output counts of the integrator's GPU tests (bf_integrate.hip through test_gpu_beam_power.py,
test_gpu_incoherent_beam.py, test_gpu_stokes.py and test_gpu_correlator.py), kept here so that tests/test_launch_forms.py can
take a census of the unrolled trips and tails they present to the kernel without a GPU."""

# (n, accumulates too) per word type of the integration tests as they were; nblk is the shape's own block count
OLD_F32_NBLK = (4, 6, 16, 2)        # test_integration_is_the_ordered_sum: n in (1, 2, nblk)
OLD_U32 = (1, 2, 16, 6, 3, 12, 40)  # the exact-sum test (1, 2, nblk), several workgroups (1, 2), bit 31 (1, 2, 3, 12), full scale 40
OLD_I32 = (1, 2, 3, 12)             # Stokes (1, 2, 3, nblk); visibilities (1, 3)


def old_calls():
    """(kind, n, accumulate) of the older tests."""
    for nblk in OLD_F32_NBLK:
        for n in (1, 2, nblk):
            yield "f32", n, False
            yield "f32", n, True
    for kind, ns in (("u32", OLD_U32), ("i32", OLD_I32)):
        for n in ns:
            yield kind, n, False
            yield kind, n, True


# no trip, one and two full trips of the float loop's four and of the integer loops' eight, each with and without a tail
FORM_N = (1, 2, 3, 4, 5, 8, 9, 16, 17)
FORM_NBLK = 12240  # the least common multiple of FORM_N


def form_calls():
    for kind in ("f32", "u32", "i32"):
        for n in FORM_N:
            yield kind, n, False
            yield kind, n, True
