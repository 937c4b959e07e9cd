"""The parametrisations of tests/test_gpu_channeliser.py that hold an output to the model on seeded data, kept here so that
tests/test_channeliser_model.py can count, without a GPU, which of the kernel's instantiations they run."""

SIZES = (64, 128, 256, 512, 1024, 2048)  # test_the_float_output_is_the_model_in_its_place: every N

# test_the_quantised_output_is_the_model_and_the_float_output_quantised: N, P, inputs, spectra.  Every N, because every int8
# epilogue has a lane map of its own, made when compiling.
QUANTISED_CASES = ((64, 4, 3, 32), (256, 5, 2, 16), (2048, 16, 1, 16), (128, 3, 5, 16), (512, 2, 3, 32), (1024, 5, 2, 16))


def instantiations():
    """The (log2 N, int8 epilogue) pairs those two tests run."""
    return {(N.bit_length() - 1, False) for N in SIZES} | {(c[0].bit_length() - 1, True) for c in QUANTISED_CASES}
