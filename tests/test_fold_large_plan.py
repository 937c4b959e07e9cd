"""The plan of tests/test_gpu_fold_large.py, without a device: that the filterbank and the profiles pass 2^32 bytes where the
plan says, that the pattern's period does not divide 2^32, and -- the CPU stand-in for "would fail if the kernels' offsets were
32-bit" -- that the profiles folded from rows read 4 GiB low differ from the right ones, and that a profile word stored 4 GiB low
lands in sub-integrations which the test reads and expects to hold something else."""
import numpy as np

from helpers import fold_large as fl
from helpers import large_tensor as lt


def test_sizes_lines_and_period():
    assert fl.NBYTES == lt.LINE + 2 * 2048 * fl.C and fl.IN_SPECTRA * fl.C < lt.LINE
    assert fl.LINE_ROW == (1 << 25) - 2048 and (fl.IN_SPECTRA + fl.LINE_ROW) * fl.C == lt.LINE
    assert fl.WINDOW == 8192 and fl.FIRST_AT_LINE + fl.WINDOW == fl.IN_SPECTRA  # the window ends where the tensor ends
    assert fl.FIRST_AT_LINE + fl.WINDOW // 2 == fl.LINE_ROW                     # half of it on either side of the line, in beam 1
    assert fl.B * (fl.IN_SPECTRA - 2048) * fl.C <= lt.LINE                      # with 2048 rows fewer nothing would lie above the line
    pat = fl.pattern(71)
    assert pat.dtype == np.uint8 and pat.shape[0] % 2 == 1 and lt.LINE % pat.nbytes != 0 and pat.nbytes <= lt.HOST_LIMIT
    assert np.unique(pat).size == 256
    assert fl.delays(82).max() == fl.MAX_DELAY and np.all(fl.delays(82)[:, -1] == fl.MAX_DELAY)
    # the profiles: just over 2^13 sub-integrations, the smallest even count above the line that holds half a call
    assert fl.SUBINT_BYTES == 1 << 18 and fl.PROFILES_BYTES == lt.LINE + (1 << 23) and fl.OUT_SUBINTS * fl.SUBINT_BYTES < lt.LINE
    assert fl.LINE_SUB == (1 << 13) - 16 and (fl.OUT_SUBINTS + fl.LINE_SUB) * fl.SUBINT_BYTES == lt.LINE
    assert fl.FIRST_SUB_AT_LINE + fl.SHORT_SUBINTS // 2 == fl.LINE_SUB and fl.FIRST_SUB_AT_LINE + fl.SHORT_SUBINTS <= fl.OUT_SUBINTS
    assert fl.FIRST_SUB_BELOW + fl.SHORT_SUBINTS <= fl.FIRST_SUB_AT_LINE


def test_a_wrapped_read_would_show():
    pat = fl.pattern(71)
    right, hits = fl.expected_fold(pat, fl.FIRST_AT_LINE)
    wrong, whits = fl.expected_fold(pat, fl.FIRST_AT_LINE, wrapped=True)
    assert np.array_equal(hits, whits) and np.all(hits.sum(axis=-1) == fl.SUBINT_LEN)
    # beam 0 reads the same bytes either way, and so do the sub-integrations of beam 1 that end below the line
    assert np.array_equal(right[0], wrong[0])
    below = [s for s in range(fl.NR_SUBINTS) if fl.FIRST_AT_LINE + (s + 1) * fl.SUBINT_LEN + fl.MAX_DELAY <= fl.LINE_ROW]
    above = [s for s in range(fl.NR_SUBINTS) if fl.FIRST_AT_LINE + s * fl.SUBINT_LEN >= fl.LINE_ROW]
    assert below == [0] and above == [3]  # 1 and 2 straddle the line, with their delays
    assert np.array_equal(right[1, below], wrong[1, below])
    # above the line nearly every word that was hit differs
    hit = hits[1, 3] > 0
    assert hit.sum() > 32 and np.mean(right[1, 3][:, hit] != wrong[1, 3][:, hit]) > 0.95
    assert np.any(right[1, 1] != wrong[1, 1]) or np.any(right[1, 2] != wrong[1, 2])
    # the wrapped rows ARE the first rows of beam 0, which the window at row 0 holds: that window is folded too
    low = fl.window(pat, fl.FIRST_BELOW)
    assert np.array_equal(fl.window(pat, fl.FIRST_AT_LINE, wrapped=True)[1, fl.WINDOW // 2:], low[0, :fl.WINDOW // 2])
    assert not np.array_equal(fl.expected_fold(pat, fl.FIRST_BELOW)[0], right)


def test_a_wrapped_store_would_show():
    """The second call's sub-integrations of beam 1 at and above LINE_SUB, stored 2^32 bytes low, land in sub-integrations 0 .. 3
    of beam 0, which hold the first call's profiles: the test reads them after the second call and expects them unchanged, and
    the two calls' profiles differ there."""
    first, second = fl.expected_short(91), fl.expected_short(93)
    half = fl.SHORT_SUBINTS // 2
    for s in range(fl.SHORT_SUBINTS):
        b, low = fl.wrapped_subint(1, fl.FIRST_SUB_AT_LINE + s)
        if s < half:
            assert (b, low) == (1, fl.FIRST_SUB_AT_LINE + s)
        else:
            assert (b, low) == (0, s - half) and fl.FIRST_SUB_BELOW <= low < fl.FIRST_SUB_BELOW + fl.SHORT_SUBINTS
            assert np.mean(second[1, s] != first[0, low]) > 0.01 and np.any(second[1, s] != 0)
    assert fl.wrapped_subint(0, fl.FIRST_SUB_AT_LINE) == (0, fl.FIRST_SUB_AT_LINE)
    # and where the store stayed 4 GiB low, the sub-integrations above the line would keep the prefill, which no folded word is
    pre = np.uint32(fl.PREFILL * 0x01010101)
    assert not np.any(second == pre) and not np.any(first == pre)
