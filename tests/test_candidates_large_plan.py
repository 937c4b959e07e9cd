"""The plan of tests/test_gpu_candidates_large.py, without a device: that d_snr passes 2^32 bytes and d_peaks 2^33, which
windows lie past the line, that what lies 4 GiB (or 8 GiB) below them is no window of the call -- so it holds the decoys
or the fill -- and, the CPU stand-in for "would fail if the kernel's offsets were 32-bit", that a list made from planes
read with wrapped offsets is another list."""
import numpy as np

from helpers import candidates_large as cl
from helpers import large_tensor as lt
from helpers.candidates_model import same_bits


PEAKS_PAST = [(1, 3)] + [(m, i) for m in (2, 3) for i in range(4)]  # the (DM, width) rows of d_peaks whose window lies past the line


def overlaps(a, b):
    return a[0] < b[1] and b[0] < a[1]


def test_sizes_and_the_line():
    assert cl.SNR_BYTES == 4_294_983_680 > lt.LINE and cl.SNR_BYTES < 1.01 * lt.LINE
    assert cl.PEAKS_BYTES == 8_589_967_360 > 2 * lt.LINE
    # no smaller peak_blocks of this shape passes the line with whole tiles of 64 blocks behind it
    assert cl.B * cl.NR_DM * cl.NR_WIDTHS * (cl.PEAK_BLOCKS - 256) * 4 == lt.LINE
    past = [(m, i) for m in range(cl.NR_DM) for i in range(cl.NR_WIDTHS) if cl.row_entry(m, i) * 4 >= lt.LINE]
    assert past == [(3, 3)] and (cl.row_entry(3, 2) + cl.NR_BLOCKS) * 4 < lt.LINE  # the rows on both sides of the line
    past = [(m, i) for m in range(cl.NR_DM) for i in range(cl.NR_WIDTHS) if cl.row_entry(m, i) * 8 >= lt.LINE]
    assert past == PEAKS_PAST and (cl.row_entry(3, 3) + cl.NR_BLOCKS) * 8 > 2 * lt.LINE
    assert cl.B * cl.NR_DM * cl.NR_BLOCKS < 1 << 32 and cl.FIRST_BLOCK + cl.NR_BLOCKS == cl.PEAK_BLOCKS < 1 << 32
    assert cl.FILL_FLOAT < 0 and np.isfinite(cl.FILL_FLOAT) and cl.FILL_FLOAT < cl.THRESHOLD < cl.SNR_DECOY


def test_what_lies_below_the_windows_is_no_window():
    planted = cl.planted_entries()
    assert len(planted) == 16 and all(b - a == cl.NR_BLOCKS for a, b in planted)
    # d_snr: the last row's window, 4 GiB low, is blocks 3968 .. 4095 of row (0, 0): no cells of the call
    decoy = (cl.decoy_entry(), cl.decoy_entry() + cl.NR_BLOCKS)
    assert decoy == (3968, 4096) and decoy[1] < cl.FIRST_BLOCK and not any(overlaps(decoy, w) for w in planted)
    assert (decoy[0] * 4 + lt.LINE) // 4 == cl.row_entry(3, 3)
    # d_peaks: every window past the line, 4 or 8 GiB low, lies between the windows
    for m, i in PEAKS_PAST:
        low = cl.wrapped_entry(cl.row_entry(m, i), 8)
        assert low != cl.row_entry(m, i) and not any(overlaps((low, low + cl.NR_BLOCKS), w) for w in planted), (m, i)


def test_a_wrapped_offset_gives_another_list():
    rec, count = cl.expected()
    assert 10 < count[0] == count[1] < cl.MAX_CANDIDATES
    at = {(int(r["dm"]), int(r["width_index"]), int(r["block"]) - cl.FIRST_BLOCK) for r in rec}
    assert {(3, 3, 40), (3, 2, 100), (0, 0, 70)} <= at  # past the line, before it, and in the row 4 GiB below
    assert len({int(r["dm"]) for r in rec}) == cl.NR_DM and rec["block"].min() >= cl.FIRST_BLOCK
    low_snr, low_snr_count = cl.expected(wrap_snr=True)
    assert low_snr_count[0] != count[0] and not any(r["snr"] == 30.0 for r in low_snr)
    assert any(r["snr"] == cl.SNR_DECOY and r["width_index"] == 3 for r in low_snr)
    low_peaks, low_peaks_count = cl.expected(wrap_peaks=True)
    assert low_peaks_count.tolist() == count.tolist() and not same_bits(low_peaks, rec)
    high = np.array([(int(r["dm"]), int(r["width_index"])) in PEAKS_PAST for r in rec])
    assert high.any() and np.all(low_peaks["value"][high] == cl.FILL_WORD) and not np.any(rec["value"][high] == cl.FILL_WORD)
    assert same_bits(low_peaks[~high], rec[~high])
