"""The plans of tests/test_gpu_single_pulse_large.py, without a device: that each tensor named as passing 2^32 (or 2^33)
bytes does, that the plane pattern's period does not divide 2^32, and -- the CPU stand-in for "would fail if the kernel's
offsets were 32-bit" -- that for every window at or above the line the words 4 GiB lower differ from the window's own, and
with them the sums and the peaks; that a store 4 GiB low lands on rows the tests read as untouched; and that a peak read 4
or 8 GiB low gives another signal-to-noise."""
import numpy as np

from helpers import large_tensor as lt
from helpers import single_pulse_large as sl
from helpers.single_pulse_model import peaks, snr, sums


def test_sizes_and_period():
    k = sl.PLANE
    assert sl.PLANE_BYTES == 4_295_032_832 > lt.LINE and sl.PLANE_BYTES % lt.LINE < 0.01 * lt.LINE
    assert 3 * k["plane_spectra"] * 4 < lt.LINE  # the line falls into the last series
    assert 0 < sl.LINE_WORD < k["plane_spectra"] and (3 * k["plane_spectra"] + sl.LINE_WORD) * 4 == lt.LINE
    pattern = sl.plane_pattern()
    assert pattern.dtype == np.uint32 and pattern.shape[0] % 2 == 1 and lt.LINE % pattern.nbytes != 0 and pattern.nbytes <= lt.HOST_LIMIT
    assert int(pattern.max()) > 0xFFF00000 and int(pattern.min()) < 0x000FFFFF  # full-range words: every sum wraps
    p, s = sl.PEAKS_OUT, sl.SNR_OUT
    nw = len(sl.WIDTHS_OUT)
    assert p["nr_dm"] * nw * p["peak_blocks"] * 8 == 4_295_032_832
    assert s["nr_dm"] * nw * s["peak_blocks"] * 4 == 4_294_983_680 > lt.LINE
    assert s["nr_dm"] * nw * s["peak_blocks"] * 8 == 8_589_967_360 > 2 * lt.LINE
    # grids beyond 2^31 workgroups are refused by the launchers: no case comes near
    assert s["nr_dm"] * sl.ROW_BLOCKS < 1 << 20


def test_a_wrapped_plane_offset_would_show():
    k = sl.PLANE
    pattern = sl.plane_pattern()
    widths = np.array(k["widths"], np.uint32)
    firsts = sl.plane_firsts()
    assert firsts[0] + sl.PLANE_WINDOW == sl.LINE_WORD and firsts[-1] + sl.PLANE_WINDOW == k["plane_spectra"]
    assert firsts[1] < sl.LINE_WORD < firsts[1] + k["T"] and firsts[3] == sl.LINE_WORD
    seen = 0
    for first in firsts:
        own, low = sl.plane_window(pattern, first), sl.plane_window(pattern, first, wrapped=True)
        assert np.array_equal(own[0, :3], low[0, :3])  # the first three series lie below the line
        if first + sl.PLANE_WINDOW <= sl.LINE_WORD:
            assert np.array_equal(own, low)
            continue
        seen += 1
        assert not np.array_equal(own[0, 3], low[0, 3])
        assert not np.array_equal(sums(own, 0, k["T"])[0, 3], sums(low, 0, k["T"])[0, 3])
        a, b = (peaks(w, 0, k["T"], widths, k["max_width"], k["block_len"])[0, 3] for w in (own, low))
        differ = np.any(a != b, axis=(0, 2))  # per block
        assert differ.any() and (first < sl.LINE_WORD or differ.all()), first
    assert seen == 5


def test_a_wrapped_store_or_peak_read_would_show():
    nw = len(sl.WIDTHS_OUT)
    # peaks past the line: one written row lies past it, and the row 4 GiB below is one the test reads as untouched
    row_bytes, per, written, alias = sl.out_rows(sl.PEAKS_OUT["peak_blocks"], 8)
    assert row_bytes == 128 and written.size == 4 * nw and np.all(np.diff(written) == per)
    assert (written * row_bytes >= lt.LINE).sum() == 1 and alias.tolist() == [int(written[-1]) - lt.LINE // row_bytes] == [511]
    assert not set(alias.tolist()) & set(written.tolist()) and alias[0] % per < per - 1
    # signal-to-noise past the line, peaks past two: the same for the stores, and the peak rows read 4 or 8 GiB low are rows
    # that hold the prefill, whose figures are not those of the peaks
    srow, sper, swritten, salias = sl.out_rows(sl.SNR_OUT["peak_blocks"], 4)
    assert (swritten * srow >= lt.LINE).sum() == 1 and salias.tolist() == [255] and not set(salias.tolist()) & set(swritten.tolist())
    prow, pper, pwritten, palias = sl.out_rows(sl.SNR_OUT["peak_blocks"], 8)
    assert (pwritten * prow >= lt.LINE).sum() == 9 and (pwritten * prow >= 2 * lt.LINE).sum() == 1
    assert palias.size == 10 and not set(palias.tolist()) & set(pwritten.tolist())
    widths = np.array(sl.WIDTHS_OUT, np.uint32)
    plane = np.random.default_rng(33).integers(0, 1 << 20, size=(1, 4, sl.ROW_BLOCKS * 64 + 63), dtype=np.uint32)
    pk, sm = peaks(plane, 0, sl.ROW_BLOCKS * 64, widths, 64, 64), sums(plane, 0, sl.SNR_OUT["count"])
    own, _ = snr(pk, widths, 64, sm, sl.SNR_OUT["count"])
    low, _ = snr(np.full_like(pk, 0xA5A5A5A5), widths, 64, sm, sl.SNR_OUT["count"])
    assert not np.any(own[:, :, :3].view(np.uint32) == low[:, :, :3].view(np.uint32))
