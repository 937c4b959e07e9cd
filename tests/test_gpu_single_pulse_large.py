"""The single-pulse search held to its 64-bit offsets (include/dcs_single_pulse.h): a plane, a peak plane and a
signal-to-noise tensor past 2^32 bytes, which never exist on the host (helpers/large_tensor.py, helpers/single_pulse_large.py).
A byte offset worked out in 32 bits wraps inside the same allocation, 4 GiB lower: nothing faults and no canary is touched,
so the plane holds a pattern in which the words 4 GiB apart differ, and the outputs are prefilled so that a wrapped store
shows both above the line (the prefill stays) and below it (the prefill is spoiled).  Every other test of the search passes
with 32-bit offsets; these do not (tests/test_single_pulse_large_plan.py shows it without a device)."""
import numpy as np
import pytest

from helpers import large_tensor as lt
from helpers import single_pulse_large as sl
from helpers.device_buffers import Context
from helpers.single_pulse_model import nr_blocks_of, peaks, snr, sums

pytestmark = pytest.mark.gpu

PREFILL = 0xA5
PREFILL_WORD = 0xA5A5A5A5


@pytest.fixture
def case(gpu):
    c = Context(gpu, 64)
    yield c
    c.close()


def test_plane_past_the_line(gpu, case):
    """nr_dm = 4, plane_spectra = 2^28 + 4096: 4,295,032,832 bytes, and word 2^28 - 12288 of DM 3 begins on the line.  The sums
    and the peaks of 5000 times from windows that end below the line, straddle it and begin above it, all four series at once."""
    from dc_sand_amd.generator import boxcar_peaks_bytes, dm_time_bytes, dm_time_sums_bytes

    g, alloc, upload = case.g, case.alloc, case.upload
    k = sl.PLANE
    B, nr_dm, ps, T, max_width, block_len = k["B"], k["nr_dm"], k["plane_spectra"], k["T"], k["max_width"], k["block_len"]
    widths = np.array(k["widths"], np.uint32)
    nbytes = dm_time_bytes(B, nr_dm, ps)
    assert nbytes == sl.PLANE_BYTES and lt.LINE < nbytes < 1.01 * lt.LINE and sl.LINE_WORD == (1 << 28) - 12288
    pattern = sl.plane_pattern()
    d_plane = alloc(nbytes)
    lt.fill(gpu, d_plane, nbytes, pattern)
    d_widths = upload(widths)
    nb = nr_blocks_of(T, block_len)
    sbytes, kbytes = dm_time_sums_bytes(B, nr_dm), boxcar_peaks_bytes(B, nr_dm, widths.size, nb)
    d_sums, d_peaks = case.out(sbytes), case.out(kbytes)
    for first in sl.plane_firsts():
        assert 0 <= first and first + sl.PLANE_WINDOW <= ps
        case.refill(d_sums)
        case.refill(d_peaks)
        g.dm_time_sums(d_plane, nbytes, ps, first, T, B, nr_dm, d_sums, sbytes)
        g.boxcar_peaks(d_plane, nbytes, ps, first, T, B, nr_dm, d_widths, widths.size, max_width, block_len, d_peaks, kbytes, nb)
        gpu.synchronize()
        window = sl.plane_window(pattern, first)  # [1][4][T + max_width - 1] from the pattern
        exp_sums, exp_peaks = sums(window, 0, T), peaks(window, 0, T, widths, max_width, block_len)
        assert np.unique(exp_peaks[..., 1]).size >= 50 and not np.array_equal(exp_peaks[0, 0], exp_peaks[0, 3])
        got_sums = case.read(d_sums, sbytes, np.uint64, exp_sums.shape)
        assert np.array_equal(got_sums, exp_sums), (first, got_sums, exp_sums)
        got = case.read(d_peaks, kbytes, np.uint32, exp_peaks.shape)
        assert np.array_equal(got, exp_peaks), (first, np.argwhere(got != exp_peaks)[:3])
    # what the device holds is the pattern: the words on both sides of the line, read back
    rows = np.array([0, 1, lt.LINE // 4096 - 1, lt.LINE // 4096, nbytes // 4096 - 1], dtype=np.int64)
    assert np.array_equal(lt.read_rows(gpu, d_plane, 4096, rows), lt.rows_of(pattern, rows))


def test_peak_plane_past_the_line(gpu, case):
    """nr_dm = 4, four widths, peak_blocks = 2^25 + 512: 4,295,032,832 bytes of peaks.  16 blocks at the end of every (DM,
    width) row: those of the last row lie past the line, and the entries 4 GiB below them keep the prefill."""
    from dc_sand_amd.generator import boxcar_peaks_bytes

    g, upload = case.g, case.upload
    k = sl.PEAKS_OUT
    B, nr_dm, pb, T, block_len, max_width = k["B"], k["nr_dm"], k["peak_blocks"], k["T"], k["block_len"], k["max_width"]
    widths = np.array(sl.WIDTHS_OUT, np.uint32)
    kbytes = boxcar_peaks_bytes(B, nr_dm, widths.size, pb)
    row_bytes, per, written, alias = sl.out_rows(pb, 8)
    assert lt.LINE < kbytes < 1.01 * lt.LINE and written[-1] * row_bytes > lt.LINE and alias.size == 1
    plane = np.random.default_rng(32).integers(0, 1 << 20, size=(B, nr_dm, 3 + T + max_width - 1), dtype=np.uint32)
    d_plane, d_widths = upload(plane), upload(widths)
    d_peaks = case.out(kbytes)
    g.boxcar_peaks(d_plane, plane.nbytes, plane.shape[2], 3, T, B, nr_dm, d_widths, widths.size, max_width, block_len, d_peaks, kbytes,
                   pb, first_block=pb - sl.ROW_BLOCKS)
    gpu.synchronize()
    exp = peaks(plane, 3, T, widths, max_width, block_len).reshape(-1, sl.ROW_BLOCKS * 2)  # [16 rows][16 blocks x {value, time}]
    got = lt.read_rows(gpu, d_peaks, row_bytes, written).view(np.uint32)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:3]
    untouched = np.array(sorted({0, 1, *alias.tolist(), int(alias[0]) - 1, int(alias[0]) + 1, *(int(w) - 1 for w in written)}), dtype=np.int64)
    assert not set(untouched.tolist()) & set(written.tolist())
    kept = lt.read_rows(gpu, d_peaks, row_bytes, untouched).view(np.uint32)
    assert np.all(kept == PREFILL_WORD), "a block outside [first_block, first_block + nr_blocks) was written"
    case.guard_untouched(d_peaks)


def test_signal_to_noise_past_the_line_from_peaks_past_two(gpu, case):
    """peak_blocks = 2^26 + 256: 4,294,983,680 bytes of signal-to-noise read from 8,589,967,360 bytes of peaks, over the last 16
    blocks of every (DM, width) row.  The peaks elsewhere hold the prefill, so an entry read 4 or 8 GiB low gives other figures."""
    from dc_sand_amd.generator import best_width_bytes, boxcar_peaks_bytes, peak_snr_bytes

    g, alloc, upload = case.g, case.alloc, case.upload
    k = sl.SNR_OUT
    B, nr_dm, pb, count, max_width = k["B"], k["nr_dm"], k["peak_blocks"], k["count"], k["max_width"]
    widths = np.array(sl.WIDTHS_OUT, np.uint32)
    nw, nblk = widths.size, sl.ROW_BLOCKS
    kbytes, nbytes, bbytes = boxcar_peaks_bytes(B, nr_dm, nw, pb), peak_snr_bytes(B, nr_dm, nw, pb), best_width_bytes(B, nr_dm, pb)
    assert 2 * lt.LINE < kbytes < 2.01 * lt.LINE and lt.LINE < nbytes < 1.01 * lt.LINE
    prow, _, pwritten, palias = sl.out_rows(pb, 8)
    srow, _, swritten, salias = sl.out_rows(pb, 4)
    assert not set(palias.tolist()) & set(pwritten.tolist()) and palias.size >= 2 and salias.size == 1
    plane = np.random.default_rng(33).integers(0, 1 << 20, size=(B, nr_dm, nblk * 64 + max_width - 1), dtype=np.uint32)
    pk = peaks(plane, 0, nblk * 64, widths, max_width, 64)  # [1][4][4][16][2]
    sm = sums(plane, 0, count)
    d_peaks, d_snr, d_best = alloc(kbytes), case.out(nbytes), case.out(bbytes)
    gpu.memset(d_peaks, PREFILL, kbytes)
    for row, values in zip(pwritten, pk.reshape(-1, nblk * 2)):
        gpu.memcpy_htod(int(d_peaks) + int(row) * prow, np.ascontiguousarray(values))
    d_widths, d_sums = upload(widths), upload(sm)
    g.peak_snr(d_peaks, kbytes, pb, pb - nblk, nblk, B, nr_dm, d_widths, nw, max_width, d_sums, sm.nbytes, count, d_snr, nbytes,
               d_best, bbytes)
    gpu.synchronize()
    exp, exp_best = snr(pk, widths, max_width, sm, count)
    assert np.isfinite(exp[:, :, :3]).all() and np.unique(exp).size > 100
    got = lt.read_rows(gpu, d_snr, srow, swritten).view(np.uint32)
    assert np.array_equal(got, exp.reshape(-1, nblk).view(np.uint32)), np.argwhere(got != exp.reshape(-1, nblk).view(np.uint32))[:3]
    untouched = np.array(sorted({0, 1, *salias.tolist(), int(salias[0]) - 1, *(int(w) - 1 for w in swritten)}), dtype=np.int64)
    assert not set(untouched.tolist()) & set(swritten.tolist())
    assert np.all(lt.read_rows(gpu, d_snr, srow, untouched).view(np.uint32) == PREFILL_WORD), "a block outside the call's was written"
    # the best widths: the last 16 words of every DM's row, and the words before them
    brow = nblk * 4
    per = pb * 4 // brow
    bwritten = np.array([(m + 1) * per - 1 for m in range(nr_dm)], dtype=np.int64)
    assert np.array_equal(lt.read_rows(gpu, d_best, brow, bwritten).view(np.uint32), exp_best.reshape(nr_dm, nblk))
    assert np.all(lt.read_rows(gpu, d_best, brow, bwritten - 1).view(np.uint32) == PREFILL_WORD)
    case.guard_untouched(d_snr)
    case.guard_untouched(d_best)
