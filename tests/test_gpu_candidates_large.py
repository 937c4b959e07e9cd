"""The candidate sifter held to its 64-bit offsets (include/dcs_candidates.h): a signal-to-noise plane past 2^32 bytes and
the peaks behind it past 2^33, which never exist on the host (helpers/candidates_large.py).  An offset worked out in 32
bits wraps inside the same allocation: nothing faults and no canary is touched, so the planes hold a byte fill below the
threshold with the call's windows copied in, and decoys above the threshold where the window past the line would be read
4 GiB low.  Every other test of the sifter passes with 32-bit offsets; this one does not
(tests/test_candidates_large_plan.py shows it without a device)."""
import numpy as np
import pytest

from helpers import candidates_large as cl
from helpers.candidates_model import CANDIDATE, expected_buffer, same_bits
from helpers.device_buffers import Context

pytestmark = pytest.mark.gpu

PREFILL = 0x3C


def test_planes_past_the_line(gpu):
    from dc_sand_amd.generator import boxcar_peaks_bytes, candidates_bytes, candidates_workspace_bytes, peak_snr_bytes

    sbytes = peak_snr_bytes(cl.B, cl.NR_DM, cl.NR_WIDTHS, cl.PEAK_BLOCKS)
    kbytes = boxcar_peaks_bytes(cl.B, cl.NR_DM, cl.NR_WIDTHS, cl.PEAK_BLOCKS)
    cbytes, wbytes = candidates_bytes(cl.MAX_CANDIDATES), candidates_workspace_bytes(cl.B, cl.NR_DM, cl.NR_BLOCKS)
    assert (sbytes, kbytes) == (cl.SNR_BYTES, cl.PEAKS_BYTES)
    c = Context(gpu, 64)
    try:
        d_snr, d_peaks = c.alloc(sbytes), c.alloc(kbytes)
        d_cands, d_count, d_work = (c.out(n, PREFILL) for n in (cbytes, 8, wbytes))
        gpu.memset(d_snr, cl.FILL, sbytes)
        gpu.memset(d_peaks, cl.FILL, kbytes)
        snr, peaks = cl.window_planes()
        for m in range(cl.NR_DM):
            for i in range(cl.NR_WIDTHS):
                gpu.memcpy_htod(int(d_snr) + cl.row_entry(m, i) * 4, np.ascontiguousarray(snr[0, m, i]))
                gpu.memcpy_htod(int(d_peaks) + cl.row_entry(m, i) * 8, np.ascontiguousarray(peaks[0, m, i]))
        gpu.memcpy_htod(int(d_snr) + cl.decoy_entry() * 4, np.full(cl.NR_BLOCKS, cl.SNR_DECOY, np.float32))
        c.g.find_candidates(d_snr, sbytes, d_peaks, kbytes, cl.PEAK_BLOCKS, cl.FIRST_BLOCK, cl.NR_BLOCKS, cl.B, cl.NR_DM, cl.NR_WIDTHS,
                            cl.THRESHOLD, *cl.RADII, d_cands, cbytes, cl.MAX_CANDIDATES, d_count, d_work, wbytes)
        gpu.synchronize()
        rec, count = cl.expected()
        got = c.read(d_cands, cbytes)
        assert c.read(d_count, 8, np.uint32).tolist() == count.tolist()
        prefill = np.zeros(cl.MAX_CANDIDATES, CANDIDATE)
        prefill.view(np.uint8)[:] = PREFILL
        exp = expected_buffer(rec, count, prefill)
        bad = np.flatnonzero((got[:cbytes].view(np.uint32) != exp.view(np.uint32)).reshape(-1, 8).any(axis=1))
        assert bad.size == 0, (len(bad), got[:cbytes].view(CANDIDATE)[bad[0]], exp[bad[0]])
        assert same_bits(got[:cbytes].view(CANDIDATE), exp)
        # the planes are as they were made: the decoys and a window on each side of the line, read back
        back = np.empty(cl.NR_BLOCKS, np.float32)
        for entry, want in ((cl.decoy_entry(), np.full(cl.NR_BLOCKS, cl.SNR_DECOY, np.float32)), (cl.row_entry(3, 3), snr[0, 3, 3]),
                            (cl.row_entry(3, 2), snr[0, 3, 2])):
            gpu.memcpy_dtoh(back, int(d_snr) + entry * 4)
            assert np.array_equal(back.view(np.uint32), want.view(np.uint32))
    finally:
        c.close()
