"""The correlator held to its 64-bit offsets (include/dcs_correlator.h): a sample tensor and a visibility tensor past 2^32
bytes, which never exist on the host (helpers/large_tensor.py, helpers/correlator_large.py).  A byte offset worked out in 32
bits wraps inside the same allocation, 4 GiB lower: nothing faults and no canary is touched, so the samples hold a pattern in
which the bytes 4 GiB apart differ, and the visibilities are prefilled so that a wrapped store shows both above the line (the
prefill stays) and below it (another row's words).  Every other test of the correlator passes with 32-bit offsets; these do
not (tests/test_correlator_large_plan.py shows it without a device)."""
import numpy as np
import pytest

from helpers import correlator_large as cl
from helpers import large_tensor as lt
from helpers.device_buffers import Context

pytestmark = pytest.mark.gpu


def run_case(gpu, k, seed):
    from dc_sand_amd.generator import block_visibilities_bytes

    A, C, nblk, n = k["A"], k["C"], k["nblk"], k["n"]
    _, rin, rout, rows = cl.geometry(k)
    c = Context(gpu, C, A, NR_SAMPLES_PER_CHANNEL=16 * nblk)
    abytes, vbytes = rows * rin, block_visibilities_bytes(c.bp, 16 * nblk, n)
    assert abytes == A * C * nblk * 32 and vbytes == rows * rout
    pat = cl.pattern(k, seed)
    try:
        d_ant, d_vis = c.alloc(abytes), c.out(vbytes, cl.PREFILL, cl.PREFILL)
        lt.fill(gpu, d_ant, abytes, pat)
        c.g.correlate_block(d_ant, abytes, d_vis, vbytes, 16 * nblk, n)
        gpu.synchronize()
        sample = cl.plan(k, seed)
        got = lt.read_rows(gpu, d_vis, rout, sample).view(np.int32).reshape(sample.size, -1, 2)
        for i, r in enumerate(sample):
            exp = cl.expected_row(k, pat, int(r))
            assert np.array_equal(got[i], exp), (int(r), np.argwhere(got[i] != exp)[:3])
        c.guard_untouched(d_vis)
        # what the device holds is the pattern: the sample rows on both sides of the lines, read back
        blk = A * 32
        block_rows = np.array(sorted({0, 1, abytes // blk - 1, *(x // blk + d for x in lt.lines_of(blk, abytes // blk) for d in (-1, 0))}),
                              dtype=np.int64)
        assert np.array_equal(lt.read_rows(gpu, d_ant, blk, block_rows), lt.rows_of(pat, block_rows))
    finally:
        c.close()
    return abytes, vbytes


def test_samples_past_the_line(gpu):
    """A = 64, 16384 channels of one visibility of 129 blocks: 4,328,521,728 bytes of samples; channel 16256 straddles the line."""
    abytes, vbytes = run_case(gpu, cl.SAMPLES, 41)
    assert abytes > lt.LINE > vbytes


def test_visibilities_past_the_line(gpu):
    """A = 256, n = 1, 16 channels of 1021 blocks: 16336 rows of 263,168 bytes, 4,299,112,448 bytes of visibilities from 134 MB of
    samples; row 16320 straddles the line."""
    abytes, vbytes = run_case(gpu, cl.VIS, 42)
    assert vbytes > lt.LINE > abytes
