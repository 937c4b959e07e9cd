"""The plans of tests/test_gpu_correlator_large.py, without a device: that each tensor named as passing 2^32 bytes does, that
the sample pattern's period does not divide 2^32, and -- the CPU stand-in for "would fail if the kernel's offsets were
32-bit" -- that for every sampled row at or above the samples' line the bytes 4 GiB lower give other visibilities, and that a
store 4 GiB low leaves the prefill in a sampled row above the visibilities' line and lands in a sampled row below it."""
import numpy as np

from helpers import correlator_large as cl
from helpers import large_tensor as lt


def test_sizes_and_periods():
    blk, rin, rout, rows = cl.geometry(cl.SAMPLES)
    assert (blk, rin, rout, rows) == (2048, 264_192, 16_640, 16384)
    assert rows * rin == 4_328_521_728 > lt.LINE and rows * rout < lt.LINE  # the samples pass the line, their visibilities do not
    assert cl.SAMPLES["n"] % 4 == 1 and cl.SAMPLES["n"] <= 4095
    blk, rin, rout, rows = cl.geometry(cl.VIS)
    assert (blk, rin, rout, rows) == (8192, 8192, 263_168, 16336) and rows >= 16321
    assert rows * rout == 4_299_112_448 > lt.LINE and rows * rin == 133_824_512  # the visibilities pass the line
    for k, seed in ((cl.SAMPLES, 41), (cl.VIS, 42)):
        pat = cl.pattern(k, seed)
        assert pat.shape[0] % 2 == 1 and pat.shape[0] > 1 and lt.LINE % pat.nbytes != 0 and pat.nbytes <= lt.HOST_LIMIT
        assert int(pat.min()) == -128 and int(pat.max()) == 127
    # one wave per (channel, visibility, unit) item and the grid-stride loop: no launch comes near 2^31 workgroups
    assert cl.SAMPLES["C"] * 1 < 1 << 31 and 16336 * 10 < 1 << 31


def test_a_wrapped_sample_offset_would_show():
    k = cl.SAMPLES
    _, rin, _, rows = cl.geometry(k)
    pat = cl.pattern(k, 41)
    sample = cl.plan(k, 41)
    line_row = lt.LINE // rin
    assert line_row == 16256 and lt.LINE % rin != 0  # row 16256 straddles the line
    assert {0, 1, line_row - 1, line_row, line_row + 1, rows - 2, rows - 1} <= set(sample.tolist()) and sample.size <= 40
    seen = 0
    for r in sample:
        own, low = cl.expected_row(k, pat, int(r)), cl.expected_row(k, pat, int(r), wrapped=True)
        if r < line_row:
            assert low is None
            continue
        seen += 1
        assert low is not None and not np.array_equal(own, low)
        assert (own != low).mean() > 0.9  # nearly every word, not a chance few
        # and the rows that hold the bytes 4 GiB below are sampled too
        assert set(lt.alias_rows(rin, rows, int(r))) <= set(sample.tolist())
    assert seen >= 5


def test_a_wrapped_store_would_show():
    k = cl.VIS
    _, rin, rout, rows = cl.geometry(k)
    pat = cl.pattern(k, 42)
    sample = cl.plan(k, 42)
    line_row = lt.LINE // rout
    assert line_row == 16320 and lt.LINE % rout != 0
    above = [int(r) for r in sample if (r + 1) * rout > lt.LINE]
    assert {line_row, line_row + 1, rows - 2, rows - 1} <= set(above)
    prefill = np.full(cl.nr_baselines(k["A"]) * 2, 0xA5A5A5A5, dtype=np.uint32).view(np.int32).reshape(-1, 2)
    for r in above:
        own = cl.expected_row(k, pat, r)
        # a store 4 GiB low leaves the prefill here, which is not the row's visibilities ...
        assert not np.any(own == prefill)
        # ... and lands in rows that the test reads and that hold other values
        alias = lt.alias_rows(rout, rows, r)
        assert alias and set(alias) <= set(sample.tolist())
        for q in alias:
            assert not np.array_equal(cl.expected_row(k, pat, q), own)
