"""The RFI flagger held to its 64-bit offsets (include/dcs_rfi.h): filterbanks past 2^32 bytes, which never exist on the host
(helpers/large_tensor.py: the filling, the pattern whose period does not divide 2^32, the row reads; helpers/rfi_large.py: the
shape).  A byte offset worked out in 32 bits wraps inside the same allocation, 4 GiB lower: nothing faults and no canary is
touched, so the filterbanks hold a pattern in which the rows 4 GiB apart differ.  Every other test of the flagger passes with
32-bit offsets; this one does not (tests/test_rfi_large_plan.py)."""
import numpy as np
import pytest

from helpers import large_tensor as lt
from helpers import rfi_large as rl
from helpers.device_buffers import Context

pytestmark = pytest.mark.gpu


@pytest.fixture
def case(gpu):
    c = Context(gpu, rl.C)
    yield c
    c.close()


def test_moments_and_clean_on_both_sides_of_the_line(gpu, case):
    from dc_sand_amd.generator import rfi_cell_sums_bytes, rfi_zero_dm_bytes

    g = case.g
    pat = rl.pattern(71)
    d_fb = case.out(rl.NBYTES)
    lt.fill(gpu, d_fb, rl.NBYTES, pat)
    sbytes, zbytes = rfi_cell_sums_bytes(case.bp, rl.B, rl.NR_BLOCKS), rfi_zero_dm_bytes(rl.B, rl.WINDOW)
    d_cs, d_z = case.out(sbytes), case.out(zbytes)
    # the statistics of the window at the line, and of the window that holds the rows 4 GiB below its upper half
    for first in (rl.FIRST_AT_LINE, rl.FIRST_BELOW):
        case.refill(d_cs)
        case.refill(d_z)
        g.rfi_moments(d_fb, rl.NBYTES, rl.IN_SPECTRA, first, rl.NR_BLOCKS, rl.BLOCK_LEN, rl.B, d_cs, sbytes, d_z, zbytes)
        gpu.synchronize()
        cs, z, _, _ = rl.expected(pat, first)
        got_cs = case.read(d_cs, sbytes, np.uint32, cs.shape)
        got_z = case.read(d_z, zbytes, np.uint32, z.shape)
        assert np.array_equal(got_cs, cs), (first, np.argwhere(got_cs != cs)[:3])
        assert np.array_equal(got_z, z), (first, np.argwhere(got_z != z)[:3])
    # cleaned in place at the line
    cell, mask, spec = rl.flags(72)
    d_cell, d_mask, d_spec, d_rep = case.upload(cell), case.upload(mask), case.upload(spec), case.out(rl.B * 8, 0)
    g.rfi_clean_q8(d_fb, rl.NBYTES, rl.IN_SPECTRA, rl.FIRST_AT_LINE, rl.NR_BLOCKS, rl.BLOCK_LEN, rl.B, rl.FILL, d_fb, rl.NBYTES,
                   rl.IN_SPECTRA, first_out=rl.FIRST_AT_LINE, d_cell_flags=d_cell, d_channel_mask=d_mask, d_spectrum_flags=d_spec,
                   d_replaced=d_rep)
    gpu.synchronize()
    _, _, cleaned, replaced = rl.expected(pat, rl.FIRST_AT_LINE, cell, mask, spec)
    rows = rl.FIRST_AT_LINE + np.arange(rl.WINDOW, dtype=np.int64)
    for b in range(rl.B):  # the whole window of either beam: beam 1's straddles the line
        got = lt.read_rows(gpu, d_fb, rl.C, b * rl.IN_SPECTRA + rows)
        assert np.array_equal(got, cleaned[b]), (b, np.argwhere(got != cleaned[b])[:3])
    assert np.array_equal(case.read(d_rep, rl.B * 8, np.uint64, (rl.B,)), replaced)
    # untouched: the rows 4 GiB below the cleaned rows of beam 1, the rows in front of either window, the first of beam 1
    below = np.arange(rl.WINDOW // 2 + 2, dtype=np.int64)
    before = np.arange(rl.FIRST_AT_LINE - 2, rl.FIRST_AT_LINE, dtype=np.int64)
    untouched = np.concatenate([below, before, rl.IN_SPECTRA + np.arange(2), rl.IN_SPECTRA + before])
    assert np.array_equal(lt.read_rows(gpu, d_fb, rl.C, untouched), lt.rows_of(pat, untouched))
    case.guard_untouched(d_fb)
