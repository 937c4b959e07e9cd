"""The plan of tests/test_gpu_rfi_large.py, without a device: that the filterbanks pass 2^32 bytes where the plan says, that the
pattern's period does not divide 2^32, and -- the CPU stand-in for "would fail if the kernels' offsets were 32-bit" -- that
every block, every zero-DM word and every cleaned row above the line comes out different from the rows 4 GiB lower, and that a
store 4 GiB low would land in rows that the test reads and expects untouched."""
import numpy as np

from helpers import large_tensor as lt
from helpers import rfi_large as rl


def test_sizes_line_and_period():
    assert rl.NBYTES == lt.LINE + 2 * 2048 * rl.C and rl.IN_SPECTRA * rl.C < lt.LINE
    assert rl.LINE_ROW == (1 << 25) - 2048 and (rl.IN_SPECTRA + rl.LINE_ROW) * rl.C == lt.LINE
    assert rl.FIRST_AT_LINE + rl.WINDOW == rl.IN_SPECTRA          # the window ends where the tensor ends
    assert rl.FIRST_AT_LINE + rl.WINDOW // 2 == rl.LINE_ROW       # half of it on either side of the line, in beam 1
    assert rl.LINE_ROW % rl.BLOCK_LEN == 0 and (rl.LINE_ROW - rl.FIRST_AT_LINE) // rl.BLOCK_LEN == rl.NR_BLOCKS // 2
    # with 2048 rows fewer per beam nothing of a window would lie above the line
    assert rl.B * (rl.IN_SPECTRA - 2048) * rl.C <= lt.LINE
    pat = rl.pattern(71)
    assert pat.dtype == np.uint8 and pat.shape[0] % 2 == 1 and lt.LINE % pat.nbytes != 0 and pat.nbytes <= lt.HOST_LIMIT
    assert np.unique(pat).size == 256
    # the rows 2^32 below the upper half of beam 1's window at the line are the first rows of beam 0: the other window reads them
    assert rl.FIRST_BELOW == 0 and rl.WINDOW // 2 <= rl.WINDOW


def test_a_wrapped_read_would_show():
    pat = rl.pattern(71)
    cell, mask, spec = rl.flags(72)
    cs, z, cleaned, replaced = rl.expected(pat, rl.FIRST_AT_LINE, cell, mask, spec)
    wcs, wz, wcleaned, _ = rl.expected(pat, rl.FIRST_AT_LINE, cell, mask, spec, wrapped=True)
    half = rl.NR_BLOCKS // 2
    # beam 0 and the blocks of beam 1 below the line read the same bytes either way
    assert np.array_equal(cs[0], wcs[0]) and np.array_equal(cs[1, :half], wcs[1, :half]) and np.array_equal(z[0], wz[0])
    # above the line every block's sums differ in most channels, every zero-DM word but a few, and every cleaned row
    differs = np.any(cs[1, half:] != wcs[1, half:], axis=-1)
    assert np.all(differs.mean(axis=1) > 0.9)
    assert np.mean(z[1, rl.WINDOW // 2:] != wz[1, rl.WINDOW // 2:]) > 0.95 and np.array_equal(z[1, :rl.WINDOW // 2], wz[1, :rl.WINDOW // 2])
    kept = spec[1, rl.WINDOW // 2:] == 0  # a flagged spectrum is the fill whatever was read
    assert kept.mean() > 0.9 and np.all(np.any(cleaned[1, rl.WINDOW // 2:] != wcleaned[1, rl.WINDOW // 2:], axis=1)[kept])
    # the wrapped rows ARE the first rows of beam 0, which the window at row 0 holds
    low = rl.window(pat, rl.FIRST_BELOW)
    assert np.array_equal(rl.window(pat, rl.FIRST_AT_LINE, wrapped=True)[1, rl.WINDOW // 2:], low[0, :rl.WINDOW // 2])
    assert 0.2 < replaced.min() / (rl.WINDOW * rl.C) and replaced.max() / (rl.WINDOW * rl.C) < 0.4


def test_a_wrapped_store_would_show():
    """A cleaned row of beam 1 stored 2^32 bytes low lands in rows 0 .. 4095 of beam 0, which lie outside the window that is
    cleaned: the test reads them back and expects the pattern, and the cleaned rows differ from the pattern there."""
    pat = rl.pattern(71)
    cell, mask, spec = rl.flags(72)
    _, _, cleaned, _ = rl.expected(pat, rl.FIRST_AT_LINE, cell, mask, spec)
    low = rl.window(pat, rl.FIRST_BELOW)[0, :rl.WINDOW // 2]
    assert rl.FIRST_BELOW + rl.WINDOW // 2 <= rl.FIRST_AT_LINE  # outside the cleaned window
    assert np.all(np.any(cleaned[1, rl.WINDOW // 2:] != low, axis=1))
    # and the cleaned rows are no copy: where the store stayed 4 GiB low, the rows above the line would keep the pattern
    assert np.all(np.any(cleaned[1, rl.WINDOW // 2:] != rl.window(pat, rl.FIRST_AT_LINE)[1, rl.WINDOW // 2:], axis=1))
