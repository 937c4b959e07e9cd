"""The shape of tests/test_gpu_rfi_large.py and what the host can say about filterbanks that exist on the device only
(helpers/large_tensor.py).  tests/test_rfi_large_plan.py walks the same plan without a device and shows that a byte offset
worked out in 32 bits cannot pass it.

B = 2, C = 64, in_spectra = 2^25 + 2048: 2^32 + 262144 bytes, the smallest two-beam filterbank of 64 channels that has half a
window of 32 blocks of 256 spectra above the line.  Beam 1's row LINE_ROW = 2^25 - 2048 begins on the line, and its last 4096
rows lie above it; the bytes 2^32 below row r >= LINE_ROW of beam 1 are row r - LINE_ROW of beam 0.  The window at the line
is rows [LINE_ROW - 4096, in_spectra) of every beam: it ends where the tensor ends.  The window at row 0 holds, in beam 0,
the rows 2^32 below the upper half of the other.  The device bytes repeat a pattern whose period is an odd number of rows, so
it does not divide 2^32 and rows 2^32 apart differ."""
import numpy as np

from helpers import large_tensor as lt
from helpers import rfi_model as rm

B, C = 2, 64
IN_SPECTRA = (1 << 25) + 2048
NBYTES = B * IN_SPECTRA * C
LINE_ROW = (lt.LINE - IN_SPECTRA * C) // C  # of beam 1
BLOCK_LEN, NR_BLOCKS = 256, 32
WINDOW = BLOCK_LEN * NR_BLOCKS
FIRST_AT_LINE = LINE_ROW - WINDOW // 2
FIRST_BELOW = 0
FILL = 128


def pattern(seed):
    """uint8 [period][C], every byte value."""
    return lt.int8_pattern(C, seed).view(np.uint8)


def window(pat, first, wrapped=False):
    """uint8 [B][WINDOW][C]: rows first .. first + WINDOW - 1 of every beam; ``wrapped``: as a kernel would read them whose
    byte offsets came out modulo 2^32."""
    rows = first + np.arange(WINDOW, dtype=np.int64)
    out = []
    for b in range(B):
        g = b * IN_SPECTRA + rows
        if wrapped:
            g = np.where(g * C >= lt.LINE, g - lt.LINE // C, g)
        out.append(lt.rows_of(pat, g))
    return np.stack(out)


def flags(seed):
    """(cell flags [B][NR_BLOCKS][C], channel masks [B][C], spectrum flags [B][WINDOW]) with about three tenths of the bytes replaced."""
    rng = np.random.default_rng(seed)
    cell = rng.choice(np.array([0] * 15 + [1, 2, 3], np.uint8), size=(B, NR_BLOCKS, C))
    mask = rng.choice(np.array([1] * 15 + [0], np.uint8), size=(B, C))
    spec = rng.choice(np.array([0] * 15 + [1], np.uint8), size=(B, WINDOW))
    return cell, mask, spec


def expected(pat, first, cell=None, mask=None, spec=None, wrapped=False):
    """(cell sums, zero-DM series, cleaned window uint8 [B][WINDOW][C], bytes replaced) of the window at ``first``."""
    fb = window(pat, first, wrapped)
    cs, z = rm.moments(fb, 0, NR_BLOCKS, BLOCK_LEN)
    cleaned, replaced = rm.clean(fb, 0, NR_BLOCKS, BLOCK_LEN, FILL, cell, mask, spec)
    return cs, z, cleaned, replaced
