"""The shapes of tests/test_gpu_correlator_large.py, and what the host can say about tensors that exist on the device only
(helpers/large_tensor.py).  tests/test_correlator_large_plan.py walks the same plans without a device and shows that a byte
offset worked out in 32 bits cannot pass them.

A row is one (channel, visibility): n blocks of [A][16][2] samples in, NB (re, im) pairs out.  The device tensor of samples
repeats a pattern of (channel, block) rows with an odd period, so the host can produce the samples of any row."""
import numpy as np

from helpers import large_tensor as lt
from helpers.correlator_model import nr_baselines, visibilities

# the samples past 2^32 bytes: 16384 channels of one visibility of 129 blocks (32 K groups of four and one block) of 64 antennas
SAMPLES = dict(A=64, C=16384, nblk=129, n=129)
# the visibilities past 2^32 bytes: 256 antennas, a visibility per block; C * nr_vis = 16336 >= 16321 rows of 263168 bytes
VIS = dict(A=256, C=16, nblk=1021, n=1)
RANDOM_ROWS = 8
PREFILL = 0xA5


def geometry(k):
    """(bytes of a (channel, block) of samples, row_bytes_in, row_bytes_out, rows)."""
    blk = k["A"] * 32
    return blk, k["n"] * blk, nr_baselines(k["A"]) * 8, k["C"] * (k["nblk"] // k["n"])


def pattern(k, seed):
    """int8 [odd period][A * 32]: full-range (channel, block) rows."""
    return lt.int8_pattern(k["A"] * 32, seed)


def plan(k, seed):
    """The sorted sample of rows: the first and last two; for every multiple of 2^32 inside either tensor the row that holds
    the line, its neighbours and the row half way to the end; a few seeded rows; and for every one of these the rows 2^32 bytes below it in either tensor."""
    _, rin, rout, rows = geometry(k)
    base = {0, 1, rows - 2, rows - 1} | {int(r) for r in np.random.default_rng(seed).integers(0, rows, size=RANDOM_ROWS)}
    for rb in (rin, rout):
        for line in lt.lines_of(rb, rows):
            r = line // rb
            base |= {r - 1, r, min(r + 1, rows - 1), (r + rows) // 2}  # and one half way between the line and the end
    sample = set(base)
    for rb in (rin, rout):
        for r in base:
            sample |= set(lt.alias_rows(rb, rows, r))
    return np.array(sorted(sample), dtype=np.int64)


def samples_of_row(k, pat, r, wrapped=False):
    """int8 [1][n][A][16][2]: the samples of row r of a device tensor filled with ``pat``; ``wrapped``: as a kernel would read
    them whose byte offsets at or above 2^32 came out 2^32 lower (None where the row lies below the line altogether)."""
    blk, rin, _, _ = geometry(k)
    if wrapped:
        raw = lt.row_as_wrapped(pat, rin, r)
        if raw is None:
            return None
    else:
        raw = lt.rows_of(pat, r * k["n"] + np.arange(k["n"], dtype=np.int64)).reshape(-1)
    return raw.view(np.int8).reshape(1, k["n"], k["A"], 16, 2)


def expected_row(k, pat, r, wrapped=False):
    """int32 [NB][2] of row r, or None."""
    s = samples_of_row(k, pat, r, wrapped)
    return None if s is None else visibilities(s, k["n"])[0, 0]
