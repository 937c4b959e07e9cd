"""The shapes of tests/test_gpu_fold_large.py and what the host can say about tensors that exist on the device only
(helpers/large_tensor.py).  tests/test_fold_large_plan.py walks the same plan without a device and shows that a byte offset
worked out in 32 bits cannot pass it.

Filterbank past 4 GiB.  B = 2, C = 64, in_spectra = 2^25 + 2048: 2^32 + 262144 bytes, the shape of helpers/rfi_large.py.  Beam
1's row LINE_ROW = 2^25 - 2048 begins on the line; the bytes 2^32 below row r >= LINE_ROW of beam 1 are row r - LINE_ROW of beam
0.  The window at the line is rows [LINE_ROW - 4096, in_spectra) of every beam -- 4 sub-integrations of 2032 spectra and 64 rows
of delay -- and ends where the tensor ends; the window at row 0 holds, in beam 0, the rows 2^32 below the upper half of the other.
The device bytes repeat a pattern whose period is an odd number of rows, so rows 2^32 apart differ.

Profiles past 4 GiB.  uint32 [2][OUT_SUBINTS][64][1024] with OUT_SUBINTS = 2^13 + 16: a sub-integration of a beam is 2^18 bytes,
the tensor 2^32 + 2^23.  Beam 1's sub-integration LINE_SUB = 2^13 - 16 begins on the line; the bytes 2^32 below sub-integration
s >= LINE_SUB of beam 1 are sub-integration s - LINE_SUB of beam 0.  One call folds 8 short sub-integrations at 0, another --
with other bytes and other models -- 8 at LINE_SUB - 4, half of them on either side of the line."""
import numpy as np

from helpers import fold_model as fm
from helpers import large_tensor as lt

TURN = 1 << 64
B, C = 2, 64

# ---- the filterbank
IN_SPECTRA = (1 << 25) + 2048
NBYTES = B * IN_SPECTRA * C
LINE_ROW = (lt.LINE - IN_SPECTRA * C) // C  # of beam 1
SUBINT_LEN, NR_SUBINTS, MAX_DELAY, NBIN = 2032, 4, 64, 64
WINDOW = SUBINT_LEN * NR_SUBINTS + MAX_DELAY
FIRST_AT_LINE = LINE_ROW - WINDOW // 2
FIRST_BELOW = 0


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


def models(seed, nr_subints, nbin):
    """dcs_bf_fold_model [B][nr_subints]: a few spectra per bin, seeded phases, a small acceleration of either sign."""
    rng = np.random.default_rng(seed)
    rows = [fm.model(int(rng.integers(0, 1 << 62)) * 4 + 1, TURN // (3 * nbin) + int(rng.integers(0, 1 << 40)), (-1) ** i * ((1 << 38) + i))
            for i in range(B * nr_subints)]
    return np.array(rows, dtype=fm.model_dtype).reshape(B, nr_subints)


def delays(seed):
    """int32 [B][C]: seeded entries in [0, MAX_DELAY], the last column at MAX_DELAY, so that the last row of the tensor is read."""
    t = np.random.default_rng(seed).integers(0, MAX_DELAY + 1, size=(B, C)).astype(np.int32)
    t[:, -1] = MAX_DELAY
    return t


def expected_fold(pat, first, wrapped=False):
    """(profiles uint32 [B][NR_SUBINTS][C][NBIN], hits) of the window at ``first``."""
    return fm.fold(window(pat, first, wrapped), models(81, NR_SUBINTS, NBIN), 0, SUBINT_LEN, NBIN, delays=delays(82), max_delay=MAX_DELAY)


# ---- the profiles
BIG_NBIN = 1024
OUT_SUBINTS = (1 << 13) + 16
SUBINT_BYTES = C * BIG_NBIN * 4
PROFILES_BYTES = B * OUT_SUBINTS * SUBINT_BYTES
LINE_SUB = (lt.LINE - OUT_SUBINTS * SUBINT_BYTES) // SUBINT_BYTES  # of beam 1
SHORT_LEN, SHORT_SUBINTS = 64, 8
FIRST_SUB_AT_LINE = LINE_SUB - SHORT_SUBINTS // 2
FIRST_SUB_BELOW = 0
PREFILL = 0x3C


def short_filterbank(seed):
    """uint8 [B][SHORT_SUBINTS * SHORT_LEN][C], no byte 0: every word of a folded bin that was hit differs from an empty one."""
    return np.random.default_rng(seed).integers(1, 256, size=(B, SHORT_SUBINTS * SHORT_LEN, C), dtype=np.uint8)


def expected_short(seed):
    """profiles uint32 [B][SHORT_SUBINTS][C][BIG_NBIN] of the call with this seed's bytes and models."""
    return fm.fold(short_filterbank(seed), models(seed + 1, SHORT_SUBINTS, BIG_NBIN), 0, SHORT_LEN, BIG_NBIN)[0]


def wrapped_subint(b, s):
    """(beam, sub-integration) where a store to (b, s) lands whose byte offset came out modulo 2^32."""
    g = b * OUT_SUBINTS + s
    g = g - lt.LINE // SUBINT_BYTES if g * SUBINT_BYTES >= lt.LINE else g
    return divmod(g, OUT_SUBINTS)
