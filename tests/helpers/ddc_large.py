"""The shape of tests/test_gpu_ddc_large.py and what the host can say about tensors that exist on the device only
(helpers/large_tensor.py).  tests/test_ddc_large_plan.py walks the same plan without a device and shows that a byte offset
worked out in 32 bits cannot pass it.

Two input rows of 2^27 - 2 outputs each (T = 64: 2^31 + 16 samples) in a stride of 2^31 + 2^20 bytes: the smallest two-row
shape with a padded stride whose sample tensor passes 2^32 bytes; the line falls inside row 1, 65536 outputs before its end.
With two bands and rows of 2^16 + 2 pairs of padding the output passes 2^32 bytes too, inside the row of (band 1, input 1).
The device samples repeat a pattern whose period is an odd number of 4096-byte rows, so it does not divide 2^32 and the host
can produce the samples of any window of outputs."""
import numpy as np

from helpers import ddc_model as model
from helpers import large_tensor as lt

T, NI, NB = 64, 2, 2
NR_OUT = (1 << 27) - 2
ROW = 16 * (NR_OUT - 1) + T                   # 2^31 + 16 samples read of a row
IN_STRIDE = (1 << 31) + (1 << 20)
OUT_STRIDE = NR_OUT + (1 << 16) + 2
SAMPLES_BYTES = (NI - 1) * IN_STRIDE + ROW    # 2^32 + 2^20 + 16
OUT_BYTES = ((NB * NI - 1) * OUT_STRIDE + NR_OUT) * 8
WINDOW = 48                                   # outputs per sampled window: three tiles
PREFILL = 0xA5
BANDS = [(0x0EF00001, 0x12345678, 2.0 ** -20), (0xC0000001, 0xFEDCBA98, 2.0 ** -21)]
M_LINE_IN = (lt.LINE - IN_STRIDE) // 16                      # output of input 1 whose first sample is byte 2^32
M_LINE_OUT = (lt.LINE - 3 * OUT_STRIDE * 8) // 8             # output of (band 1, input 1) whose pair begins at byte 2^32


def pattern(seed):
    return lt.int8_pattern(4096, seed)


def taps(seed):
    return np.random.default_rng(seed).integers(-(model.MAX_ABS_SUM // T), model.MAX_ABS_SUM // T + 1, size=(NB, T, 2))


def plan(seed):
    """Sorted (input, m0) of the sampled windows: both ends of each row, the windows that straddle the line of either tensor
    (and end just below it, and begin just above it), the windows 2^32 bytes below those, and a few seeded ones."""
    w = {(i, m0) for i in range(NI) for m0 in (0, NR_OUT - WINDOW)}
    for m in (M_LINE_IN, M_LINE_OUT):
        w |= {(1, m - WINDOW), (1, m - WINDOW // 2), (1, m), (1, m + 4 * WINDOW)}
    w |= {(0, 4 * WINDOW)}  # 2^32 bytes below (1, M_LINE_IN + 4 WINDOW) in the samples; (0, 0) is below (1, M_LINE_IN)
    w |= {(int(i), int(m)) for i, m in zip(*np.random.default_rng(seed).integers(0, [[NI], [NR_OUT - WINDOW]], size=(2, 6)))}
    assert all(0 <= i < NI and 0 <= m0 <= NR_OUT - WINDOW for i, m0 in w)
    return sorted(w)


def window_samples(pat, i, m0, wrapped=False):
    """int8 [1][16 (WINDOW - 1) + T]: what outputs m0 .. m0 + WINDOW - 1 of input i read; ``wrapped``: as a kernel would read
    them whose byte offsets came out modulo 2^32."""
    off = i * IN_STRIDE + 16 * m0 + np.arange(16 * (WINDOW - 1) + T, dtype=np.int64)
    return lt.elements_of(pat, off % lt.LINE if wrapped else off).reshape(1, -1)


def expected(pat, tp, i, m0, wrapped=False):
    """float32 [NB][WINDOW][2] of a window."""
    return model.ddc(window_samples(pat, i, m0, wrapped), tp, BANDS, WINDOW, first_output=m0)[:, 0]


def out_offset(b, i, m):
    return ((b * NI + i) * OUT_STRIDE + m) * 8
