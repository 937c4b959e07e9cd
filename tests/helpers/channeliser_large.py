"""The shape of tests/test_gpu_channeliser_large.py and what the host can say about tensors that exist on the device only
(helpers/large_tensor.py).  tests/test_channeliser_large_plan.py walks the same plan without a device and shows that a byte
offset worked out in 32 bits cannot pass it.

N = 64, P = 1, two inputs of 2^18 + 1 blocks of 16 spectra: the smallest two-input shape at which both tensors pass 2^32
bytes -- a row is (2^22 + 16) 64 pairs = 2^31 + 8192 bytes, the float output 64 (2^18 + 1) 2 128 = 2^32 + 16384 bytes; one
block fewer and neither does.  The input's line falls inside row 1 at the first pair of block 2^18 - 1; the float output's
line at (channel 63, block 2^18 - 63, input 0).  A window is one block of one input: 16 spectra, 1024 pairs in, one run of 16
pairs in each of the 64 channels out.  The device input repeats a pattern of floats whose period is an odd number of 4096-byte
rows, so it does not divide 2^32 and the host can produce the pairs of any window."""
import numpy as np

from helpers import channeliser_model as model
from helpers import large_tensor as lt

N, P, NI = 64, 1, 2
BLOCKS = (1 << 18) + 1
NR_SPECTRA = 16 * BLOCKS
IN_STRIDE = NR_SPECTRA * N                    # pairs: no padding, the rows are 2^31 + 8192 bytes
IN_BYTES = NI * IN_STRIDE * 8                 # 2^32 + 16384
OUT_BYTES = N * BLOCKS * NI * 16 * 8          # 2^32 + 16384
OUT_Q8_BYTES = OUT_BYTES // 4
PREFILL = 0xA5
BLOCK_LINE_IN = (lt.LINE - IN_STRIDE * 8) // (16 * N * 8)   # block of input 1 whose first pair is byte 2^32
C_LINE_OUT = lt.LINE // (BLOCKS * NI * 128)                 # channel whose runs pass byte 2^32 of the float output
BLOCK_LINE_OUT = (lt.LINE - C_LINE_OUT * BLOCKS * NI * 128) // (NI * 128)  # ... from the run of this block and input 0 on


def pattern(seed):
    """float32 [period][1024]: integers in [-2000, 2000]."""
    p = lt.period_rows(4096)
    return np.random.default_rng(seed).integers(-2000, 2001, size=(p, 1024)).astype(np.float32)


def taps(seed):
    return model.seeded_taps(N, P, seed)


def gains():
    """2^-7 (1 + (c mod 7) / 8): with |taps| < 1 and |z| <= 2000 over 64 columns the outputs' rms is about 5000."""
    g = 2.0 ** -7 * (1.0 + (np.arange(N) % 7) / 8.0)
    return np.broadcast_to(g.astype(np.float32), (NI, N)).copy()


def plan(seed):
    """Sorted (input, block) of the sampled windows: both ends of each row; the blocks on both sides of the line of either
    tensor; the windows 2^32 bytes below those; and a few seeded ones."""
    w = {(i, b) for i in range(NI) for b in (0, BLOCKS - 1)}
    w |= {(1, BLOCK_LINE_IN - 1), (1, BLOCK_LINE_IN), (1, BLOCK_LINE_IN + 1)}
    w |= {(i, b) for i in range(NI) for b in (BLOCK_LINE_OUT - 1, BLOCK_LINE_OUT)}
    w |= {(0, 1)}  # 2^32 bytes below (1, BLOCK_LINE_IN + 1) in the input; (0, 0) is below (1, BLOCK_LINE_IN) in the input, and
    #                in the float output channel 0 of (i, 0) is below channel 63 of (i, BLOCK_LINE_OUT)
    w |= {(int(i), int(b)) for i, b in zip(*np.random.default_rng(seed).integers(0, [[NI], [BLOCKS]], size=(2, 4)))}
    assert all(0 <= i < NI and 0 <= b < BLOCKS for i, b in w)
    return sorted(w)


def in_offset(i, b):
    """Byte offset of the first pair that block b of input i reads."""
    return (i * IN_STRIDE + 16 * b * N) * 8


def window_pairs(pat, i, b, wrapped=False):
    """float32 [1][16 N][2]: what block b of input i reads; ``wrapped``: as a kernel would read it whose byte offsets came out
    modulo 2^32."""
    off = in_offset(i, b) + 4 * np.arange(16 * N * 2, dtype=np.int64)
    off = off % lt.LINE if wrapped else off
    return lt.elements_of(pat, off // 4).reshape(1, 16 * N, 2)


def expected(pat, h, W, i, b, wrapped=False):
    """float32 [N][16][2] of a window: the runs of its 64 channels."""
    X = model.channelise(window_pairs(pat, i, b, wrapped), h, W, N, P, 16)
    return model.tensor(X)[:, 0, 0]


def expected_q8(pat, h, W, i, b):
    T = model.tensor(model.channelise(window_pairs(pat, i, b), h, W, N, P, 16))
    q, n = model.quantise(T, gains()[i:i + 1])
    return q[:, 0, 0], int(n[0])


def out_offset(c, b, i, elem=4):
    """Byte offset of the run of (channel, block, input) in the output of words of elem bytes."""
    return ((c * BLOCKS + b) * NI + i) * 32 * elem
