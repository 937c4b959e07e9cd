"""The numpy model of the correlator (include/dcs_correlator.h): the exact integer visibilities of
every antenna pair b <= a of the sample tensor, and their integration with one rounding.  int64 throughout.
tests/test_correlator_model.py anchors it against plain Python-int arithmetic; the GPU tests hold the kernels to it bit for bit."""
import numpy as np

from helpers import stokes_model
from helpers.incoherent_model import same_bits  # noqa: F401  (the GPU tests compare float bits with it)

MAX_BLOCKS = 4095  # blocks per visibility at most: 4095 * 16 * 2 * 128^2 < 2^31 <= 4096 * 16 * 2 * 128^2


def nr_baselines(A):
    return A * (A + 1) // 2


def baseline(a, b):
    """The index of the pair (a, b), b <= a: row a of the lower triangle, the autocorrelation last in its row."""
    assert 0 <= b <= a
    return a * (a + 1) // 2 + b


def pairs(A):
    """(a, b) index arrays of the NB baselines in their order."""
    a, b = np.tril_indices(A)
    assert np.array_equal(a * (a + 1) // 2 + b, np.arange(nr_baselines(A)))
    return a, b


def full_matrix(ant, n):
    """int8 [C][K][A][16][2] -> (re, im) int64 [C][K / n][A][A]: V[a][b] = sum x_a conj(x_b) over the 16 n samples of every n
    blocks: re = sum re_a re_b + im_a im_b, im = sum im_a re_b - re_a im_b."""
    assert ant.dtype == np.int8 and ant.ndim == 5 and ant.shape[3:] == (16, 2)
    C, K, A = ant.shape[:3]
    assert 1 <= n <= MAX_BLOCKS and K % n == 0
    x = ant.astype(np.int64).reshape(C, K // n, n, A, 16, 2).transpose(0, 1, 2, 4, 3, 5).reshape(C, K // n, n * 16, A, 2)
    xr, xi = x[..., 0], x[..., 1]  # [C][nr_vis][n * 16][A]
    def outer(p, q):  # int64 in, int64 out: every product and sum an exact integer
        return np.einsum("cvta,cvtb->cvab", p, q, optimize=True)

    re = outer(xr, xr) + outer(xi, xi)
    im = outer(xi, xr) - outer(xr, xi)
    return re, im


def visibilities(ant, n):
    """int8 [C][K][A][16][2] -> int32 [C][K / n][NB][2]: the lower triangle of full_matrix, {re, im} innermost."""
    re, im = full_matrix(ant, n)
    a, b = pairs(ant.shape[2])
    out = np.stack([re[:, :, a, b], im[:, :, a, b]], axis=-1)
    assert np.abs(out).max(initial=0) < 1 << 31
    return out.astype(np.int32)


def integrate(vis, m, prior=None):
    """int32 [C][nr_vis][NB][2] -> float32 [nr_vis / m][C][NB][2]: the rule of stokes_model.integrate -- the exact int64 sum
    of m words, RN((float)S), and with ``prior`` RN(prior + that)."""
    return stokes_model.integrate(vis, m, prior=prior)
