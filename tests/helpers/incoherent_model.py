"""The numpy model of the incoherent beam (include/dcs_incoherent_beam.h): exact integer block
powers of the antennas whose weight is not 0, and their integration with one rounding.  tests/test_incoherent_model.py
anchors it against plain Python-int loops; the GPU tests hold the kernels to it bit for bit."""
import numpy as np

from helpers import stokes_model
from helpers.stokes_model import same_bits, to_float  # noqa: F401  (the tests use both through this module)


def flags(weights, A):
    """Which antennas take part: all without weights, else those whose value != 0 (-0.0 is 0; NaN and Inf are not)."""
    if weights is None:
        return np.ones(A, dtype=bool)
    w = np.asarray(weights, dtype=np.float32)
    assert w.shape == (A,)
    return w != 0


def block_power(ant, weights=None):
    """int8 [C][nt / 16][A][16][2] -> uint32 [C][nt / 16]: re^2 + im^2 summed over the block's 16 samples and over the
    antennas taking part, in int64 (at most 2^27)."""
    assert ant.dtype == np.int8 and ant.ndim == 5 and ant.shape[3:] == (16, 2)
    x = ant.astype(np.int64)
    per_antenna = (x * x).sum(axis=(3, 4))  # [C][K][A]
    P = (per_antenna * flags(weights, ant.shape[2]).astype(np.int64)).sum(axis=2)
    assert P.max(initial=0) <= 1 << 27
    return P.astype(np.uint32)


def integrate(P, n, prior=None):
    """Block powers [C][nr_blocks] -> spectra float32 [nr_blocks / n][C]: the rule of stokes_model.integrate -- S exactly in
    int64, RN((float)S), and with ``prior`` (the spectra before an accumulating call) RN(prior + that) -- on words that are
    no less than 0, so no sum is either."""
    C, K = P.shape
    assert n >= 1 and K % n == 0 and P.min(initial=0) >= 0
    if prior is not None:
        prior = np.asarray(prior, dtype=np.float32)
        assert prior.shape == (K // n, C)
        prior = prior.reshape(K // n, C, 1, 1)
    out = stokes_model.integrate(P.reshape(C, K, 1, 1), n, prior=prior).reshape(K // n, C)
    assert prior is not None or out.min(initial=0) >= 0
    return out


def full_range_words(C=3, K=12):
    """Seeded block powers uint32 [C][K] over the whole 32-bit range, 0xFFFFFFFF, 0x80000000 and 0x7FFFFFFF among them: what
    the detection never makes (it ends at 2^27) and the integration's contract covers -- words and sums that are unsigned."""
    P = np.random.default_rng(32).integers(0, 1 << 32, size=(C, K), dtype=np.uint64).astype(np.uint32)
    P[0, 0], P[C // 2, K // 2], P[-1, -1] = 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF
    return P
