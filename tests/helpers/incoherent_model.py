"""The numpy model of the incoherent beam (include/dcs_incoherent_beam.h): exact integer block
powers of the antennas whose weight is not 0, and their integration with one rounding.  tests/test_incoherent_model.py
anchors it against plain Python-int loops; the GPU tests hold the kernels to it bit for bit."""
import numpy as np


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


def to_float(S):
    """RN((float)S) of every exact sum: np.float32 of a Python int goes through a double, which holds a sum below 2^53
    exactly, so the result is rounded once."""
    S = np.asarray(S, dtype=np.int64)
    assert S.min(initial=0) >= 0 and S.max(initial=0) < 1 << 53
    return np.array([np.float32(int(s)) for s in S.ravel()], dtype=np.float32).reshape(S.shape)


def integrate(P, n, prior=None):
    """Block powers [C][nr_blocks] -> spectra float32 [nr_blocks / n][C]: S exactly in int64, RN((float)S); with
    ``prior`` (the spectra before an accumulating call) RN(prior + RN((float)S))."""
    C, K = P.shape
    assert n >= 1 and K % n == 0
    S = P.astype(np.int64).reshape(C, K // n, n).sum(axis=2).T  # [K / n][C]
    out = to_float(S)
    if prior is not None:
        prior = np.asarray(prior, dtype=np.float32)
        assert prior.shape == out.shape
        out = (prior + out).astype(np.float32)  # float32 + float32: one rounded add
    return out


def same_bits(got, exp):
    """None if the float32 arrays agree bit for bit, else the first difference."""
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    if got.shape != exp.shape:
        return ("shape", got.shape, exp.shape)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != exp.view(np.uint32).ravel())
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (bad.size, np.unravel_index(i, got.shape), float(got.ravel()[i]), float(exp.ravel()[i]))
