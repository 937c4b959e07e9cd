"""The numpy model of the Stokes detection (include/dcs_stokes.h): exact integer block Stokes
parameters of two int8 beam tensors, and their integration with one rounding.  int64 throughout.
tests/test_stokes_model.py anchors it against plain Python-int arithmetic; the GPU tests hold the kernels to it bit for bit."""
import numpy as np

_CHUNK = 1 << 18  # rows (of 16 samples) taken at a time: bounds the int64 temporaries of a large tensor


def block_stokes(x, y, nr_stokes):
    """int8 [C][nt / 16][B][16][2] twice (polarisations x and y) -> int32 [C][nt / 16][B][nr_stokes]: I = Pxx + Pyy, and
    with nr_stokes = 4 also Q = Pxx - Pyy, U = 2 sum(xr yr + xi yi), V = 2 sum(xi yr - xr yi), over the block's 16 samples."""
    assert nr_stokes in (1, 4)
    assert x.dtype == np.int8 and x.ndim == 5 and x.shape[3:] == (16, 2) and y.dtype == np.int8 and y.shape == x.shape
    xs, ys = x.reshape(-1, 16, 2), y.reshape(-1, 16, 2)
    out = np.empty((xs.shape[0], nr_stokes), dtype=np.int64)
    for lo in range(0, xs.shape[0], _CHUNK):
        a, b = xs[lo:lo + _CHUNK].astype(np.int64), ys[lo:lo + _CHUNK].astype(np.int64)
        xr, xi, yr, yi = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
        pxx = (xr * xr + xi * xi).sum(axis=1)
        pyy = (yr * yr + yi * yi).sum(axis=1)
        o = out[lo:lo + _CHUNK]
        o[:, 0] = pxx + pyy
        if nr_stokes == 4:
            o[:, 1] = pxx - pyy
            o[:, 2] = 2 * (xr * yr + xi * yi).sum(axis=1)
            o[:, 3] = 2 * ((xi * yr).sum(axis=1) - (xr * yi).sum(axis=1))
    assert np.abs(out).max(initial=0) <= 1 << 20
    return out.astype(np.int32).reshape(x.shape[:3] + (nr_stokes,))


def to_float(S):
    """RN((float)S) of every exact signed sum: np.float32 of a Python int goes through a double, which holds a sum below
    2^53 in magnitude exactly, so the result is rounded once."""
    S = np.asarray(S, dtype=np.int64)
    assert np.abs(S).max(initial=0) < 1 << 53
    return np.array([np.float32(int(s)) for s in S.ravel()], dtype=np.float32).reshape(S.shape)


def integrate(block, n, prior=None):
    """Block Stokes [C][nr_blocks][B][NS] -> spectra float32 [nr_blocks / n][C][B][NS]: S exactly in int64, RN((float)S);
    with ``prior`` (the spectra before an accumulating call) RN(prior + RN((float)S))."""
    C, K, B, NS = block.shape
    assert n >= 1 and K % n == 0
    S = block.astype(np.int64).reshape(C, K // n, n, B, NS).sum(axis=2).transpose(1, 0, 2, 3)  # [K / n][C][B][NS]
    out = to_float(S)
    if prior is not None:
        prior = np.asarray(prior, dtype=np.float32)
        assert prior.shape == out.shape
        with np.errstate(invalid="ignore"):
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
