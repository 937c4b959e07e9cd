"""The numpy model of the 8-bit search filterbanks (include/dcs_filterbank.h): the three contracts
restated.  tests/test_filterbank_model.py anchors it against exact rationals and plain Python loops; the GPU tests hold
the kernels to it bit for bit."""
import numpy as np


def spectra_sums(spectra, prior=None):
    """float32 [T][C][B] -> float64 [C][B][2] = {s1, s2}: from {0, 0}, or from ``prior``, for t in order
    s1 = RN64(s1 + x), s2 = RN64(s2 + x * x) with x the double of the float (x * x is exact in a double)."""
    spectra = np.asarray(spectra)
    assert spectra.dtype == np.float32 and spectra.ndim == 3
    T, C, B = spectra.shape
    sums = np.zeros((C, B, 2), np.float64) if prior is None else np.array(prior, dtype=np.float64)
    assert sums.shape == (C, B, 2)
    with np.errstate(all="ignore"):
        for t in range(T):  # a Python loop over t: the order is the contract
            x = spectra[t].astype(np.float64)
            sums[:, :, 0] = sums[:, :, 0] + x
            sums[:, :, 1] = sums[:, :, 1] + x * x
    return sums


def scales(sums, count, target_std):
    """float64 [C][B][2] -> float32 [C][B][2] = {mu, k}, every operation in numpy float64, rounded once."""
    sums = np.asarray(sums)
    assert sums.dtype == np.float64 and sums.shape[-1] == 2 and 1 <= int(count) < 1 << 53
    with np.errstate(all="ignore"):
        N = np.float64(int(count))
        m = sums[..., 0] / N
        var = sums[..., 1] / N - m * m
        sd = np.where(var > 0, np.sqrt(np.where(var > 0, var, 0.0)), 0.0)  # a NaN var gives 0
        k = np.where(sd > 0, (np.float64(np.float32(target_std)) / np.where(sd > 0, sd, 1.0)).astype(np.float32), np.float32(0))
        return np.stack([m.astype(np.float32), k.astype(np.float32)], axis=-1)


def quantise(spectra, scale, level):
    """float32 [T][C][B] and scales float32 [C][B][2] -> (q uint8 [T][C][B], clipped bool [T][C][B]), in float32:
    d = x - mu, y = d * k + level (two roundings), r = rint(y) (ties to even); q = 0 for a NaN y, else clamp(r, 0, 255);
    clipped where y is NaN, r < 0 or r > 255."""
    spectra, scale = np.asarray(spectra), np.asarray(scale)
    assert spectra.dtype == np.float32 and scale.dtype == np.float32 and scale.shape == spectra.shape[1:] + (2,)
    with np.errstate(all="ignore"):
        d = spectra - scale[None, :, :, 0]
        y = d * scale[None, :, :, 1]
        y = y + np.float32(level)
        assert d.dtype == y.dtype == np.float32
        r = np.rint(y)
        nan = np.isnan(y)
        clipped = nan | (r < 0) | (r > 255)
        q = np.where(nan, np.float32(0), np.clip(r, 0, 255)).astype(np.uint8)
    return q, clipped


def filterbank(spectra, scale, level, descending=False, out=None, first=0):
    """The bytes uint8 [B][out_spectra][C] (``out``, or a fresh one of exactly T rows) with rows first .. first + T - 1
    of every beam written, and the clipped elements per beam, uint64 [B]."""
    q, clipped = quantise(spectra, scale, level)
    T, C, B = q.shape
    rows = np.transpose(q, (2, 0, 1))  # [B][T][C]
    if descending:
        rows = rows[:, :, ::-1]
    if out is None:
        out = np.zeros((B, first + T, C), np.uint8)
    else:
        out = np.array(out, dtype=np.uint8)
    assert out.shape[0] == B and out.shape[2] == C and first + T <= out.shape[1]
    out[:, first:first + T, :] = rows
    return out, clipped.sum(axis=(0, 1)).astype(np.uint64)


def same_bits(got, exp):
    """None if the arrays (float32, float64 or integers of one dtype) agree bit for bit, else the first difference.  Two
    NaNs agree: IEEE 754 leaves a NaN's sign and payload to the implementation, so the contract cannot state them."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return ("shape / dtype", got.shape, exp.shape, got.dtype, exp.dtype)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    differ = got.view(u).ravel() != exp.view(u).ravel()
    if got.dtype.kind == "f":
        differ &= ~(np.isnan(got.ravel()) & np.isnan(exp.ravel()))
    bad = np.flatnonzero(differ)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (bad.size, np.unravel_index(i, got.shape), got.ravel()[i], exp.ravel()[i])
