"""The numpy model of the RFI flagger (include/dcs_rfi.h): the three contracts with uint64 sums, np.sort for the medians,
one float64 multiply and np.maximum for the limit.  Every integer involved is below 2^53, so float64 holds it exactly.
tests/test_rfi_model.py anchors it on plain Python integers; the GPU tests compare with it bit for bit."""
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class Thresholds:
    mean_thr: float = 6.0
    mean_floor: float = 0.0
    var_thr: float = 6.0
    var_floor: float = 0.0
    zero_dm_thr: float = 6.0
    zero_dm_floor: float = 0.0
    max_bad_blocks: int = 0


def moments(fb, first, nr_blocks, block_len):
    """uint8 [B][in_spectra][C] -> (cell sums uint32 [B][nr_blocks][C][2], zero-DM series uint32 [B][nr_blocks * block_len])."""
    B, _, C = fb.shape
    x = fb[:, first:first + nr_blocks * block_len].astype(np.uint64).reshape(B, nr_blocks, block_len, C)
    s1, s2 = x.sum(axis=2), (x * x).sum(axis=2)
    assert nr_blocks == 0 or s2.max(initial=0) < 1 << 32
    z = x.reshape(B, nr_blocks * block_len, C).sum(axis=2) & np.uint64(0xFFFFFFFF)
    return np.stack([s1, s2], axis=-1).astype(np.uint32), z.astype(np.uint32)


def lower_median(v, axis=-1):
    """The element of rank (K - 1) >> 1 of the sorted values along ``axis`` (kept as an axis of length 1)."""
    v = np.asarray(v)
    K = v.shape[axis]
    return np.take(np.sort(v, axis=axis), [(K - 1) >> 1], axis=axis)


def outliers(v, thr, floor, axis=-1):
    """The test of include/dcs_rfi.h on the unsigned integers ``v`` along ``axis``: bool, v's shape."""
    v = np.asarray(v, dtype=np.uint64)
    med = lower_median(v, axis)
    d = np.where(v > med, v - med, med - v)
    mad = lower_median(d, axis)
    with np.errstate(over="ignore"):
        limit = np.maximum(np.float64(thr) * mad.astype(np.float64), np.float64(floor))
    return d.astype(np.float64) > limit


def flags(cell_sums, zero_dm, block_len, thr=Thresholds()):
    """(cell flags uint8 [B][nr_blocks][C], channel masks uint8 [B][C], spectrum flags uint8 [B][W] or None, counts uint32
    [B][3]) of cell sums uint32 [B][nr_blocks][C][2] and the zero-DM series uint32 [B][W] or None."""
    s = np.asarray(cell_sums).astype(np.uint64)
    B, nr_blocks, C, _ = s.shape
    m = s[..., 0]
    q = np.uint64(block_len) * s[..., 1] - m * m
    cell = (outliers(m, thr.mean_thr, thr.mean_floor).astype(np.uint8) |
            (outliers(q, thr.var_thr, thr.var_floor).astype(np.uint8) << 1)) if nr_blocks else np.zeros((B, 0, C), np.uint8)
    bad = (cell != 0).sum(axis=1)
    mask = (bad <= thr.max_bad_blocks).astype(np.uint8)
    counts = np.zeros((B, 3), np.uint32)
    counts[:, 0] = bad.sum(axis=1)
    counts[:, 1] = (mask == 0).sum(axis=1)
    spectrum = None
    if zero_dm is not None:
        z = np.asarray(zero_dm)
        spectrum = (outliers(z, thr.zero_dm_thr, thr.zero_dm_floor) if z.shape[1] else np.zeros(z.shape, bool)).astype(np.uint8)
        counts[:, 2] = spectrum.sum(axis=1)
    return cell, mask, spectrum, counts


def clean(fb, first, nr_blocks, block_len, fill, cell_flags=None, channel_mask=None, spectrum_flags=None, out=None, first_out=0):
    """(out uint8 [B][out_spectra][C] with rows first_out .. first_out + W - 1 written, bytes replaced uint64 [B]); ``out``
    defaults to W rows of zeros."""
    B, _, C = fb.shape
    W = nr_blocks * block_len
    x = fb[:, first:first + W]
    rep = np.zeros((B, W, C), bool)
    if channel_mask is not None:
        rep |= (np.asarray(channel_mask) == 0)[:, None, :]
    if cell_flags is not None:
        rep |= np.repeat(np.asarray(cell_flags) != 0, block_len, axis=1)
    if spectrum_flags is not None:
        rep |= (np.asarray(spectrum_flags) != 0)[:, :, None]
    out = np.zeros((B, first_out + W, C), np.uint8) if out is None else out.copy()
    out[:, first_out:first_out + W] = np.where(rep, np.uint8(fill), x)
    return out, rep.reshape(B, -1).sum(axis=1).astype(np.uint64)


# ---- the seeded recipe: noise with a channel of doubled noise, a dead channel, a channel raised for three blocks and a
# four-spectrum broadband burst

RECIPE_SHAPE = (2, 16, 64, 256)  # B, nr_blocks, block_len, C
RECIPE_BURST = (1, 500, 504)     # beam, first and one past the last spectrum


def recipe():
    """uint8 [2][1024][256]."""
    rng = np.random.default_rng(20261021)
    B, nb, n, C = RECIPE_SHAPE
    T = nb * n

    def q8(x):
        return np.clip(np.rint(x), 0, 255).astype(np.uint8)

    fb = q8(rng.normal(128, 16, (B, T, C)))
    fb[0, :, 37] = q8(rng.normal(128, 32, T))
    fb[1, :, 90] = 128
    fb[0, 3 * n:6 * n, 200] = q8(fb[0, 3 * n:6 * n, 200].astype(np.int64) + 12)
    fb[1, 500:504, :] = q8(fb[1, 500:504, :].astype(np.int64) + 10)
    return fb
