"""The numpy model of the single-pulse search (include/dcs_single_pulse.h): the three contracts
restated.  tests/test_single_pulse_model.py anchors it against plain Python loops over Python integers and exact rationals;
the GPU tests hold the kernels to it bit for bit."""
import numpy as np

NO_TIME = 0xFFFFFFFF  # the time of a width that takes no part, and the best width where none does
MAX_WIDTH_LIMIT = 4096


# The chain of tests/test_gpu_single_pulse.py and of the CPU test that chooses its numbers: C = 64 columns of noise bytes with
# a pulse of 8 spectra along the track of one DM of DMS_40, dedispersed into 1024 outputs and searched with six widths.
CHAIN = dict(C=64, outputs=1024, dm_index=20, row=500, pulse_spectra=8, pulse_height=24, widths=(1, 2, 4, 8, 16, 32), max_width=32,
             block_len=256, count=1024)


def chain_filterbank(table, seed):
    """uint8 [1][outputs + max delay][C]: clip(rint(N(128, 16))) with pulse_height added on pulse_spectra rows along the
    track table[dm_index] from row ``row``.  ``table`` is the delay table int32 [nr_dm][C]."""
    k = CHAIN
    rows = k["outputs"] + int(table.max())
    x = np.random.default_rng(seed).normal(128.0, 16.0, size=(1, rows, k["C"]))
    for c in range(k["C"]):
        r = k["row"] + int(table[k["dm_index"], c])
        x[0, r:r + k["pulse_spectra"], c] += k["pulse_height"]
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def nr_blocks_of(nr_spectra, block_len):
    return -(-int(nr_spectra) // int(block_len))


def takes_part(widths, max_width):
    """bool [nr_widths]: the widths in [1, max_width]."""
    w = np.asarray(widths, dtype=np.uint32).astype(np.int64)
    return (w >= 1) & (w <= int(max_width))


def sums(plane, first, nr_spectra, out=None):
    """plane uint32 [B][nr_dm][plane_spectra] -> uint64 [B][nr_dm][2] = {sum x, sum x^2 mod 2^64} over the words
    first .. first + nr_spectra - 1; added to ``out`` mod 2^64 where it is given (accumulate)."""
    plane = np.asarray(plane)
    assert plane.dtype == np.uint32 and plane.ndim == 3 and first + nr_spectra <= plane.shape[2]
    x = plane[:, :, first:first + nr_spectra].astype(np.uint64)
    with np.errstate(over="ignore"):
        res = np.stack([x.sum(axis=2, dtype=np.uint64), (x * x).sum(axis=2, dtype=np.uint64)], axis=-1)
        if out is not None:
            res = res + np.asarray(out, dtype=np.uint64)
    return res


def peaks(plane, first, nr_spectra, widths, max_width, block_len, out=None, first_block=0):
    """plane uint32 [B][nr_dm][plane_spectra] -> uint32 [B][nr_dm][nr_widths][peak_blocks][2] (``out``, or a fresh one of
    exactly nr_blocks blocks) with blocks first_block .. first_block + nr_blocks - 1 written: per width that takes part the
    largest S_w[t] = P[t + w] - P[t] (a uint32 cumulative sum, so mod 2^32) of the block and the first t that attains it;
    {0, 0xFFFFFFFF} for a width outside [1, max_width]."""
    plane = np.asarray(plane)
    widths = np.asarray(widths, dtype=np.uint32)
    assert plane.dtype == np.uint32 and plane.ndim == 3 and block_len % 64 == 0 and 64 <= block_len <= 4096
    assert 1 <= max_width <= MAX_WIDTH_LIMIT and first + nr_spectra + max_width - 1 <= plane.shape[2]
    B, nr_dm, _ = plane.shape
    nb = nr_blocks_of(nr_spectra, block_len)
    if out is None:
        out = np.zeros((B, nr_dm, widths.size, first_block + nb, 2), np.uint32)
    else:
        out = np.array(out, dtype=np.uint32)
    assert out.shape[:3] == (B, nr_dm, widths.size) and first_block + nb <= out.shape[3]
    if nr_spectra == 0:
        return out
    window = plane[:, :, first:first + nr_spectra + max_width - 1]
    with np.errstate(over="ignore"):
        prefix = np.concatenate([np.zeros((B, nr_dm, 1), np.uint32), np.cumsum(window, axis=2, dtype=np.uint32)], axis=2)
    on = takes_part(widths, max_width)
    for i, w in enumerate(widths.tolist()):
        if not on[i]:
            out[:, :, i, first_block:first_block + nb] = (0, NO_TIME)
            continue
        with np.errstate(over="ignore"):
            s = prefix[:, :, w:w + nr_spectra] - prefix[:, :, :nr_spectra]  # uint32: wraps
        for k in range(nb):
            blk = s[:, :, k * block_len:(k + 1) * block_len]
            at = np.argmax(blk, axis=2)  # the first of equal maxima
            out[:, :, i, first_block + k, 0] = np.take_along_axis(blk, at[..., None], axis=2)[..., 0]
            out[:, :, i, first_block + k, 1] = (at + k * block_len).astype(np.uint32)
    return out


def snr(peak_plane, widths, max_width, sum_pairs, count, first_block=0, nr_blocks=None, out=None, best_out=None):
    """peaks uint32 [B][nr_dm][nr_widths][peak_blocks][2], sums uint64 [B][nr_dm][2] -> (snr float32
    [B][nr_dm][nr_widths][peak_blocks], best uint32 [B][nr_dm][peak_blocks]), the blocks first_block .. first_block +
    nr_blocks - 1 written into ``out`` / ``best_out`` (or fresh zeroed ones).  float64, one numpy operation per stated
    operation, so each rounded once."""
    peak_plane, widths = np.asarray(peak_plane), np.asarray(widths, dtype=np.uint32)
    sum_pairs = np.asarray(sum_pairs)
    assert peak_plane.dtype == np.uint32 and sum_pairs.dtype == np.uint64 and count > 0
    B, nr_dm, nw, pb, _ = peak_plane.shape
    assert nw == widths.size and sum_pairs.shape == (B, nr_dm, 2)
    nr_blocks = pb - first_block if nr_blocks is None else nr_blocks
    sl = slice(first_block, first_block + nr_blocks)
    out = np.zeros((B, nr_dm, nw, pb), np.float32) if out is None else np.array(out, dtype=np.float32)
    best_out = np.zeros((B, nr_dm, pb), np.uint32) if best_out is None else np.array(best_out, dtype=np.uint32)
    with np.errstate(all="ignore"):
        N = np.float64(count)
        mean = sum_pairs[..., 0].astype(np.float64) / N
        var = sum_pairs[..., 1].astype(np.float64) / N - mean * mean
        wd = widths.astype(np.float64)[None, None, :, None]
        value = peak_plane[:, :, :, sl, 0].astype(np.float64)
        num = value - wd * mean[:, :, None, None]
        den = np.sqrt(wd * var[:, :, None, None])
        res = (num / den).astype(np.float32)
    res = np.where((var > 0)[:, :, None, None], res, np.float32(0.0))
    res = np.where(takes_part(widths, max_width)[None, None, :, None], res, np.float32(-np.inf)).astype(np.float32)
    out[:, :, :, sl] = res
    if nw:
        best = np.argmax(res, axis=2).astype(np.uint32)  # the lowest index of equal maxima
        best[np.max(res, axis=2) == -np.inf] = NO_TIME
    else:
        best = np.full((B, nr_dm, nr_blocks), NO_TIME, np.uint32)
    best_out[:, :, sl] = best
    return out, best_out
