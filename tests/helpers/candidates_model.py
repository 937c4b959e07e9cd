"""The model of the candidate sifter (include/dcs_candidates.h), twice: the five rules in vectorised
numpy, which the GPU tests hold the kernels to as integers and float bits, and a deliberately naive second implementation
-- Python loops over the cells and over each cell's window, Python floats -- that tests/test_candidates_model.py holds the
first to.  Both return (records of every candidate found, in order; count = [found, min(found, max_candidates)])."""
import numpy as np

NO_WIDTH = 0xFFFFFFFF
MAX_RADIUS = 8
# dcs_bf_candidate, restated
CANDIDATE = np.dtype([("beam", np.uint32), ("dm", np.uint32), ("width_index", np.uint32), ("block", np.uint32),
                      ("time", np.uint32), ("value", np.uint32), ("snr", np.float32), ("members", np.uint32)])


def collapse(snr, first_block, nr_blocks):
    """Rule 1.  snr float32 [B][nr_dm][nr_widths][peak_blocks] -> (s float32, i* uint32) [B][nr_dm][nr_blocks]."""
    snr = np.asarray(snr)
    assert snr.dtype == np.float32 and snr.ndim == 4 and first_block + nr_blocks <= snr.shape[3]
    x = snr[:, :, :, first_block:first_block + nr_blocks]
    s = np.full((x.shape[0], x.shape[1], nr_blocks), -np.inf, np.float32)
    best = np.full(s.shape, NO_WIDTH, np.uint32)
    for i in range(x.shape[2]):
        take = x[:, :, i] > s  # false for a NaN
        s = np.where(take, x[:, :, i], s)
        best = np.where(take, np.uint32(i), best)
    return s, best


def _records(at, s, best, members, peaks, first_block):
    rec = np.zeros(len(at), CANDIDATE)
    b, m, k = at[:, 0], at[:, 1], at[:, 2]
    i = best[b, m, k].astype(np.int64)  # a width index: a candidate's s is above -infinity
    rec["beam"], rec["dm"], rec["width_index"], rec["block"] = b, m, i, first_block + k
    rec["value"], rec["time"] = peaks[b, m, i, first_block + k, 0], peaks[b, m, i, first_block + k, 1]
    rec["snr"], rec["members"] = s[b, m, k], members[b, m, k]
    return rec


def _count(found, max_candidates):
    return np.array([found, min(found, max_candidates)], np.uint32)


def find_candidates(snr, peaks, first_block, nr_blocks, threshold, dm_radius, block_radius, max_candidates):
    """Rules 1 to 5, vectorised: one shifted view of the collapsed plane per cell of the window."""
    assert 0 <= dm_radius <= MAX_RADIUS and 0 <= block_radius <= MAX_RADIUS and np.isfinite(threshold)
    peaks = np.asarray(peaks)
    assert peaks.dtype == np.uint32 and peaks.shape == np.asarray(snr).shape + (2,)
    s, best = collapse(snr, first_block, nr_blocks)
    B, D, K = s.shape
    thr = np.float32(threshold)
    dr, br = int(dm_radius), int(block_radius)
    padded = np.full((B, D + 2 * dr, K + 2 * br), np.nan, np.float32)  # a cell that does not exist: beats and counts for nothing
    padded[:, dr:dr + D, br:br + K] = s
    beaten = np.zeros(s.shape, bool)
    members = np.zeros(s.shape, np.uint32)
    for dq in range(2 * dr + 1):
        for dk in range(2 * br + 1):
            q = padded[:, dq:dq + D, dk:dk + K]
            beaten |= q > s
            if dq < dr or (dq == dr and dk < br):  # (m_Q, k_Q) before (m_P, k_P)
                beaten |= q == s
            members += q >= thr
    at = np.argwhere((s >= thr) & ~beaten)  # in ascending (b, m, k)
    return _records(at, s, best, members, peaks, first_block), _count(len(at), max_candidates)


def find_candidates_naive(snr, peaks, first_block, nr_blocks, threshold, dm_radius, block_radius, max_candidates):
    """The same by four nested loops, cell by cell and window by window, on Python floats (every float32 is one exactly)."""
    snr, peaks = np.asarray(snr), np.asarray(peaks)
    B, D, W, _ = snr.shape
    thr = float(np.float32(threshold))
    s = [[[float("-inf")] * nr_blocks for _ in range(D)] for _ in range(B)]
    best = [[[NO_WIDTH] * nr_blocks for _ in range(D)] for _ in range(B)]
    for b in range(B):
        for m in range(D):
            for k in range(nr_blocks):
                for i in range(W):
                    v = float(snr[b, m, i, first_block + k])
                    if v > s[b][m][k]:
                        s[b][m][k], best[b][m][k] = v, i
    out = []
    for b in range(B):
        for m in range(D):
            for k in range(nr_blocks):
                sp = s[b][m][k]
                if not sp >= thr:
                    continue
                beaten, members = False, 0
                for mq in range(max(0, m - dm_radius), min(D - 1, m + dm_radius) + 1):
                    for kq in range(max(0, k - block_radius), min(nr_blocks - 1, k + block_radius) + 1):
                        sq = s[b][mq][kq]
                        if sq > sp or (sq == sp and (mq, kq) < (m, k)):
                            beaten = True
                        if sq >= thr:
                            members += 1
                if not beaten:
                    i = best[b][m][k]
                    value, time = peaks[b, m, i, first_block + k]
                    out.append((b, m, i, first_block + k, time, value, snr[b, m, i, first_block + k], members))
    return np.array(out, CANDIDATE).reshape(-1), _count(len(out), max_candidates)


def expected_buffer(records, count, prefill):
    """What d_cands holds after the call: ``prefill`` (a CANDIDATE array of max_candidates records, or more) with the first
    count[1] records replaced, and no other byte."""
    out = np.array(prefill, CANDIDATE)
    out[:int(count[1])] = records[:int(count[1])]
    return out


def same_bits(a, b):
    """Two CANDIDATE arrays compared as words: the snr as float bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def seeded_planes(B, nr_dm, nr_widths, peak_blocks, seed, special=0.0, plateau=True, step=4):
    """(snr, peaks) for the tests: float32 values in [-2, 10) on a grid of 1 / step -- coarse by default, so that equal
    maxima across widths, cells and tiles are common -- with a share ``special`` of NaN, +-inf and +-0 entries and, with
    ``plateau``, a rectangle of one value; peaks are distinct words, so a wrong cell or width shows."""
    rng = np.random.default_rng(seed)
    shape = (B, nr_dm, nr_widths, peak_blocks)
    snr = (rng.integers(-2 * step, 10 * step, size=shape) / float(step)).astype(np.float32)
    if special:
        pick = rng.random(shape)
        for j, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)):
            snr[(pick >= j * special / 5) & (pick < (j + 1) * special / 5)] = v
    if plateau and nr_dm >= 4 and peak_blocks >= 6 and nr_widths:
        snr[:, 1:4, :, 2:6] = np.float32(11.5)
    n = int(np.prod(shape))
    peaks = np.stack([np.arange(n, dtype=np.uint32) * np.uint32(2654435761), np.arange(n, dtype=np.uint32)[::-1]], axis=-1)
    return snr, peaks.reshape(shape + (2,))
