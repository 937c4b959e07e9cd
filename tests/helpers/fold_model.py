"""The numpy model of the pulsar folder (include/dcs_fold.h): phases in uint64 arithmetic that wraps as the device's does,
profiles, hits and the frequency scrunch, every one an exact integer.  tests/test_fold_model.py anchors it against a plain
Python loop over big integers; the GPU tests compare with it bit for bit."""
import numpy as np

from dc_sand_amd.fold import model_dtype

TURN = 1 << 64
U64 = np.uint64


def model(phase0, step, accel=0):
    """One dcs_bf_fold_model from Python ints; negative values are their two's complement."""
    out = np.zeros((), dtype=model_dtype)
    out[()] = (int(phase0) % TURN, int(step) % TURN, int(accel) % TURN)
    return out


def phases(m, n):
    """uint64 [n]: phi(k) = phase0 + k step + (k (k - 1) / 2) accel modulo 2^64, in array arithmetic, which wraps silently."""
    k = np.arange(n, dtype=U64)
    tri = k * (k - U64(1)) // U64(2)  # k = 0: 0 * (2^64 - 1) is 0; k < 2^32: the product is exact
    one = np.ones(n, dtype=U64)
    return one * U64(m["phase0"]) + k * U64(m["step"]) + tri * U64(m["accel"])


def bins(m, n, nbin):
    """int64 [n]: bin(k) = ((phi(k) >> 32) nbin) >> 32."""
    return (((phases(m, n) >> U64(32)) * U64(nbin)) >> U64(32)).astype(np.int64)


def columns_on(C, delays_row, max_delay, mask):
    """bool [C]: the columns that take part, and int64 [C]: their delays (0 where off)."""
    d = np.zeros(C, np.int64) if delays_row is None else np.asarray(delays_row, dtype=np.int64)
    on = (d >= 0) & (d <= max_delay)
    if mask is not None:
        on &= np.asarray(mask) != 0
    return on, np.where(on, d, 0)


def fold(fb, models, first, L, nbin, beams_per_model=1, delays=None, max_delay=0, mask=None, profiles=None, hits=None, first_subint=0,
         accumulate=False):
    """fb uint8 [B][in_spectra][C] and models [P][S] -> (profiles uint32 [B][out_subints][C][nbin], hits uint32
    [P][out_subints][nbin]).  ``profiles`` / ``hits``: what the outputs held before the call (copied; default: zeros of S
    sub-integrations); only the words the call addresses change, by assignment or, with ``accumulate``, by addition modulo 2^32."""
    B, in_spectra, C = fb.shape
    models = np.asarray(models, dtype=model_dtype)
    P, S = models.shape
    assert P * beams_per_model == B and first + S * L + max_delay <= in_spectra
    profiles = np.zeros((B, first_subint + S, C, nbin), np.uint32) if profiles is None else profiles.copy()
    hits = np.zeros((P, first_subint + S, nbin), np.uint32) if hits is None else hits.copy()
    cols = np.arange(C)
    for p in range(P):
        on, d = columns_on(C, None if delays is None else delays[p], max_delay, mask)
        for s in range(S):
            b_k = bins(models[p, s], L, nbin)
            h = np.bincount(b_k, minlength=nbin).astype(np.uint32)
            hits[p, first_subint + s] = hits[p, first_subint + s] + h if accumulate else h
            rows = first + s * L + np.arange(L)[:, None] + d[None, :]          # [L][C]
            index = (cols[None, :] * nbin + b_k[:, None]).ravel()               # word (c, j) of the sub-integration
            for b in range(p * beams_per_model, (p + 1) * beams_per_model):
                vals = np.where(on[None, :], fb[b][rows, cols[None, :]], 0).astype(np.float64)  # sums below 2^53: exact
                w = np.bincount(index, weights=vals.ravel(), minlength=C * nbin).astype(np.uint64).astype(np.uint32).reshape(C, nbin)
                profiles[b, first_subint + s] = profiles[b, first_subint + s] + w if accumulate else w
    return profiles, hits


def scrunch(profiles, first_subint, nr_subints, out=None, accumulate=False):
    """profiles uint32 [B][out_subints][C][nbin] -> uint64 [B][out_subints][nbin]: the sums over C of the addressed sub-integrations."""
    B, OS, C, nbin = profiles.shape
    out = np.zeros((B, OS, nbin), np.uint64) if out is None else out.copy()
    sl = slice(first_subint, first_subint + nr_subints)
    sums = profiles[:, sl].astype(np.uint64).sum(axis=2, dtype=np.uint64)
    out[:, sl] = out[:, sl] + sums if accumulate else sums
    return out


# ---- the plain-Python anchor: big integers, one spectrum at a time

def phase_int(m, k):
    return (int(m["phase0"]) + k * int(m["step"]) + (k * (k - 1) // 2) * int(m["accel"])) % TURN


def fold_slow(fb, models, first, L, nbin, beams_per_model=1, delays=None, max_delay=0, mask=None):
    """The same as fold() from zeroed outputs at first_subint 0, in Python integers."""
    B, in_spectra, C = fb.shape
    P, S = models.shape
    profiles = [[[[0] * nbin for _ in range(C)] for _ in range(S)] for _ in range(B)]
    hits = [[[0] * nbin for _ in range(S)] for _ in range(P)]
    for p in range(P):
        for s in range(S):
            for k in range(L):
                j = ((phase_int(models[p, s], k) >> 32) * nbin) >> 32
                hits[p][s][j] += 1
                for c in range(C):
                    d = 0 if delays is None else int(delays[p][c])
                    if (mask is not None and not mask[c]) or d < 0 or d > max_delay:
                        continue
                    for b in range(p * beams_per_model, (p + 1) * beams_per_model):
                        profiles[b][s][c][j] += int(fb[b, first + s * L + k + d, c])
    return np.array(profiles, dtype=np.uint64).astype(np.uint32).reshape(B, S, C, nbin), np.array(hits, dtype=np.uint32).reshape(P, S, nbin)
