"""The numpy model of the incoherent dedispersion (include/dcs_dedisperse.h): both contracts
restated.  tests/test_dedisperse_model.py anchors it against exact rationals and plain Python loops; the GPU tests hold the
kernels to it bit for bit."""
import numpy as np

INT32_MAX, INT32_MIN = 2**31 - 1, -(2**31)
K_DM = 4.148808e3

# (freq_first_mhz, freq_step_mhz, sample_time_s) of the two bands of the GPU tests: with DMs 0, 2.5 .. 97.5 the delays run
# from 0 to about 1330 spectra and take all four residues mod 4
BAND_DESCENDING_64 = (1500.0, -10.64, 306.24e-6)
BAND_ASCENDING_100 = (830.0, 6.77, 306.24e-6)
DMS_40 = np.arange(40, dtype=np.float64) * 2.5


def column_frequencies(C, freq_first, freq_step):
    """f_j = RN(first + RN(j * step)), float64 [C]."""
    return np.float64(freq_first) + np.arange(C, dtype=np.float64) * np.float64(freq_step)


def dm_delays(C, freq_first, freq_step, sample_time, dms):
    """int32 [nr_dm][C]: every operation one numpy float64 operation, so rounded once; the divides are IEEE."""
    dms = np.asarray(dms, dtype=np.float64)
    with np.errstate(all="ignore"):
        f = column_frequencies(C, freq_first, freq_step)
        f_ref = np.float64(freq_first) if freq_step <= 0 else f[C - 1]
        a = np.float64(1.0) / (f * f)
        b = np.float64(1.0) / (f_ref * f_ref)
        s = ((np.float64(K_DM) * dms)[:, None] * (a - b)[None, :]) / np.float64(sample_time)
        high = np.isnan(s) | (s > 2147483647.0)
        low = s < -2147483648.0
        r = np.rint(np.where(high | low, 0.0, s))  # ties to even
    return np.where(high, INT32_MAX, np.where(low, INT32_MIN, r)).astype(np.int64).astype(np.int32)


def takes_part(delays, max_delay, mask=None):
    """bool [nr_dm][C]: the (DM, column) terms that are summed."""
    delays = np.asarray(delays)
    assert delays.dtype == np.int32 and delays.ndim == 2
    on = (delays >= 0) & (delays.astype(np.int64) <= int(max_delay))
    if mask is not None:
        on &= (np.asarray(mask) != 0)[None, :]
    return on


def dedisperse(filterbank, delays, first, nr_spectra, max_delay, mask=None, out=None, first_out=0):
    """filterbank uint8 [B][in_spectra][C], delays int32 [nr_dm][C] -> uint32 [B][nr_dm][out_spectra] (``out``, or a fresh
    one of exactly nr_spectra words per series) with words first_out .. first_out + nr_spectra - 1 of every series written:
    the sum mod 2^32 over the columns that take part of filterbank[b][first + t + d][c]."""
    filterbank, delays = np.asarray(filterbank), np.asarray(delays)
    assert filterbank.dtype == np.uint8 and filterbank.ndim == 3
    B, in_spectra, C = filterbank.shape
    nr_dm = delays.shape[0]
    assert delays.shape == (nr_dm, C) and first + nr_spectra + max_delay <= in_spectra
    on = takes_part(delays, max_delay, mask)
    if out is None:
        out = np.zeros((B, nr_dm, first_out + nr_spectra), np.uint32)
    else:
        out = np.array(out, dtype=np.uint32)
    assert out.shape[:2] == (B, nr_dm) and first_out + nr_spectra <= out.shape[2]
    for m in range(nr_dm):
        acc = np.zeros((B, nr_spectra), np.uint64)
        for c in np.flatnonzero(on[m]):
            r = first + int(delays[m, c])
            acc += filterbank[:, r:r + nr_spectra, c]
        out[:, m, first_out:first_out + nr_spectra] = (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def smooth_table(C, nr_dm, top, seed):
    """A seeded table that is smooth in the column and monotone in the DM, like dm_delays makes them, for any C: entry
    (m, j) = rint(m / (nr_dm - 1 or 1) * top * g_j) with g falling from 1 at column 0 to 0 at the last column along a seeded
    power law.  int32 [nr_dm][C], entries 0 .. top."""
    p = np.random.default_rng(seed).uniform(1.5, 3.0)
    x = np.arange(C, dtype=np.float64) / max(C - 1, 1)
    g = (1.0 - x) ** p if C > 1 else np.ones(1)
    scale = np.arange(nr_dm, dtype=np.float64) / max(nr_dm - 1, 1) if nr_dm > 1 else np.ones(1)
    return np.rint(scale[:, None] * top * g[None, :]).astype(np.int32)
