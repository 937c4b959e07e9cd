"""The shapes, DM lists, tables and masks of the dedispersion's band, smooth and random GPU tests
(tests/test_gpu_dedisperse.py), kept here so that tests/test_dedisperse_paths.py can take a census of them without a GPU."""
import numpy as np

from helpers.dedisperse_model import (BAND_ASCENDING_100, BAND_DESCENDING_64, DMS_40, INT32_MAX, INT32_MIN, dm_delays,
                                      smooth_table)

# ------------------------------------------------------------------------------------- planes with the tables dm_delays makes

DM_SETS = {1: DMS_40[39:], 7: DMS_40[3::6], 40: DMS_40}  # 97.5 alone; 7.5, 22.5 .. 97.5; all
assert [len(v) for v in DM_SETS.values()] == [1, 7, 40]
SPECTRA = [1, 3, 4, 5, 63, 64, 65, 257, 1000]


def plane_cases():
    """Every nr_spectra twice, with B, nr_dm, first_spectrum and first_out rotating through their values at different
    periods, so that every value of each meets both bands and several sizes."""
    out = []
    for r in range(2):
        for i, T in enumerate(SPECTRA):
            k = i + 4 * r
            out.append((T, (1, 3)[(k + r) % 2], (1, 7, 40)[k % 3], (0, 1, 6)[(k // 2 + r) % 3], (0, 5)[(k // 3) % 2]))
    return out


CASES = plane_cases()
assert {c[1] for c in CASES} == {1, 3} and {c[2] for c in CASES} == {1, 7, 40} and {c[3] for c in CASES} == {0, 1, 6}
assert {c[4] for c in CASES} == {0, 5} and len(set(CASES)) == 18

# ------------------------------------------------------------------------------------------------------- ragged, any, mask

RAGGED_C = [1, 3, 17, 257]
RAGGED_CASES = ((7, 600, 65, 3, 1), (40, 1330, 257, 1, 6), (1, 90, 1000, 2, 0), (19, 333, 513, 1, 3))  # nr_dm, top, T, B, first

ANY_SHAPE = (64, 2, 300, 50000, 9)  # C, B, T, max_delay, nr_dm


def any_tables():
    """A random table with entries in [0, max_delay]; the same with entries outside [0, max_delay] sprinkled in and a DM
    whose every term drops; and a smooth table -- one that is staged -- with the same bad entries."""
    C, _, _, max_delay, nr_dm = ANY_SHAPE
    rng = np.random.default_rng(50000)
    table = rng.integers(0, max_delay + 1, size=(nr_dm, C)).astype(np.int32)
    table[0, 0], table[1, 1] = 0, max_delay
    bad = table.copy()
    pos = rng.choice(bad.size, size=40, replace=False)
    bad.reshape(-1)[pos] = np.resize(np.array([-1, INT32_MIN, max_delay + 1, INT32_MAX], np.int64), 40).astype(np.int32)
    bad[5] = np.resize(np.array([-1, INT32_MIN, max_delay + 1, INT32_MAX, -77, 2**30], np.int64), C).astype(np.int32)
    smooth = smooth_table(C, nr_dm, 400, seed=3)
    smooth.reshape(-1)[pos] = bad.reshape(-1)[pos]
    smooth[5] = bad[5]
    return table, bad, smooth


MASK_DMS = DMS_40[30:37]


def some_mask(C):
    """Any non-zero byte keeps the column; a whole chunk of columns that no DM takes."""
    mask = np.random.default_rng(3).integers(0, 2, size=C).astype(np.uint8) * 0x80
    mask[:34] = 0
    return mask


def table_255(C):
    return np.stack([np.zeros(C, np.int32), smooth_table(C, 2, 300, seed=C)[1]])


CAPTURE_DM_SETS = [DMS_40[3::6], DMS_40[20:27], DMS_40[33:]]


def capture_mask(i, C):
    return (np.random.default_rng(70 + i).integers(0, 4, size=C) > 0).astype(np.uint8)


CHAIN_BAND = (829.68, 10.64, 306.24e-6)  # f0, df of the spectra's channels, and the sample time


def calls():
    """(table, nr_spectra, max_delay, mask) of every dedispersion call those tests make (the example, which makes its
    table itself, aside)."""
    for C, band in ((64, BAND_DESCENDING_64), (100, BAND_ASCENDING_100)):
        for T, _, nr_dm, _, _ in CASES:
            table = dm_delays(C, *band, DM_SETS[nr_dm])
            yield table, T, int(table.max()), None
        table = dm_delays(C, *band, DMS_40[33:])
        yield table, 700, int(table.max()), None
    for C in RAGGED_C:
        for nr_dm, top, T, _, _ in RAGGED_CASES:
            table = smooth_table(C, nr_dm, top, seed=C + nr_dm)
            yield table, T, int(table.max()), None
    for table in any_tables():
        yield table, ANY_SHAPE[2], ANY_SHAPE[3], None
    table = dm_delays(100, *BAND_ASCENDING_100, MASK_DMS)
    for mask in (None, np.ones(100, np.uint8), some_mask(100), np.zeros(100, np.uint8)):
        yield table, 130, int(table.max()), mask
    for C in (1030, 1024):
        yield table_255(C), 100, 300, None
    top = max(int(dm_delays(100, *BAND_ASCENDING_100, d).max()) for d in CAPTURE_DM_SETS)
    for i, dms in enumerate(CAPTURE_DM_SETS):
        yield dm_delays(100, *BAND_ASCENDING_100, dms), 200, top, capture_mask(i, 100)
    f0, df, ts = CHAIN_BAND
    table = dm_delays(64, f0 + 63 * df, -df, ts, DMS_40[33:])
    yield table, 300, int(table.max()), None
