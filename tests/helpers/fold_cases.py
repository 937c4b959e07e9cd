"""The case table of the pulsar folder's GPU tests (tests/test_gpu_fold.py), kept here so that tests/test_fold_forms.py can take
a census of the forms it presents to the launcher without a GPU, and the builders of its models and delay tables, which are
conditions on the inputs before a GPU sees them."""
from collections import namedtuple

import numpy as np

from helpers import fold_model as fm
from helpers.dedisperse_model import BAND_ASCENDING_100, BAND_DESCENDING_64

TURN = 1 << 64
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

CHANNELS = [1, 3, 64, 100, 317]
# 1, 2, 3, 64, 100, 1024 and both sides of every boundary in nbin between two forms: 64|65, 128|129, 256|257, 512|513
NBINS = [1, 2, 3, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024]
SUBINT_LENS = [1, 7, 513, 4096]
NR_SUBINTS = [1, 3]
BEAMS = [(1, 1), (3, 1), (8, 4), (8, 1)]  # nr_beams, beams_per_model
MODEL_KINDS = ["zero", "bin", "bin+1", "bin-1", "skip", "slow", "accel+", "accel-"]
DELAY_KINDS = ["none", "dm", "hand", "dm", "hand"]
LIMIT = 3 << 20   # bytes of a case's filterbank window, so that the model stays quick
GROUPS = 3        # a C's cases run as this many tests

Case = namedtuple("Case", "C nbin L S B bpm model delays hits first first_subint mask")


def cases():
    """C -> [Case]: every C with every nbin, while the other parameters rotate at different periods (tests/test_fold_forms.py
    holds what the table must contain); the largest are cut in beams and sub-integrations."""
    out = {}
    for ci, C in enumerate(CHANNELS):
        out[C] = []
        for i, nbin in enumerate(NBINS):
            n = i + 5 * ci
            L, S = SUBINT_LENS[n % 4], NR_SUBINTS[(n // 2) % 2]
            B, bpm = BEAMS[(n + ci) % 4]
            if B * S * L * C > LIMIT:
                B, bpm = (4, 4) if bpm == 4 else (1, 1)
            if B * S * L * C > LIMIT:
                S = 1
            out[C].append(Case(C, nbin, L, S, B, bpm, MODEL_KINDS[(n + i // 8) % 8], DELAY_KINDS[(n + i // 5) % 5], n % 3 != 2, (0, 5)[n % 2],
                               (0, 2)[(n // 3) % 2], n % 4 == 1))
    return out


def all_cases():
    return [c for rows in cases().values() for c in rows]


def census_calls():
    """(C, nbin, subint_len) of every fold_q8 call of the table."""
    return [(c.C, c.nbin, c.L) for c in all_cases()]


def step_of(kind, nbin):
    return {"zero": 0, "bin": TURN // nbin, "bin+1": TURN // nbin + 1, "bin-1": TURN // nbin - 1, "skip": TURN // 2 + TURN // 7,
            "slow": TURN // (nbin * 150), "accel+": TURN // (3 * nbin) + 12345, "accel-": TURN // (5 * nbin) + 54321}[kind]


def accel_of(kind):
    return {"accel+": (1 << 44) + 12345, "accel-": -(1 << 43) - 999}.get(kind, 0)


def models_of(case, seed):
    """dcs_bf_fold_model [P][S]: the case's kind of step in every row, a seeded phase0 -- one step below a wrap in the first
    row, the last unit of a turn in the last, so that the phase wraps at k = 1."""
    P = case.B // case.bpm
    rng = np.random.default_rng(seed)
    step, accel = step_of(case.model, case.nbin), accel_of(case.model)
    rows = []
    for p in range(P):
        for s in range(case.S):
            phase0 = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
            if (p, s) == (0, 0):
                phase0 = (TURN - step) % TURN
            elif (p, s) == (P - 1, case.S - 1):
                phase0 = TURN - 1
            rows.append(fm.model(phase0, step, accel))
    return np.array(rows, dtype=rows[0].dtype).reshape(P, case.S)


def band_of(C):
    """(freq_first_mhz, freq_step_mhz, sample_time_s): the two bands of helpers/dedisperse_model.py at their own C, the
    same spans in the other direction elsewhere."""
    if C == 64:
        return BAND_DESCENDING_64
    if C == 100:
        return BAND_ASCENDING_100
    return (830.0, 670.0 / C, 306.24e-6) if C % 2 else (1500.0, -670.0 / C, 306.24e-6)


def dms_of(P):
    return (10.0 + 12.5 * np.arange(P)).astype(np.float64)


def hand_table(case, max_delay, seed):
    """int32 [P][C]: seeded entries in [0, max_delay], the last column at max_delay itself, and, where the band has the
    columns, -1, INT32_MIN, max_delay + 1 and INT32_MAX, which fold their columns to zero."""
    P = case.B // case.bpm
    t = np.random.default_rng(seed).integers(0, max_delay + 1, size=(P, case.C)).astype(np.int64)
    t[:, -1] = max_delay
    for p in range(P):
        for i, bad in enumerate((-1, INT32_MIN, max_delay + 1, INT32_MAX)):
            if case.C >= 3:
                t[p, (7 * p + 5 * i + 1) % (case.C - 1)] = bad
    return t.astype(np.int32)


HAND_MAX_DELAY = 37


def mask_of(case, seed):
    if not case.mask:
        return None
    m = np.random.default_rng(seed).choice(np.array([1, 1, 1, 0x80, 0], np.uint8), size=case.C)
    if case.C >= 3:
        m[0], m[1] = 0, 1
    return m
