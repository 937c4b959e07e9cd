"""The delay tables of tests/test_gpu_beamformer_exact_slow.py, beam-major [b * A + a] as the beamformers take them, and the
condition every case of that file states on the CPU before it calls anything (tests/test_beamformer_model.py holds
pair_classes to bf_math.h compiled for the host on these very tables)."""
import numpy as np

from conftest import rand_table
from helpers.beamformer_model import FAST_HIGH, SLOW, UNCLEAR, pair_classes

SAMPLING_PERIOD = 1e-7  # BeamformerParameters' default


def one_slow_pair(A, B, seed=0):
    """rand_table (all pairs of the lowest class) with ONE finite slow pair at (beam B // 2, antenna A // 2):
    fPhase_rad = 40000.  Every other pair is a fast-class pair that a beamformer nevertheless makes with coeff_slow."""
    t = rand_table(A * B, seed=A + B + seed)
    t["fPhase_rad"][(B // 2) * A + A // 2] = 40000.0
    return t


def one_full_degree_pair(A, B, seed=0):
    """The same with fPhase_rad = 20000: one pair of the full-degree fast class, which puts every pair of the table (block)
    on the full-degree polynomials in a beamformer and only its own run of pairs in the generator."""
    t = rand_table(A * B, seed=A + B + seed)
    t["fPhase_rad"][(B // 2) * A + A // 2] = 20000.0
    return t


def all_slow(A, B, seed=0):
    """Every pair's fPhase_rad seeded in +-[40000, 100000]; pair 1 (or 0) with fDelayRate_sps = 1e-30 (a rate term below the
    constant divide's range), the last pair with 1e-2 (|fRotation| of some 1e5 from the rate alone)."""
    n = A * B
    rng = np.random.default_rng(1000 + A + B + seed)
    t = rand_table(n, seed=A + B + seed)
    t["fPhase_rad"] = rng.choice([-1.0, 1.0], n) * rng.uniform(40000.0, 100000.0, n)
    t["fDelayRate_sps"][min(1, n - 1)] = 1e-30
    t["fDelayRate_sps"][n - 1] = 1e-2
    return t


CROSSING_PHASE_RATE = 3e4


def crossing(A, B, seed=0):
    """rand_table with one pair at (beam B // 2, antenna A // 2) whose phase grows with time: fPhaseRate_radps = 3e4,
    fPhase_rad = 0 -- its bound is 3e4 * fDeltaTime (+ less than 100 from the other values)."""
    t = rand_table(A * B, seed=A + B + seed)
    i = (B // 2) * A + A // 2
    t["fPhase_rad"][i] = 0.0
    t["fPhaseRate_radps"][i] = CROSSING_PHASE_RATE
    return t


def crossing_times():
    """48 fDeltaTime values, three 16-sample blocks.  Block 0: sixteen times in [0.1, 0.9] (bound 3000 .. 27000: fast, full
    degree).  Block 1: 0.95, 1.0, 1.05, 1.1, ... (bound 28500, 30000, 31500, then 33000 and beyond: the class changes inside
    the block, which therefore runs slow as a whole).  Block 2: sixteen times from 1.75 on, all slow."""
    return np.concatenate([np.linspace(0.1, 0.9, 16), 0.95 + 0.05 * np.arange(16), 1.75 + 0.05 * np.arange(16)]).astype(np.float32)


CROSSING_BLOCK_CLASSES = (FAST_HIGH, SLOW, SLOW)


def non_finite(A, B, seed=0):
    """rand_table with fDelayRate_sps = inf at (beam 1, antenna min(3, A - 1)) and fDelay_s = NaN at (beam B - 2, antenna
    A // 2); returns (table, the two beams, the NaN pair's antenna)."""
    assert B >= 4
    t = rand_table(A * B, seed=A + B + seed)
    t["fDelayRate_sps"][1 * A + min(3, A - 1)] = np.inf
    t["fDelay_s"][(B - 2) * A + A // 2] = np.nan
    return t, (1, B - 2), A // 2


def classes_of(table, dts, C):
    """pair_classes of a case, with the condition every case states: no pair at any time is unclear."""
    cls = pair_classes(table, dts, C, SAMPLING_PERIOD)
    assert not np.any(cls == UNCLEAR), f"{int(np.sum(cls == UNCLEAR))} pair(s) too close to a class boundary: change the inputs"
    return cls


def block_classes(cls):
    """The class a 16-sample block of the fused kernel runs in: the highest of its sixteen times' pairs.  cls [nt][pairs]."""
    assert cls.shape[0] % 16 == 0
    return cls.reshape(cls.shape[0] // 16, -1).max(axis=1)
