"""The quantiser of include/dcs_beam_quant.h in numpy alone: no GPU, no library.  Per component,
y = RN(v * k_b) in fp32; NaN -> -128; otherwise clamp(rint(y), -127, 127) with ties to even; clipped when y is NaN or
|rint(y)| > 127.  tests/test_beam_quant_model.py anchors it against exact rational arithmetic; tests/test_gpu_beam_quant.py
applies it to the float call's output and compares the quantised kernels with it byte for byte."""
import numpy as np

from helpers.bacc_cases import QUANT_SHAPES as SHAPES  # noqa: F401  (the table stands with the beamformer's others)


def quantise(v, gains, beam_axis=2):
    """v: fp32 array with the beams on ``beam_axis`` (default: the beam tensor [C][nt/16][B][16][2]); gains: [B] fp32.
    Returns (int8 array of v's shape, uint64 [B] clipped components per beam)."""
    v = np.asarray(v, dtype=np.float32)
    k = np.asarray(gains, dtype=np.float32)
    shape = [1] * v.ndim
    shape[beam_axis] = k.size
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = (v * k.reshape(shape)).astype(np.float32)  # one fp32 multiply, correctly rounded
        r = np.rint(y)                                 # ties to even
        nan = np.isnan(y)
        clipped = nan | (np.abs(r) > np.float32(127.0))
        q = np.where(nan, np.float32(-128.0), np.clip(r, np.float32(-127.0), np.float32(127.0))).astype(np.int8)
    other = tuple(i for i in range(v.ndim) if i != beam_axis)
    return q, clipped.sum(axis=other).astype(np.uint64)


# ---- the gain sets of tests/test_gpu_beam_quant.py, derived from the float output alone

# The clipping gain set puts 127 at this per-beam quantile of |v_b|: about 3 % of a beam's components lie above it, so a beam
# of 128 components (the smallest here) still expects ~4 clipped ones -- inside the 0.5 % .. 20 % window with room on both
# sides whatever the distribution's tail is
CLIP_QUANTILE = 0.97


def _per_beam(v, fn):
    a = np.abs(np.asarray(v, dtype=np.float32))
    B = a.shape[2]
    return np.array([fn(np.moveaxis(a, 2, 0)[b].ravel()) for b in range(B)], dtype=np.float64)


def gains_without_clipping(v):
    """k_b = 100 / max |v_b| (1 for a beam that is all zero)."""
    m = _per_beam(v, np.max)
    return np.where(m > 0, 100.0 / np.where(m > 0, m, 1.0), 1.0).astype(np.float32)


def gains_with_clipping(v):
    """k_b = 127 / the CLIP_QUANTILE quantile of |v_b| (1 for a beam whose quantile is zero)."""
    m = _per_beam(v, lambda x: np.quantile(x.astype(np.float64), CLIP_QUANTILE))
    return np.where(m > 0, 127.0 / np.where(m > 0, m, 1.0), 1.0).astype(np.float32)


def expected_without_clipping(v):
    """(gains, int8, counts) with the asserts that keep a trivial tensor from passing: no clips, >= 100 distinct values."""
    k = gains_without_clipping(v)
    q, n = quantise(v, k)
    assert int(n.sum()) == 0, n
    assert np.unique(q).size >= 100, np.unique(q).size
    return k, q, n


def expected_with_clipping(v):
    """(gains, int8, counts) with the asserts: 0.5 % .. 20 % of all components clipped, and some in at least half the beams."""
    k = gains_with_clipping(v)
    q, n = quantise(v, k)
    share = float(n.sum()) / q.size
    assert 0.005 <= share <= 0.20, share
    assert np.count_nonzero(n) * 2 >= n.size, n
    return k, q, n


def seeded_weights(B, A, seed=11):
    """Per-input beam weights of the weighted cases: a taper in [0.25, 1] with every eighth antenna flagged (weight 0)."""
    rng = np.random.default_rng(seed + 31 * B + A)
    w = rng.uniform(0.25, 1.0, size=(B, A)).astype(np.float32)
    w[:, 3::8] = 0.0
    return w
