"""The numpy quantiser the GPU tests compare with (tests/helpers/beam_quant_model.py; include/dcs_beam_quant.h): anchored
against exact rational arithmetic on seeded values, its edge cases, and -- with the oracle's beamformer on the CPU -- that
the two gain sets tests/test_gpu_beam_quant.py derives from the float output meet their own asserts on every shape it
runs.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

from conftest import rand_table
from helpers.beam_quant_model import SHAPES, expected_with_clipping, expected_without_clipping, quantise

F32 = np.float32


def _rn32(x: Fraction) -> Fraction:
    """x rounded to the nearest fp32, ties to even, as an exact Fraction (finite, normal or subnormal range, no overflow)."""
    if x == 0:
        return Fraction(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)                      # subnormals share the smallest normal's spacing
    ulp = Fraction(2) ** (e - 23)
    n, rem = divmod(a, ulp)
    if rem * 2 > ulp or (rem * 2 == ulp and n % 2):
        n += 1
    return s * n * ulp


def _rint(x: Fraction) -> int:
    n = x.numerator // x.denominator      # floor
    rem = x - n
    if rem * 2 > 1 or (rem * 2 == 1 and n % 2):
        n += 1
    return n


def exact_quantise(v: float, k: float):
    y = _rn32(Fraction(float(v)) * Fraction(float(k)))
    assert abs(y) < Fraction(2) ** 127
    r = _rint(y)
    return max(-127, min(127, r)), abs(r) > 127


def test_model_against_exact_rational_arithmetic():
    rng = np.random.default_rng(20261017)
    n = 4000
    v = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 4, n)).astype(F32)
    k = (10.0 ** rng.uniform(-4, 3, n)).astype(F32)
    # products that land on or next to a tie: v = (j + 0.5) / k for small k a power of two, and neighbours one ulp away
    j = rng.integers(-130, 131, 600)
    kk = (2.0 ** rng.integers(-6, 7, 600)).astype(F32)
    t = ((j + 0.5) / kk).astype(F32)
    v = np.concatenate([v, t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))])
    k = np.concatenate([k, kk, kk, kk])
    for vi, ki in zip(v, k):
        q, n_clip = quantise(np.array([[[vi]]], F32), np.array([ki], F32))
        eq, eclip = exact_quantise(vi, ki)
        assert int(q[0, 0, 0]) == eq and int(n_clip[0]) == int(eclip), (vi, ki, q, eq, n_clip, eclip)


def q1(v, k):
    q, n = quantise(np.array([[[v]]], F32), np.array([k], F32))
    return int(q[0, 0, 0]), int(n[0])


def test_edge_cases():
    inf, nan = F32(np.inf), F32(np.nan)
    sub = F32(1e-45)  # the smallest subnormal
    for v, k, exp in [
        (126.5, 1, (126, 0)), (-126.5, 1, (-126, 0)),            # ties to even, inside the range
        (127.5, 1, (127, 1)), (-127.5, 1, (-127, 1)),            # rint gives +-128: clipped
        (127.49999, 1, (127, 0)), (-127.49999, 1, (-127, 0)),
        (127, 1, (127, 0)), (-127, 1, (-127, 0)), (128, 1, (127, 1)), (-128, 1, (-127, 1)),
        (0.5, 1, (0, 0)), (1.5, 1, (2, 0)), (2.5, 1, (2, 0)), (-0.5, 1, (0, 0)), (-1.5, 1, (-2, 0)),
        (0.0, 1, (0, 0)), (-0.0, 1, (0, 0)), (0.0, -3, (0, 0)),
        (sub, 1, (0, 0)), (-sub, 1, (0, 0)), (sub, 1e38, (0, 0)), (F32(1e-40), F32(1e38), (0, 0)), (F32(1e-39), F32(3e38), (0, 0)),
        (F32(1e-38), F32(3e38), (3, 0)),
        (inf, 1, (127, 1)), (-inf, 1, (-127, 1)), (inf, -1, (-127, 1)), (nan, 1, (-128, 1)), (nan, 0, (-128, 1)),
        (3e38, 3e38, (127, 1)), (-3e38, 3e38, (-127, 1)),        # the multiply overflows to +-Inf
        # gains: 0 gives zeros (and NaN from Inf), Inf gives +-127 (and NaN from 0), NaN gives -128
        (5.0, 0, (0, 0)), (-5.0, 0, (0, 0)), (inf, 0, (-128, 1)),
        (5.0, inf, (127, 1)), (-5.0, inf, (-127, 1)), (0.0, inf, (-128, 1)), (-0.0, inf, (-128, 1)), (sub, inf, (127, 1)),
        (5.0, nan, (-128, 1)), (0.0, nan, (-128, 1)),
        (1.0, -200, (-127, 1)), (1.0, -127, (-127, 0)),
    ]:
        assert q1(F32(v), F32(k)) == exp, (v, k, q1(F32(v), F32(k)), exp)


def test_minus_128_only_from_nan_and_counts_per_beam():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal((3, 2, 5, 16, 2)) * 300).astype(F32)
    v[0, 0, 1, 3, 0] = np.nan
    v[1, 1, 4, 0, 1] = -np.inf
    k = np.array([1, 0.25, 1e-3, 0, 2], F32)
    q, n = quantise(v, k)
    assert q.dtype == np.int8 and q.shape == v.shape and n.dtype == np.uint64 and n.shape == (5,)
    assert np.array_equal(q == -128, np.isnan(v * k[None, None, :, None, None]))
    assert int((q == -128).sum()) == 1 and n[2] == 0 and n[3] == 0 and n[0] > 0 and n[1] >= 1
    y = (v * k[None, None, :, None, None]).astype(F32)
    ref = np.isnan(y) | (np.abs(np.rint(y)) > 127)
    assert np.array_equal(n, ref.sum(axis=(0, 1, 3, 4)).astype(np.uint64))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("A,B,C,nt", SHAPES)
def test_gain_sets_meet_their_asserts_on_the_oracles_beams(oracle, A, B, C, nt, weighted):
    """The float output of tests/test_gpu_beam_quant.py's cases is, to a few ULP, the oracle's beamformer on the same
    table and samples (weighted: scaled per antenna): the two gain sets derived from it must pass their own asserts."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times

    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs, seed=A + B)
    ant = np.random.default_rng(A).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    dt = delta_times(bp, 9, 1)[0]
    if not weighted:
        v = oracle.beamform_accumulated(op, table, dt, nt, ant)
    else:  # per-beam, per-antenna weights: the oracle has none, so its fp32 coefficients are weighted here
        from helpers.beam_quant_model import seeded_weights

        w = seeded_weights(B, A)
        t_ab = np.ascontiguousarray(table.reshape(B, A).T).ravel()
        coef = oracle.generate_dt(op, t_ab, dt)[0].astype(np.float64)  # [c][a][b][2]
        v = np.einsum("cabk,ctaik->ctbik", coef * w.T.astype(np.float64)[None, :, :, None], ant.astype(np.float64)).astype(F32)
    expected_without_clipping(v)
    expected_with_clipping(v)
