"""The numpy model of the pulsar folder (helpers/fold_model.py) against a plain-Python loop over big integers, and the host
design functions of dc_sand_amd/fold.py: advance is exact, fold_models lies within its stated bound of the exact polynomial,
bin_of at the bin edges.  Every comparison is integer equality.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

from dc_sand_amd import fold as design
from helpers import fold_model as fm

TURN = 1 << 64


def test_model_dtype_is_the_headers_struct():
    assert design.model_dtype.itemsize == 24 and design.model_dtype.names == ("phase0", "step", "accel")
    assert [design.model_dtype.fields[n][1] for n in design.model_dtype.names] == [0, 8, 16]


MODELS = [fm.model(0, 0), fm.model(TURN - 1, 1), fm.model(TURN - 5, TURN // 7 + 3, -12345), fm.model(123, TURN // 2 + 99, 1 << 40),
          fm.model(TURN // 3, TURN // 100, -(1 << 50)), fm.model(TURN - (TURN // 3), TURN // 3 - 1, TURN - 1)]


@pytest.mark.parametrize("nbin", [1, 2, 3, 100, 1024])
def test_phases_and_bins_are_the_big_integer_ones(nbin):
    for m in MODELS:
        phi = fm.phases(m, 300)
        assert phi.dtype == np.uint64 and [int(x) for x in phi] == [fm.phase_int(m, k) for k in range(300)]
        assert fm.bins(m, 300, nbin).tolist() == [((fm.phase_int(m, k) >> 32) * nbin) >> 32 for k in range(300)]
        assert np.array_equal(design.bin_of(phi, nbin), fm.bins(m, 300, nbin))
    assert fm.phases(MODELS[2], 0).size == 0
    # far into the longest sub-integration: k (k - 1) / 2 needs 47 bits and the products wrap many times
    m = MODELS[4]
    assert [int(x) for x in fm.phases(m, 1 << 24)[-3:]] == [fm.phase_int(m, k) for k in range((1 << 24) - 3, 1 << 24)]


def test_fold_is_the_slow_fold():
    rng = np.random.default_rng(5)
    B, C, L, S, nbin, first, max_delay = 4, 5, 23, 2, 7, 3, 6
    fb = rng.integers(0, 256, size=(B, first + S * L + max_delay, C), dtype=np.uint8)
    models = np.array([[MODELS[2], MODELS[3]], [MODELS[4], MODELS[1]]], dtype=design.model_dtype)
    delays = np.array([[0, 6, 7, -1, 3], [2, 2, 0, 5, 2**31 - 1]], np.int32)
    mask = np.array([1, 1, 1, 1, 0], np.uint8)
    for kw in (dict(), dict(delays=delays, max_delay=max_delay), dict(delays=delays, max_delay=max_delay, mask=mask)):
        got = fm.fold(fb, models, first, L, nbin, beams_per_model=2, **kw)
        exp = fm.fold_slow(fb, models, first, L, nbin, beams_per_model=2, **kw)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[0].dtype == np.uint32
        assert got[1].sum(axis=-1).tolist() == [[L] * S] * 2
    both = fm.fold(fb, models, first, L, nbin, beams_per_model=2, delays=delays, max_delay=max_delay, mask=mask)[0]
    assert not both[:2, :, 2].any() and both[2:, :, 2].any() and not both[:2, :, 3].any() and not both[:, :, 4].any() and both[2:, :, 3].any()
    # placement and accumulation: only the addressed sub-integrations change
    pre_p, pre_h = np.full((B, 5, C, nbin), 0xFFFFFFF0, np.uint32), np.full((2, 5, nbin), 7, np.uint32)
    plain = fm.fold(fb, models, first, L, nbin, 2)
    p, h = fm.fold(fb, models, first, L, nbin, 2, profiles=pre_p, hits=pre_h, first_subint=2)
    assert np.array_equal(p[:, 2:4], plain[0]) and np.all(p[:, :2] == 0xFFFFFFF0) and np.all(p[:, 4] == 0xFFFFFFF0)
    assert np.array_equal(h[:, 2:4], plain[1]) and np.all(h[:, :2] == 7) and np.all(h[:, 4] == 7)
    p, h = fm.fold(fb, models, first, L, nbin, 2, profiles=pre_p, hits=pre_h, first_subint=2, accumulate=True)
    assert np.array_equal(p[:, 2:4], plain[0] + np.uint32(0xFFFFFFF0)) and np.array_equal(h[:, 2:4], plain[1] + np.uint32(7))  # modulo 2^32
    assert (plain[0] + np.uint32(0xFFFFFFF0) < plain[0]).any()
    s = fm.scrunch(plain[0], 1, 1)
    assert s.dtype == np.uint64 and np.array_equal(s[:, 1], plain[0][:, 1].astype(np.int64).sum(axis=1)) and not s[:, 0].any()


def test_advance_is_exact_at_every_cut():
    """A sub-integration cut at m and folded in two calls, the second with the advanced model and accumulate, is the one call."""
    rng = np.random.default_rng(9)
    L, C, nbin = 41, 3, 5
    fb = rng.integers(0, 256, size=(1, L, C), dtype=np.uint8)
    for m0 in MODELS[1:]:
        whole = fm.fold(fb, np.array([[m0]]), 0, L, nbin)
        for m in range(L + 1):
            adv = design.advance(m0, m)
            assert [int(x) for x in fm.phases(adv, L - m)] == [fm.phase_int(m0, m + k) for k in range(L - m)]
            if 0 < m < L:
                head = fm.fold(fb, np.array([[m0]]), 0, m, nbin)
                both = fm.fold(fb, np.array([[adv]]), m, L - m, nbin, profiles=head[0], hits=head[1], accumulate=True)
                assert np.array_equal(both[0], whole[0]) and np.array_equal(both[1], whole[1])
    assert design.advance(design.advance(MODELS[2], 1000), 2345) == design.advance(MODELS[2], 3345)


def test_fold_models_lie_within_the_bound_of_the_exact_polynomial():
    """Three members, each rounded once to the nearest 2^-64 turn: |device phase - exact phase| <= (1 + k + k (k - 1) / 2) 2^-65."""
    cases = [(641.9282333, -4.3e-14, 0.25, 64e-6, 4096, 3, 0), (1.3373, 2.0e-9, 0.999999, 1.0e-3, 100, 4, 777),
             (29.946923, -3.77535e-10, 0.0, 81.92e-6, 1 << 12, 2, 10**9), (0.5, 0.0, 0.5, 0.25, 8, 3, 1)]
    for f0, f1, phi0, dt, L, S, first in cases:
        models = design.fold_models(f0, f1, phi0, dt, L, S, first_sample=first)
        assert models.dtype == design.model_dtype and models.shape == (S,)
        F0, F1, P0, DT = Fraction(f0), Fraction(f1), Fraction(phi0), Fraction(dt)
        for s in range(S):
            for k in sorted({0, 1, 2, 3, L // 2, L - 1}):
                t = (first + s * L + k) * DT
                exact = P0 + F0 * t + F1 * t * t / 2
                got = Fraction(fm.phase_int(models[s], k), TURN)
                err = (got - exact) % 1
                err = min(err, 1 - err)
                assert err <= Fraction(1 + k + k * (k - 1) // 2, 1 << 65), (f0, s, k, float(err))
    # a negative derivative is a two's complement accel; the last case is exact: two spectra a turn
    assert int(design.fold_models(1.0, -1e-3, 0.0, 1e-3, 10, 1)[0]["accel"]) > TURN // 2
    m = design.fold_models(0.5, 0.0, 0.5, 0.25, 8, 3, 1)
    assert [(int(x["phase0"]), int(x["step"]), int(x["accel"])) for x in m] == [(TURN * 5 // 8, TURN // 8, 0), (TURN * 5 // 8, TURN // 8, 0),
                                                                              (TURN * 5 // 8, TURN // 8, 0)]
    with pytest.raises(ValueError):
        design.fold_models(1.0, 0.0, 0.0, 1e-3, 0, 1)
    with pytest.raises(ValueError):
        design.fold_models(1.0, 0.0, 0.0, 1e-3, (1 << 24) + 1, 1)


@pytest.mark.parametrize("nbin", [1, 2, 3, 100, 1024])
def test_bin_of_at_the_bin_edges(nbin):
    """Bin j holds the phases whose upper 32 bits u satisfy j 2^32 <= u nbin < (j + 1) 2^32: its first u is ceil(j 2^32 / nbin)."""
    assert design.bin_of(0, nbin) == 0 and design.bin_of(TURN - 1, nbin) == nbin - 1
    for j in range(nbin):
        u = -(-(j << 32) // nbin)
        assert design.bin_of(u << 32, nbin) == j and design.bin_of((u << 32) | 0xFFFFFFFF, nbin) == j
        if j:
            assert design.bin_of((u << 32) - 1, nbin) == j - 1
    edges = np.array([(-(-(j << 32) // nbin)) << 32 for j in range(nbin)], dtype=np.uint64)
    assert design.bin_of(edges, nbin).tolist() == list(range(nbin))
    assert design.bin_of(edges[1:] - np.uint64(1), nbin).tolist() == list(range(nbin - 1))
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            design.bin_of(0, bad)
