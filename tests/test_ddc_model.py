"""The numpy model of the digital down-converter (helpers/ddc_model.py; include/dcs_ddc.h), anchored
three ways: its sums on Python integers, its ``turn32`` on dc_sand_amd/csrc/bf_math.h compiled for the host (bit for bit) and
on fp64 cos / sin (within 2^-22), and the whole on the reference's ddc.py through tests/golden/ddc/ (made by
tests/golden/make_ddc_golden.py) within a tolerance computed from the fixture; then the host-side design functions of
dc_sand_amd/ddc.py.  No GPU needed."""
import ctypes
import hashlib
import json
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from helpers import ddc_model as model

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "ddc"
CASES = ("random", "centre", "dual", "bandedge", "outofband")

LAB_SOURCE = '''
#include <stddef.h>

#include "bf_math.h"
extern "C" void lab_turn32(const uint32_t *u, size_t n, float *sn, float *cs)
{
    for (size_t i = 0; i < n; i++) dcs_sincos_turn32(u[i], &sn[i], &cs[i]);
}
'''


@pytest.fixture(scope="module")
def lab(tmp_path_factory):
    """bf_math.h compiled by g++ with the flags of tests/numerics: an fp32 fma / mul / add gives the same bits on the host and
    on gfx950."""
    d = tmp_path_factory.mktemp("ddc_lab")
    (d / "lab.cpp").write_text(LAB_SOURCE)
    fma = ["-mfma"] if "fma" in Path("/proc/cpuinfo").read_text().split() else []
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", *fma, "-fPIC", "-Wall", "-Wextra", "-std=gnu++17", "-shared",
                    "-I", str(ROOT / "dc_sand_amd" / "csrc"), "-o", str(d / "liblab.so"), str(d / "lab.cpp"), "-lm"], check=True)
    L = ctypes.CDLL(str(d / "liblab.so"))
    L.lab_turn32.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.lab_turn32.restype = None
    return L


def phase_sweep():
    """A strided set of phase words and every quadrant boundary (multiples of 2^30 and the rounding points 2^29 + k 2^30)
    +- 4."""
    near = [(b + d) % (1 << 32) for b in range(0, 1 << 32, 1 << 29) for d in range(-4, 5)]
    rng = np.random.default_rng(32)
    return np.unique(np.concatenate([np.arange(0, 1 << 32, 65521, dtype=np.uint64), np.array(near, dtype=np.uint64),
                                     rng.integers(0, 1 << 32, size=4096, dtype=np.uint64)])).astype(np.uint32)


def test_turn32_is_the_header_bit_for_bit_and_within_2_to_minus_22_of_fp64(lab):
    u = phase_sweep()
    assert u.size > 65000
    sn, cs = np.empty(u.size, dtype=np.float32), np.empty(u.size, dtype=np.float32)
    lab.lab_turn32(u.ctypes.data, u.size, sn.ctypes.data, cs.ctypes.data)
    msn, mcs = model.turn32(u)
    assert model.same_bits(msn, sn) is None and model.same_bits(mcs, cs) is None
    # one rounding of r (2^-24 relative), one of the product, k's own: 3 * 2^-24 * pi / 4 < 2^-22.7 on x; the polynomials'
    # 1 ULP below 1 is 2^-24: together below 2^-22
    angle = u.astype(np.float64) * (2.0 * np.pi / 4294967296.0)
    err = max(np.abs(sn - np.sin(angle)).max(), np.abs(cs - np.cos(angle)).max())
    print("turn32: largest |error| against fp64 over", u.size, "phase words:", err, "=", err * 2.0 ** 22, "* 2^-22")
    assert err <= 2.0 ** -22
    # the cardinal points are exact: the accumulator at 0 passes the samples through
    for word, (s0, c0) in {0: (0.0, 1.0), 1 << 30: (1.0, 0.0), 1 << 31: (0.0, -1.0), 3 << 30: (-1.0, 0.0)}.items():
        s, c = model.turn32(np.array([word], dtype=np.uint32))
        assert (float(s[0]), float(c[0])) == (s0, c0)
    s, c = model.turn32(np.array([0], dtype=np.uint32))
    assert not np.signbit(s[0]) and not np.signbit(c[0])


def test_fma32_rounds_once():
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal(20000).astype(np.float32), rng.standard_normal(20000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1 + 2.0 ** -20)  # cancellation
    for cc in (c, rng.standard_normal(20000).astype(np.float32)):
        got = model.fma32(a, b, cc)
        exp = np.array([float(np.float32(float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))))) for x, y, z in
                        zip(a[:3000], b[:3000], cc[:3000])], dtype=np.float32)
        assert model.same_bits(got[:3000], exp) is None


def test_digits_hold_every_tap_up_to_8355711_and_wrap_beyond():
    v = np.array([0, 1, -1, 127, 128, -128, -129, 32767, 32768, -32768, -32769, 8355711, -8355711, 10185 << 5, -(4490 << 5)])
    for d in model.split_digits(v):
        assert d.min() >= -128 and d.max() <= 127
    assert np.array_equal(model.effective_taps(v), v)
    rng = np.random.default_rng(1)
    v = rng.integers(-model.MAX_ABS_TAP, model.MAX_ABS_TAP + 1, size=100000)
    assert np.array_equal(model.effective_taps(v), v)
    beyond = np.array([8355712, 8421503, 8421504, -8421504, -8421505, 1 << 24, (1 << 31) - 1, -(1 << 31), 12345678, -12345678])
    eff = model.effective_taps(beyond)
    assert np.array_equal(eff, ((beyond + 8421504) % (1 << 24)) - 8421504)
    assert eff[0] == -8421504 and eff[1] == -8355713 and eff[3] == -8421504 and eff[4] == 8355711 and eff[5] == 0


def test_sums_are_the_integers_modulo_2_to_32():
    rng = np.random.default_rng(2)
    T, nr_out = 128, 5
    x = rng.integers(-128, 128, size=16 * (nr_out - 1) + T, dtype=np.int8)
    for scale, wraps in ((1 << 16, False), (1 << 23, True)):
        v = rng.integers(-scale, scale + 1, size=T)
        if not wraps:
            assert np.abs(v).sum() <= model.MAX_ABS_SUM
        g = [int(t) for t in model.effective_taps(v)]
        exact = [sum(g[j] * int(x[16 * m + j]) for j in range(T)) for m in range(nr_out)]
        got = model.sums_mod32(x, v, nr_out)
        assert [int(s) for s in got] == [((e + (1 << 31)) % (1 << 32)) - (1 << 31) for e in exact]
        assert wraps == any(abs(e) >= 1 << 31 for e in exact)
    # the int32 extremes under the bound: all -128 against taps whose |g| sum to 2^24 - 1, of one sign
    v = np.full(256, 65535)
    v[0] += model.MAX_ABS_SUM - int(v.sum())
    lo = model.sums_mod32(np.full(256, -128, dtype=np.int8), v, 1)[0]
    hi = model.sums_mod32(np.full(256, -128, dtype=np.int8), -v, 1)[0]
    assert (int(lo), int(hi)) == (-128 * model.MAX_ABS_SUM, 128 * model.MAX_ABS_SUM) and 128 * model.MAX_ABS_SUM < 1 << 31


def test_zero_phase_is_the_scaled_integer_and_a_cut_series_is_one_series():
    rng = np.random.default_rng(3)
    T, nr_out = 64, 40
    x = rng.integers(-128, 128, size=(2, 16 * (nr_out - 1) + T), dtype=np.int8)
    taps = rng.integers(-3000, 3001, size=(1, T, 2))
    gain = np.float32(1.0 / 4096.0)
    y = model.ddc(x, taps, [(0, 0, gain)], nr_out)
    for i in range(2):
        for comp in range(2):
            S = model.sums_mod32(x[i], taps[0, :, comp], nr_out)
            assert model.same_bits(y[0, i, :, comp], S.astype(np.float32) * gain) is None
    band = [(0x12345679, 0xF0000001, 0.37)]
    whole = model.ddc(x, taps, band, nr_out, first_output=(1 << 32) - 7)
    for cut in (5, 16):
        a = model.ddc(x[:, :16 * (cut - 1) + T], taps, band, cut, first_output=(1 << 32) - 7)
        b = model.ddc(x[:, 16 * cut:], taps, band, nr_out - cut, first_output=(1 << 32) - 7 + cut)
        assert model.same_bits(np.concatenate([a, b], axis=2), whole) is None


@pytest.fixture(scope="module")
def golden():
    manifest = json.loads((GOLDEN / "manifest.json").read_text())
    for name, meta in manifest["files"].items():
        raw = (GOLDEN / name).read_bytes()
        assert len(raw) == meta["bytes"] <= 1 << 20 and hashlib.sha256(raw).hexdigest() == meta["sha256"], name
    taps = np.load(GOLDEN / "taps.npz")
    return manifest, taps, {name: np.load(GOLDEN / f"{name}.npz") for name in CASES}


def test_both_reference_designs_are_integers_over_2_to_17(golden):
    from dc_sand_amd import ddc

    _, taps, _ = golden
    for k, peak in (("107", 10185), ("53", 4490)):
        c, h = taps["c" + k], taps["h" + k]
        assert c.size == 256 and np.array_equal(ddc.integer_taps(c), h) and np.array_equal(h, h[::-1])
        assert np.abs(c * 131072.0 - h).max() <= 0.065 and np.abs(h).max() == peak
    assert int(taps["h107"].sum()) == 185178 and int(np.abs(taps["h107"]).sum()) == 306534


def golden_outputs(golden, name):
    """(x, reference y, model y as complex, tolerance per output, expected bins) of a case, through dc_sand_amd.ddc."""
    from dc_sand_amd import ddc

    manifest, taps, cases = golden
    x, y, step = cases[name]["x"], cases[name]["y"], int(cases[name]["phase_step"])
    assert x.dtype == np.int8 and y.dtype == np.complex128 and y.size == (x.size - 256) // 16 + 1
    assert step == 239 << 20  # cwg.py's int(N f / f_s) / (N - 1) = 239 / 4096 turns per sample
    s = manifest["scale_bits"]
    g, gain = ddc.band_taps(taps["h107"], step, s)
    got = model.as_complex(model.ddc(x[None, :], g[None], [(step, 0, gain)], y.size)[0, 0])
    tol = model.reference_tolerance(x, taps["c107"], taps["h107"], g, gain, s, y)
    return x, y, got, tol, manifest["cases"][name]


@pytest.mark.parametrize("name", CASES)
def test_model_is_the_reference_within_the_fixtures_own_bound(golden, name):
    _, y, got, tol, meta = golden_outputs(golden, name)
    diff = np.abs(got - y)
    print(name, "largest |model - reference|:", diff.max(), "tolerance there:", tol[np.argmax(diff / tol)], "max ratio:", (diff / tol).max())
    assert np.all(diff <= tol)
    assert tol.max() < 5e-3 and np.abs(y).max() > 10.0  # the bound is no licence: four decades below the signal
    assert diff.max() == pytest.approx(meta["max_abs_diff_model_vs_reference"], rel=1e-6)


def spectrum(y, fft_length):
    return np.abs(np.fft.fft(y[-fft_length:]) ** 2)  # the reference's: the last outputs, the transform squared


@pytest.mark.parametrize("name", CASES[1:])
def test_tones_land_in_their_bins_and_the_rest_is_60_db_down(golden, name):
    """The reference's own assertions, on the scenarios in which the fixture's reference output itself meets them at this
    size: centre, dual and out of band (60.3, 67.1 and 62.7 dB); the band-edge case (58.4 dB) is held element-wise only."""
    manifest, _, _ = golden
    _, y, got, _, meta = golden_outputs(golden, name)
    n, bins = manifest["fft_length"], meta["tone_bins"]
    ref = spectrum(y, n)
    ref_db = 10.0 * np.log10(ref[bins].min() / np.delete(ref, bins).max())
    assert round(ref_db, 2) == meta["reference_rejection_db"]
    meets = ref_db >= 60.0 and sorted(np.argsort(ref)[-len(bins):].tolist()) == bins
    assert meets == meta["reference_meets_60_db"] == (name != "bandedge")
    if not meets:
        return
    p = spectrum(got, n)
    assert sorted(np.argsort(p)[-len(bins):].tolist()) == bins
    db = 10.0 * np.log10(p[bins].min() / np.delete(p, bins).max())
    print(name, "rejection: model", db, "reference", ref_db)
    assert db >= 60.0 and abs(db - ref_db) < 0.1


def test_design_functions():
    from dc_sand_amd import ddc

    assert ddc.phase_step(0, 1712e6) == 0 and ddc.phase_step(428e6, 1712e6) == 1 << 30 and ddc.phase_step(-428e6, 1712e6) == 3 << 30
    assert ddc.phase_step(239, 4096) == 239 << 20 and ddc.phase_step(100e6, 1712e6) == round(Fraction(100, 1712) * (1 << 32))
    with pytest.raises(ValueError):
        ddc.integer_taps([0.5 / 131072.0, 1.0])  # residue 0.5
    assert ddc.integer_taps([3.04 / 131072.0, -7.93 / 131072.0]).tolist() == [3, -8]
    h = (np.array([1, 5, 9, 5, 1] * 13) + 1)[:64]
    g, gain = ddc.band_taps(h, 1 << 30, 4)  # a quarter turn per sample: taps h 2^4 (1, -i, -1, i, ...)
    exp = np.zeros((64, 2), dtype=np.int64)
    exp[0::4, 0], exp[1::4, 1], exp[2::4, 0], exp[3::4, 1] = 16 * h[0::4], -16 * h[1::4], -16 * h[2::4], 16 * h[3::4]
    assert g.dtype == np.int32 and np.array_equal(g, exp) and gain == 1.0 / (int(h.sum()) * 16)
    with pytest.raises(ValueError):
        ddc.band_taps(np.full(256, 66000), 0, 0)  # sum |g| = 16 896 000 > 2^24 - 1
    with pytest.raises(ValueError):
        ddc.band_taps(np.array([8355712] + [0] * 63), 0, 0)  # a tap past the digit range
    with pytest.raises(ValueError):
        ddc.band_taps(np.array([1.0, 2.0]), 0, 0)
    g, _ = ddc.band_taps(np.array([8355711] + [0] * 63), 0, 0)
    assert g[0].tolist() == [8355711, 0]
