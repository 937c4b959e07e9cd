"""The complex-product beamformer on the GPU (include/dcs_beam_complex.h).

Bit for bit against the numpy model (helpers/beam_complex_model.py, anchored on the CPU by tests/test_beam_complex_model.py)
wherever the coefficient bits are known: they come from the GPU generator at the call's own fDeltaTime, for tables that
all_pairs_fast admits, exactly as tests/test_gpu_beamformer_exact.py takes them (its Exact class is used here).  Beside the
model, cross-checks against the existing element-wise call that fail on a sign or operand mix-up whatever the model says.
The slow class and NaN delays are held to the fp64 complex sum of the oracle's coefficients within
2.5e-7 * sum_a (|x_re| + |x_im|) + 2e-7 * |sum| per component: the GPU bound of DESIGN.md section 5.4 with both sample
components.  Every call writes into an exactly sized buffer with a canary behind it."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import bacc_cases as bc
from helpers.bacc_case import T_COEFF, Case, random_weights
from helpers.beam_complex_model import complex_model
from helpers.beam_power_model import block_power, integrate, same_bits
from helpers.beamformer_model import first_difference, normalise, weighted_coefficients
from helpers.device_buffers import CANARY, closed_after
from test_gpu_beamformer_exact import DT_COEFF, Exact
from test_gpu_class_replay import class_table

pytestmark = pytest.mark.gpu

DEEP = bc.COMPLEX_DEEP  # (the tables: helpers/bacc_cases.py)


class Complex:
    """The complex calls on a Case (or Exact): the float call into the Case's own output buffer, the detecting call into a
    block power buffer of its own (exact size + canary), which the Case frees."""

    def __init__(self, case):
        self.c = c = case
        self.nblk = c.nt // 16
        self.pshape = (c.C, self.nblk, c.B)
        self.pbytes = c.C * self.nblk * c.B * 4
        self.d_p = c.out(self.pbytes)

    def enqueue(self, conj=False, weighted=False, dt=None, t_coeff=T_COEFF, stream=None, g=None):
        c = self.c
        kw = {"t_coeff": t_coeff} if dt is None else {"dt_coeff": float(dt)}
        (c.g if g is None else g).beamform_accumulated_complex(c.d_ant, c.ant.nbytes, c.d_beams, c.nbytes, c.nt,
                                                               d_weights=c.d_w if weighted else None, conjugate=conj, stream=stream, **kw)

    def enqueue_power(self, conj=False, weighted=False, dt=None, t_coeff=T_COEFF, stream=None):
        c = self.c
        kw = {"t_coeff": t_coeff} if dt is None else {"dt_coeff": float(dt)}
        c.g.beamform_accumulated_complex_power(c.d_ant, c.ant.nbytes, self.d_p, self.pbytes, c.nt,
                                               d_weights=c.d_w if weighted else None, conjugate=conj, stream=stream, **kw)

    def _weights(self, w):
        if w is not None:
            self.c.gpu.memcpy_htod(self.c.d_w, np.ascontiguousarray(w, dtype=np.float32))

    def floats(self, conj=False, w=None, dt=None, g=None):
        c = self.c
        c.refill(c.d_beams)
        self._weights(w)
        self.enqueue(conj, w is not None, dt, g=g)
        return c.read_beams()  # (synchronises; asserts the canary)

    def power(self, conj=False, w=None, dt=None):
        gpu = self.c.gpu
        self.c.refill(self.d_p)
        self._weights(w)
        self.enqueue_power(conj, w is not None, dt)
        gpu.synchronize()
        return self.read_power()

    def read_power(self):
        return self.c.read(self.d_p, self.pbytes, np.float32, self.pshape)


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(Case, gpu, oracle))


@pytest.fixture
def exact(gpu, oracle):
    yield from closed_after(partial(Exact, gpu, oracle))


def dt_of(c, by_index):
    from dc_sand_amd.generator import delta_times

    return None if by_index else DT_COEFF, (delta_times(c.bp, T_COEFF, 1)[0] if by_index else DT_COEFF)


def check_model(x, coef, conj, w=None, dt=None, what=""):
    """One complex float call against the model of the coefficient bits ``coef``; returns the call's output."""
    c = x.c
    if w is None:
        exp = complex_model(coef, c.ant, conj)
    else:
        s, gh = normalise(w)
        exp = complex_model(weighted_coefficients(coef, gh), c.ant, conj, scale=s)
    got = x.floats(conj, w, dt)
    diff = first_difference(got, exp) if np.all(np.isfinite(exp)) else same_bits(got, exp)
    assert diff is None, f"{what}, conjugate {conj}, dt {dt}, (A, B, C, nt) = {(c.A, c.B, c.C, c.nt)}: {diff}"
    return got


# ---- bit for bit: plain and conjugated, the index entry point and the _dt one
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_complex_product_is_the_model_bit_for_bit"))
def test_complex_product_is_the_model_bit_for_bit(gpu, oracle, exact, A, B, C, nt):
    x = Complex(exact(A, B, C, nt))
    plain = x.c.floats()
    for by_index in (True, False):
        dt_arg, dt = dt_of(x.c, by_index)
        coef = x.c.coefficient_bits(dt)[0]
        v = check_model(x, coef, False, dt=dt_arg, what="unweighted")
        vc = check_model(x, coef, True, dt=dt_arg, what="unweighted")
        assert np.all(np.isfinite(v)) and np.unique(v).size >= min(100, v.size // 2)
        # not the element-wise product, and the conjugate is another number in both planes
        assert first_difference(v, plain) is not None and np.any(v[..., 0] != vc[..., 0]) and np.any(v[..., 1] != vc[..., 1])


# ---- cross-checks against the existing call: no model involved
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_one_sample_component_at_a_time_gives_the_planes_of_the_element_wise_call"))
def test_one_sample_component_at_a_time_gives_the_planes_of_the_element_wise_call(gpu, oracle, case, A, B, C, nt):
    """x_im = 0: re = sum w_re x_re, the plain call's re plane.  x_re = 0, conjugated: re = sum w_im x_im, the plain call's
    im plane (the operand is fixed(-sigma w_im) = fixed(w_im): the same digits).  Bit for bit, both entry points."""
    x = Complex(case(A, B, C, nt))
    c = x.c
    ant = c.ant.copy()
    only_re, only_im = ant.copy(), ant.copy()
    only_re[..., 1] = 0
    only_im[..., 0] = 0
    for dt in (None, float(DT_COEFF)):
        c.set_ant(only_re)
        plain = c.floats(dt=dt)
        assert np.all(plain[..., 1] == 0) and np.unique(plain[..., 0]).size >= min(100, plain.size // 4)
        got = x.floats(False, dt=dt)
        assert first_difference(np.ascontiguousarray(got[..., 0]), np.ascontiguousarray(plain[..., 0])) is None, ("x_im = 0", dt)
        assert np.any(got[..., 1] != 0)  # im = sum w_im x_re is there
        c.set_ant(only_im)
        plain = c.floats(dt=dt)
        assert np.all(plain[..., 0] == 0) and np.unique(plain[..., 1]).size >= min(100, plain.size // 4)
        got = x.floats(True, dt=dt)
        assert first_difference(np.ascontiguousarray(got[..., 0]), np.ascontiguousarray(plain[..., 1])) is None, ("x_re = 0, conjugated", dt)
        # ... and unconjugated it is that plane negated: the same integer, negated, in other digits -- so the tail's roundings
        # (six of 2^-24 relative between the two, and the low parts' 2^31 * 2^-24 / 8355711 = 1.5e-5 each) may differ
        neg = x.floats(False, dt=dt)
        assert np.allclose(neg[..., 0], -plain[..., 1], rtol=1e-6, atol=1e-3)


# ---- weights
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_weights"))
def test_weights(gpu, oracle, exact, A, B, C, nt):
    x = Complex(exact(A, B, C, nt))
    dt_arg, dt = dt_of(x.c, True)
    coef = x.c.coefficient_bits(dt)[0]
    for conj in (False, True):
        ref = x.floats(conj)
        ones = x.floats(conj, np.ones((B, A), np.float32))
        assert first_difference(ones, ref) is None, ("all-ones weights", conj)
    w = random_weights(np.random.default_rng(A + 7 * B), B, A, zero_beam=True)
    zb = int(np.flatnonzero(~w.any(axis=1))[0])
    got = check_model(x, coef, True, w=w, what="random weights")
    assert np.all(got[:, :, zb] == 0) and np.all(np.isfinite(got))
    check_model(x, coef, False, w=w, what="random weights")
    # a NaN weight: NaN in both planes of its beam, the other beams as they were
    nb = (zb + 1) % B
    w2 = w.copy()
    w2[nb, A // 2] = np.nan
    bad = check_model(x, coef, True, w=w2, what="a NaN weight")
    assert np.all(np.isnan(bad[:, :, nb]))
    others = [b for b in range(B) if b != nb]
    assert first_difference(np.ascontiguousarray(bad[:, :, others]), np.ascontiguousarray(got[:, :, others])) is None


# ---- the slow class and NaN delays: against the fp64 complex sum of the oracle's coefficients
def fp64_complex_sum(coef, ant, conj):
    """coef fp32 [C][A][B][2] (NaN allowed), ant int8 [C][T][A][16][2] -> float64 [C][T][B][16][2] and
    sum_a (|x_re| + |x_im|) [C][T][16]."""
    w = coef[..., 0].astype(np.float64) + 1j * coef[..., 1].astype(np.float64)
    if conj:
        w = np.conj(w)
    xs = ant[..., 0].astype(np.float64) + 1j * ant[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.einsum("cab,ctai->ctbi", w, xs)
    mag = np.abs(ant.astype(np.float64)).sum(axis=(2, 4))
    return np.stack([s.real, s.imag], axis=-1), mag


def within_fp64_bound(got, coef, ant, conj, nan_beams, what):
    exp, mag = fp64_complex_sum(coef, ant, conj)
    B = got.shape[2]
    for b in range(B):
        if b in nan_beams:
            assert np.all(np.isnan(got[:, :, b])), (what, "beam", b, "must be NaN in both planes")
            continue
        assert np.all(np.isfinite(exp[:, :, b])), (what, b)
        err = np.abs(got[:, :, b].astype(np.float64) - exp[:, :, b])
        bound = 2.5e-7 * mag[..., None] + 2e-7 * np.abs(exp[:, :, b])
        i = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        assert np.all(err <= bound), f"{what}, beam {b}: |got - fp64| {err[i]:.3e} over the bound {bound[i]:.3e} at {i}"
    print(f"{what}: max |got - fp64| / sum|x| = {np.nanmax(np.abs(got - exp) / mag[:, :, None, :, None]):.3e}")


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_slow_class_and_nan_delays_against_the_fp64_sum"))
def test_slow_class_and_nan_delays_against_the_fp64_sum(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd.generator import delta_times

    x = Complex(case(A, B, C, nt))
    c = x.c
    dt = delta_times(c.bp, T_COEFF, 1)
    base = c.table.copy()
    # one slow-class pair (finite): the whole table takes the slow path
    slow = base.copy().reshape(B, A)
    slow["fPhase_rad"][3, A // 2] = 40000.0
    c.set_table(slow.ravel())
    coef = c.coefficients(dt)[0]
    assert np.all(np.isfinite(coef))
    for conj in (False, True):
        within_fp64_bound(x.floats(conj), coef, c.ant, conj, (), f"one slow pair, conjugate {conj}")
    # one NaN delay: both planes of exactly that beam's rows are NaN
    nan = base.copy().reshape(B, A)
    nan["fDelay_s"][2, min(3, A - 1)] = np.nan
    c.set_table(nan.ravel())
    coef = c.coefficients(dt)[0]
    assert np.isnan(coef[:, min(3, A - 1), 2]).any() and np.all(np.isfinite(np.delete(coef, 2, axis=2)))
    for conj in (False, True):
        got = x.floats(conj)
        within_fp64_bound(got, coef, c.ant, conj, (2,), f"one NaN delay, conjugate {conj}")
        assert np.all(np.isfinite(np.delete(got, 2, axis=2)))
        p = x.power(conj)
        assert same_bits(p, block_power(got)) is None and np.all(np.isnan(p[:, :, 2]))


# ---- where a wave takes several sample blocks
@pytest.mark.parametrize("A,B,C,nt,depth", bc.shapes_of(bc.COMPLEX + "test_several_blocks_per_wave_bit_for_bit", raw=True))
def test_several_blocks_per_wave_bit_for_bit(gpu, oracle, exact, record_property, A, B, C, nt, depth):
    """The float call plain and conjugated, and conjugated with weights, against the model; the detecting call without and
    with weights against block_power of those floats.  Every launch, read from a captured graph, must prove `depth` blocks
    on some wave and be the one helpers/launch_forms.py plans (nine coefficient operands: other LDS bytes than the
    element-wise call's)."""
    x = Complex(exact(A, B, C, nt))
    dt_arg, dt = dt_of(x.c, DEEP.index((A, B, C, nt, depth)) % 2 == 0)
    coef = x.c.coefficient_bits(dt)[0]
    check_model(x, coef, False, dt=dt_arg, what="deep")
    v = check_model(x, coef, True, dt=dt_arg, what="deep")
    record_property("gridDim.x, blockDim.x, blocks proven on some wave",
                    x.c.prove_depth(depth, lambda s: x.enqueue(True, dt=dt_arg, stream=s), kind=bc.CX))
    p = x.power(True, dt=dt_arg)  # the detected form, and its launch
    assert same_bits(p, block_power(v)) is None, same_bits(p, block_power(v))
    x.c.prove_depth(depth, lambda s: x.enqueue_power(True, dt=dt_arg, stream=s), kind=bc.CXP)
    w = random_weights(np.random.default_rng(A + 7 * B), B, A, zero_beam=False)
    vw = check_model(x, coef, True, w=w, dt=dt_arg, what="deep, weighted")
    x.c.prove_depth(depth, lambda s: x.enqueue(True, weighted=True, dt=dt_arg, stream=s), kind=bc.CXW)
    p = x.power(True, w, dt=dt_arg)
    assert np.all(np.isfinite(p)) and same_bits(p, block_power(vw)) is None, same_bits(p, block_power(vw))
    x.c.prove_depth(depth, lambda s: x.enqueue_power(True, weighted=True, dt=dt_arg, stream=s), kind=bc.CXPW)


# ---- the detected form
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_block_power_is_the_model_of_the_complex_float_output"))
def test_block_power_is_the_model_of_the_complex_float_output(gpu, oracle, case, A, B, C, nt):
    x = Complex(case(A, B, C, nt))
    w = random_weights(np.random.default_rng(3 * A + B), B, A, zero_beam=False)
    for conj, wt, dt in ((False, None, None), (True, None, float(DT_COEFF)), (True, w, None), (False, w, float(DT_COEFF))):
        v = x.floats(conj, wt, dt)
        exp = block_power(v)
        assert np.all(np.isfinite(exp)) and np.all(exp > 0) and np.unique(exp).size >= min(100, exp.size)
        got = x.power(conj, wt, dt)
        assert same_bits(got, exp) is None, (conj, wt is not None, dt, same_bits(got, exp))
    # it is not the element-wise call's power
    assert same_bits(x.power(), block_power(x.c.floats())) is not None


def test_complex_block_power_feeds_the_integration_and_the_filterbanks(gpu, oracle, case):
    """complex_power -> integrate_block_power -> spectra_sums -> filterbank_scales -> filterbank_q8, each step the model of
    the step before (helpers/beam_power_model.py, helpers/filterbank_model.py)."""
    from dc_sand_amd.generator import filterbank_bytes, filterbank_scales_bytes, power_spectra_bytes, spectra_sums_bytes
    from helpers import filterbank_model as fm

    A, B, C, nt, n = 64, 16, 5, 256, 2
    x = Complex(case(A, B, C, nt))
    c, g = x.c, x.c.g
    P = x.power(True)
    assert same_bits(P, block_power(x.floats(True))) is None
    T = x.nblk // n
    sizes = {"sp": power_spectra_bytes(c.bp, x.nblk, n), "sums": spectra_sums_bytes(c.bp, B), "sc": filterbank_scales_bytes(c.bp, B),
             "fb": filterbank_bytes(c.bp, B, T)}
    d = {k: c.out(v) for k, v in sizes.items()}
    g.integrate_block_power(x.d_p, x.pbytes, x.nblk, n, d["sp"], sizes["sp"])
    g.spectra_sums(d["sp"], sizes["sp"], T, B, d["sums"], sizes["sums"])
    g.filterbank_scales(d["sums"], sizes["sums"], T, B, 24.0, d["sc"], sizes["sc"])
    g.filterbank_q8(d["sp"], sizes["sp"], T, B, d["sc"], 128.0, d["fb"], sizes["fb"], T)
    gpu.synchronize()

    def read(k, dtype, shape):
        return c.read(d[k], sizes[k], dtype, shape)

    sp = read("sp", np.float32, (T, C, B))
    assert same_bits(sp, integrate(P, n)) is None
    sums = read("sums", np.float64, (C, B, 2))
    assert fm.same_bits(sums, fm.spectra_sums(sp)) is None
    sc = read("sc", np.float32, (C, B, 2))
    assert fm.same_bits(sc, fm.scales(sums, T, 24.0)) is None and np.all(sc[..., 1] > 0)
    fb = read("fb", np.uint8, (B, T, C))
    exp, _ = fm.filterbank(sp, sc, 128.0)
    assert np.array_equal(fb, exp) and np.unique(fb).size > 20


def test_fp32_chain_form_is_refused_and_writes_nothing(gpu, oracle, case):
    from dc_sand_amd._lib import DCS_ERR_UNSUPPORTED, DcsError

    x = Complex(case(64, 16, 2, 32))
    c = x.c
    ref = x.floats(True)
    c.g.set_tuning(math_mode=8)
    c.refill(c.d_beams)
    c.refill(x.d_p)
    gpu.memcpy_htod(c.d_w, np.ones((16, 64), np.float32))
    for call in (x.enqueue, x.enqueue_power):
        for weighted in (False, True):
            for dt in (None, 0.0):
                with pytest.raises(DcsError) as e:
                    call(True, weighted, dt)
                assert e.value.status == DCS_ERR_UNSUPPORTED
    gpu.synchronize()
    assert np.all(c.read_beams().view(np.uint32) == 0xFFFFFFFF) and np.all(x.read_power().view(np.uint32) == 0xA5A5A5A5)
    c.g.set_tuning()
    assert first_difference(x.floats(True), ref) is None


# ---- graph replay (tests/test_gpu_class_replay.py's scheme): a table with one full-degree pair
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_captured_complex_call_replayed_after_a_younger_plain_call"))
def test_captured_complex_call_replayed_after_a_younger_plain_call(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd._lib import DCS_ERR_UNSUPPORTED, DcsError
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    table, low, where = class_table(A, B, "high")
    x = Complex(case(A, B, C, nt, table=table))
    c = x.c
    s = gpu.Stream()
    # a first call under capture allocates: refused, and the capture can still be ended
    with hip_graph.capture(s) as refused:
        for call in (x.enqueue, x.enqueue_power):
            with pytest.raises(DcsError) as e:
                call(True, stream=s.handle)
            assert e.value.status == DCS_ERR_UNSUPPORTED
        gpu.memset(c.d_beams, 0xFF, CANARY, stream=s.handle)  # the capture is still alive: this is recorded
    refused.close()
    # what a fresh context gives, per sample set
    ants = [c.ant] + [np.random.default_rng(50 + i).integers(-128, 128, size=c.ant.shape, dtype=np.int8) for i in range(2)]
    fresh = []
    for ant in ants:
        c.set_ant(ant)
        g = SteeringCoefficientGenerator(c.bp)
        g.upload_delays(table)
        fresh.append(x.floats(True, g=g))
        g.close()
    assert first_difference(fresh[0], fresh[1]) is not None
    # the full-degree pair's beam differs from the all-low table's
    c.set_table(low)
    lowv = x.floats(True)  # (also the first call outside the capture)
    hb = where["high"][0]
    assert np.any(lowv[:, :, hb] != fresh[2][:, :, hb])
    c.set_table(table)
    with hip_graph.capture(s) as graph:
        x.enqueue(True, stream=s.handle)
    for i in (1, 0, 2):
        gpu.memcpy_htod(c.d_ant, ants[i])
        c.ant = ants[i]
        c.floats()  # a younger plain float call on the same context
        c.refill(c.d_beams)
        gpu.synchronize()
        graph.launch(s)
        s.synchronize()
        got = c.read_beams()
        assert first_difference(got, fresh[i]) is None, (i, first_difference(got, fresh[i]))
    graph.close()


# ---- physics: a beam steered at the source it was made for
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.COMPLEX + "test_a_conjugate_beam_on_its_own_source_adds_coherently"))
def test_a_conjugate_beam_on_its_own_source_adds_coherently(gpu, oracle, case, A, B, C, nt):
    """x_a(t) = rint(100 * w_{a, b0}) per component: conj(w) x = 100 |w|^2 = 100 per antenna up to the rounding of the
    sample, at most 0.5 per component -- magnitude sqrt(0.5) after the unit-modulus rotation -- so beam b0 is within
    0.7072 * A + 1e-3 of (100 * A, 0) in each component; the beamformer's own error is orders below that."""
    from dc_sand_amd.generator import delta_times

    x = Complex(case(A, B, C, nt))
    c = x.c
    b0 = B // 3
    coef = c.coefficients(delta_times(c.bp, T_COEFF, 1))[0]  # [c][a][b][2]
    assert np.all(np.isfinite(coef))
    src = np.rint(100.0 * coef[:, :, b0, :].astype(np.float64)).astype(np.int8)  # [c][a][2]
    c.set_ant(np.ascontiguousarray(np.broadcast_to(src[:, None, :, None, :], c.ant.shape)))
    v = x.floats(True)
    tol = 0.7072 * A + 1e-3
    assert np.all(np.abs(v[:, :, b0, :, 0] - 100.0 * A) <= tol), np.abs(v[:, :, b0, :, 0] - 100.0 * A).max()
    assert np.all(np.abs(v[:, :, b0, :, 1]) <= tol), np.abs(v[:, :, b0, :, 1]).max()
    # the other beams do not point there, and the element-wise call has no such peak
    others = np.delete(np.hypot(v[..., 0], v[..., 1]), b0, axis=2)
    assert np.median(others) < 0.5 * 100.0 * A
    p = x.power(True)
    assert np.all(p[:, :, b0] > 4 * np.delete(p, b0, axis=2).mean())
    e = c.floats()
    assert np.all(np.hypot(e[:, :, b0, :, 0], e[:, :, b0, :, 1]) < 0.9 * 100.0 * A)
