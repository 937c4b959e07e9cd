"""8-bit voltage beams of the complex product on the GPU (include/dcs_beam_complex_quant.h).

Every comparison is byte for byte, no tolerance.  The expectation is the numpy quantiser (helpers/beam_quant_model.py)
applied to what the complex float call returns on the same context and inputs -- which tests/test_gpu_beam_complex.py
holds to its model -- and, separately, to the model itself (helpers/beam_complex_model.py) on the generator's coefficient
bits, so the new kernels are held to the stated arithmetic without going through the float kernels.  Every quantised call
writes into an exactly sized buffer with a canary behind it, which must stay untouched."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import bacc_cases as bc
from helpers.bacc_case import T_COEFF
from helpers.beam_complex_model import complex_model
from helpers.beam_quant_model import (expected_with_clipping, expected_without_clipping, gains_with_clipping,
                                      gains_without_clipping, quantise, seeded_weights)
from helpers.beamformer_model import first_difference, normalise, weighted_coefficients
from helpers.device_buffers import closed_after
from test_gpu_beam_complex import Complex, dt_of
from test_gpu_beam_quant import QCase, same
from test_gpu_beamformer_exact import DT_COEFF, Exact

pytestmark = pytest.mark.gpu

SMALL, DEEP = bc.COMPLEX_SMALL, bc.COMPLEX_DEEP  # (the tables: helpers/bacc_cases.py)


class ExactQ(QCase, Exact):
    """The quantiser's buffers (QCase) on a case whose coefficient bits are known (Exact)."""


class CQ(Complex):
    """The complex calls on a QCase: Complex's float call into the case's float buffer, the quantised call into its int8
    buffer (exact size + canary), with its gains and counters."""

    def enqueue_q8(self, conj=False, weighted=False, count=True, dt=None, stream=None, g=None, d_gains=None, d_out=None, d_clip=None):
        c = self.c
        kw = {"t_coeff": T_COEFF} if dt is None else {"dt_coeff": float(dt)}
        clips = (c.d_clip if d_clip is None else d_clip) if count else None
        (c.g if g is None else g).beamform_accumulated_complex_q8(
            c.d_ant, c.ant.nbytes, c.d_k if d_gains is None else d_gains, c.d_q if d_out is None else d_out, c.qbytes, c.nt,
            d_weights=c.d_w if weighted else None, conjugate=conj, d_clip_count=clips, stream=stream, **kw)

    def q8(self, gains, conj=False, w=None, count=True, dt=None, zero=True):
        """One quantised call from clean buffers: (int8 beams, counters or None)."""
        c, gpu = self.c, self.c.gpu
        c.refill(c.d_q)
        gpu.memcpy_htod(c.d_k, np.ascontiguousarray(gains, dtype=np.float32))
        if zero:
            gpu.memset(c.d_clip, 0, c.B * 8)
        self._weights(w)
        self.enqueue_q8(conj, w is not None, count, dt)
        gpu.synchronize()
        return c.read_q8(), (c.counts() if count else None)

    def check(self, conj, w, dt, what):
        """Both gain sets against quantise(the complex float call's output); without counters the same bytes.  Returns the floats."""
        v = self.floats(conj, w, dt)
        assert np.all(np.isfinite(v)), what
        for expected in (expected_without_clipping, expected_with_clipping):
            k, exp, n_exp = expected(v)
            got, n = self.q8(k, conj, w, dt=dt)
            assert same(got, exp) is None, (what, expected.__name__, same(got, exp))
            assert np.array_equal(n, n_exp), (what, expected.__name__, n, n_exp)
            got0, _ = self.q8(k, conj, w, count=False, dt=dt)
            assert same(got0, exp) is None, (what, expected.__name__, "no counters", same(got0, exp))
        return v


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(QCase, gpu, oracle))


@pytest.fixture
def exactq(gpu, oracle):
    yield from closed_after(partial(ExactQ, gpu, oracle))


@pytest.fixture
def exact(gpu, oracle):
    yield from closed_after(partial(Exact, gpu, oracle))


# ---- 1. the bytes are the quantised floats of the complex float call: plain and conjugated, both entry points
@pytest.mark.parametrize("weighted", bc.weighted_of(bc.CQUANT + "test_bytes_and_counters_are_the_quantised_complex_float_output"))
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_bytes_and_counters_are_the_quantised_complex_float_output"))
def test_bytes_and_counters_are_the_quantised_complex_float_output(gpu, oracle, case, A, B, C, nt, weighted):
    x = CQ(case(A, B, C, nt))
    w = seeded_weights(B, A) if weighted else None
    for conj in (False, True):
        for dt in (None, float(DT_COEFF)):  # the index and the _dt entry points
            x.check(conj, w, dt, f"conjugate {conj}, weighted {weighted}, dt {dt}, (A, B, C, nt) = {(A, B, C, nt)}")


# ---- 2. ... and of the model on the generator's coefficient bits: the float kernels are not involved
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_bytes_are_the_quantised_model_on_the_coefficient_bits"))
def test_bytes_are_the_quantised_model_on_the_coefficient_bits(gpu, oracle, exactq, A, B, C, nt):
    x = CQ(exactq(A, B, C, nt))
    c = x.c
    w = seeded_weights(B, A)
    s, gh = normalise(w)
    by_index = SMALL.index((A, B, C, nt)) % 2 == 0  # the entry points in turn, shape by shape
    dt_arg, dt = dt_of(c, by_index)
    coef = c.coefficient_bits(dt)[0]
    for conj in (False, True):
        for wt, model in ((None, complex_model(coef, c.ant, conj)),
                          (w, complex_model(weighted_coefficients(coef, gh), c.ant, conj, scale=s))):
            assert np.all(np.isfinite(model))
            for expected in (expected_without_clipping, expected_with_clipping):
                k, exp, n_exp = expected(model)
                got, n = x.q8(k, conj, wt, dt=dt_arg)
                what = (conj, wt is not None, by_index, expected.__name__)
                assert same(got, exp) is None, (what, same(got, exp))
                assert np.array_equal(n, n_exp), (what, n, n_exp)


# ---- 3. not the element-wise form
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_not_the_element_wise_quantised_call_but_its_re_plane_without_x_im"))
def test_not_the_element_wise_quantised_call_but_its_re_plane_without_x_im(gpu, oracle, case, A, B, C, nt):
    x = CQ(case(A, B, C, nt))
    c = x.c
    k = gains_without_clipping(np.concatenate([x.floats(), c.floats()], axis=1))
    mine, _ = x.q8(k)
    theirs, _ = c.q8(k)
    assert same(mine, theirs) is not None and np.any(mine[..., 0] != theirs[..., 0]) and np.any(mine[..., 1] != theirs[..., 1])
    # x_im = 0: re = sum w_re x_re in both forms, the same floats, hence the same bytes; im = sum w_im x_re is there
    only_re = c.ant.copy()
    only_re[..., 1] = 0
    c.set_ant(only_re)
    for dt in (None, float(DT_COEFF)):
        k = gains_with_clipping(np.ascontiguousarray(c.floats(dt=dt)[..., :1]))
        mine, n_mine = x.q8(k, dt=dt)
        theirs, n_theirs = c.q8(k, dt=dt)
        assert np.all(theirs[..., 1] == 0) and np.unique(theirs[..., 0]).size >= min(100, theirs.size // 8)
        assert same(np.ascontiguousarray(mine[..., 0]), np.ascontiguousarray(theirs[..., 0])) is None, dt
        assert np.any(mine[..., 1] != 0) and n_theirs.sum() > 0 and np.all(n_mine >= n_theirs)


# ---- 4. where a wave takes several sample blocks
@pytest.mark.parametrize("weighted", bc.weighted_of(bc.CQUANT + "test_several_blocks_per_wave"))
@pytest.mark.parametrize("A,B,C,nt,depth", bc.shapes_of(bc.CQUANT + "test_several_blocks_per_wave", raw=True))
def test_several_blocks_per_wave(gpu, oracle, case, record_property, A, B, C, nt, depth, weighted):
    x = CQ(case(A, B, C, nt))
    w = seeded_weights(B, A) if weighted else None
    dt = float(DT_COEFF) if DEEP.index((A, B, C, nt, depth)) % 2 else None
    x.check(True, w, dt, f"deep, weighted {weighted}, (A, B, C, nt) = {(A, B, C, nt)}")
    record_property("gridDim.x, blockDim.x, blocks proven on some wave",
                    x.c.prove_depth(depth, lambda s: x.enqueue_q8(True, weighted, dt=dt, stream=s), kind=bc.CXQW if weighted else bc.CXQ))


# ---- 5. special gains and a NaN delay value touch their beam only
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_special_gains_and_a_nan_delay_touch_their_beam_only"))
def test_special_gains_and_a_nan_delay_touch_their_beam_only(gpu, oracle, case, A, B, C, nt):
    x = CQ(case(A, B, C, nt))
    c = x.c
    v = x.floats(True)
    k = gains_with_clipping(v)
    ref, n_ref = x.q8(k, True)
    exp, n_exp = quantise(v, k)
    assert same(ref, exp) is None and np.array_equal(n_ref, n_exp)
    per_beam = C * nt * 2
    for b, gain in ((0, 0.0), (B - 1, np.inf), (B // 2, np.nan), (1, -np.inf)):
        k2 = k.copy()
        k2[b] = gain
        got, n = x.q8(k2, True)
        exp2, n_exp2 = quantise(v, k2)
        assert same(got, exp2) is None, (b, gain, same(got, exp2))
        assert np.array_equal(n, n_exp2), (b, gain)
        others = [i for i in range(B) if i != b]
        assert np.array_equal(got[:, :, others], ref[:, :, others]) and np.array_equal(n[others], n_ref[others])
        if gain == 0.0:
            assert np.all(got[:, :, b] == 0) and n[b] == 0
        elif np.isnan(gain):
            assert np.all(got[:, :, b] == -128) and n[b] == per_beam
        else:
            assert np.all(np.isin(got[:, :, b], (-127, 127, -128))) and n[b] == per_beam
            assert np.array_equal(got[:, :, b] == -128, v[:, :, b] == 0)
    # a NaN delay value: the table is in the slow class in both runs (one finite slow pair in the last beam); the NaN pair
    # turns BOTH planes of its beam to -128, every component counted, and leaves the other beams as they were
    nb = B // 3
    t0 = c.table.copy().reshape(B, A)
    t0["fPhase_rad"][B - 1, A // 2] = 40000.0
    c.set_table(t0.ravel())
    v0 = x.floats(True)
    assert np.all(np.isfinite(v0))
    base, n_base = x.q8(k, True)
    exp0, n_exp0 = quantise(v0, k)
    assert same(base, exp0) is None and np.array_equal(n_base, n_exp0)
    t1 = t0.copy()
    t1["fDelay_s"][nb, min(3, A - 1)] = np.nan
    c.set_table(t1.ravel())
    v1 = x.floats(True)
    assert np.all(np.isnan(v1[:, :, nb])) and np.all(np.isfinite(np.delete(v1, nb, axis=2)))
    for conj in (True, False):
        got, n = x.q8(k, conj)
        assert np.all(got[:, :, nb] == -128) and n[nb] == per_beam, (conj, n[nb])
    got, n = x.q8(k, True)
    exp1, n_exp1 = quantise(v1, k)
    assert same(got, exp1) is None and np.array_equal(n, n_exp1)
    others = [i for i in range(B) if i != nb]
    assert np.array_equal(got[:, :, others], base[:, :, others]) and np.array_equal(n[others], n_base[others])


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_null_weights_equal_all_ones_weights"))
def test_null_weights_equal_all_ones_weights(gpu, oracle, case, A, B, C, nt):
    x = CQ(case(A, B, C, nt))
    k = gains_with_clipping(x.floats(True))
    plain, n_plain = x.q8(k, True)
    ones, n_ones = x.q8(k, True, np.ones((B, A), np.float32))
    assert np.array_equal(plain, ones) and np.array_equal(n_plain, n_ones) and n_plain.sum() > 0


# ---- 6. the output's alignment rule is the float call's
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_int8_beams_at_an_address_that_is_8_byte_aligned_only"))
def test_int8_beams_at_an_address_that_is_8_byte_aligned_only(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    x = CQ(case(A, B, C, nt))
    c = x.c
    k = gains_with_clipping(x.floats(True))
    ref, n_ref = x.q8(k, True)
    d_big = c.out(c.qbytes + 16)
    gpu.memset(c.d_clip, 0, B * 8)
    x.enqueue_q8(True, d_out=int(d_big) + 8)
    gpu.synchronize()
    host = c.read(d_big)
    assert np.all(host[:8] == 0xA5) and np.all(host[8 + c.qbytes:] == 0xA5)
    assert np.array_equal(host[8:8 + c.qbytes].view(np.int8).reshape(c.shape), ref) and np.array_equal(c.counts(), n_ref)
    with pytest.raises(DcsError) as e:
        x.enqueue_q8(True, d_out=int(d_big) + 4)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # one byte short
        c.g.beamform_accumulated_complex_q8(c.d_ant, c.ant.nbytes, c.d_k, int(d_big), c.qbytes - 1, nt, t_coeff=T_COEFF)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT


# ---- 7. gains are read when the work runs
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_captured_call_picks_up_new_gains_on_replay"))
def test_captured_call_picks_up_new_gains_on_replay(gpu, oracle, case, A, B, C, nt):
    x = CQ(case(A, B, C, nt))
    c = x.c
    w = seeded_weights(B, A)
    v = x.floats(True, w)
    k1, k2 = gains_with_clipping(v), gains_without_clipping(v)
    ref1, n1 = x.q8(k1, True, w)  # (also the calls the capture rule asks for first)
    ref2, n2 = x.q8(k2, True, w)
    assert n1.sum() > 0 and n2.sum() == 0 and same(ref1, ref2) is not None
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        x.enqueue_q8(True, weighted=True, stream=s.handle)
    for k, ref, n_ref in ((k1, ref1, n1), (k2, ref2, n2), (k1, ref1, n1)):
        gpu.memcpy_htod(c.d_k, k, stream=s.handle, sync=False)
        c.refill(c.d_q, stream=s.handle)
        gpu.memset(c.d_clip, 0, B * 8, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(c.read_q8(), ref) and np.array_equal(c.counts(), n_ref)
    graph.close()


# ---- 8. a context per beam slice, gains and counters offset
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.CQUANT + "test_beam_slices_reproduce_the_full_call"))
def test_beam_slices_reproduce_the_full_call(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd.beam_quant import BeamQuantGains
    from dc_sand_amd.sharding import beam_range, local_parameters, slice_table

    full = CQ(case(A, B, C, nt))
    fc = full.c
    k = gains_with_clipping(full.floats(True))
    ref, n_ref = full.q8(k, True)
    assert n_ref.sum() > 0
    qg = BeamQuantGains(fc.bp)
    for b in range(B):
        qg.set(b, k[b])
    qg.upload()
    table_ab = np.ascontiguousarray(fc.table.reshape(B, A).T).ravel()  # slice_table's [a][b] layout
    for rank in range(2):
        sh = beam_range(B, 2, rank)
        lp = local_parameters(fc.bp, sh)
        local_ab = slice_table(table_ab, fc.bp, sh).reshape(A, sh.n_beams)
        part = CQ(case(A, sh.n_beams, C, nt, table=np.ascontiguousarray(local_ab.T).ravel()))
        pc = part.c
        assert pc.bp.NR_BEAMS == lp.NR_BEAMS
        pc.set_ant(fc.ant)
        pc.refill(pc.d_q)
        part.enqueue_q8(True, d_gains=qg.device_ptr(sh.beam_lo), d_clip=qg.clip_count_ptr(sh.beam_lo))
        gpu.synchronize()
        assert np.array_equal(pc.read_q8(), ref[:, :, sh.beam_lo:sh.beam_hi]), rank
        pc.close()
    assert np.array_equal(qg.clip_counts(reset=True), n_ref)
    qg.free()


# ---- 9. the fp32 fma-chain form has no such output
def test_fp32_chain_form_is_refused_and_the_stream_stays_usable(gpu, oracle, case):
    from dc_sand_amd._lib import DCS_ERR_UNSUPPORTED, DcsError

    x = CQ(case(64, 16, 2, 32))
    c = x.c
    k = gains_with_clipping(x.floats(True))
    ref, n_ref = x.q8(k, True)
    c.g.set_tuning(math_mode=8)
    s = gpu.Stream()
    c.refill(c.d_q)
    gpu.memset(c.d_clip, 0, c.B * 8)
    gpu.memcpy_htod(c.d_w, np.ones((16, 64), np.float32))
    gpu.synchronize()
    for weighted in (False, True):
        for dt in (None, 0.0):
            for conj in (False, True):
                with pytest.raises(DcsError) as e:
                    x.enqueue_q8(conj, weighted, dt=dt, stream=s.handle)
                assert e.value.status == DCS_ERR_UNSUPPORTED
    s.synchronize()
    assert np.all(c.read(c.d_q) == 0xA5) and np.all(c.counts() == 0)  # nothing was enqueued
    c.g.set_tuning()
    x.enqueue_q8(True, stream=s.handle)  # the same stream, the default form again
    s.synchronize()
    assert np.array_equal(c.read_q8(), ref) and np.array_equal(c.counts(), n_ref)


# ---- 10. two stages: quantised sub-array beams are the antenna tensor of a second beamformer
def test_quantised_beams_are_the_samples_of_a_second_beamformer(gpu, oracle, exact, case):
    A1, B1, B2, C, nt = 64, 32, 5, 2, 32
    first = CQ(case(A1, B1, C, nt))
    v1 = first.floats(True)
    k = gains_without_clipping(v1)
    q1, n1 = first.q8(k, True)
    exp1, _ = quantise(v1, k)
    assert same(q1, exp1) is None and n1.sum() == 0 and np.unique(q1).size >= 100
    # the second stage reads the first stage's device tensor in place: [C][nt / 16][B1][16][2] is its [C][nt / 16][A][16][2]
    second = Complex(exact(B1, B2, C, nt, ant=q1))
    c2 = second.c
    assert c2.ant.shape == q1.shape and c2.ant.nbytes == first.c.qbytes
    own = c2.d_ant
    c2.d_ant = first.c.d_q
    dt_arg, dt = dt_of(c2, True)
    coef = c2.coefficient_bits(dt)[0]
    for conj in (True, False):
        got = second.floats(conj, dt=dt_arg)
        diff = first_difference(got, complex_model(coef, q1, conj))
        assert diff is None, (conj, diff)
        assert np.all(np.isfinite(got)) and np.unique(got).size >= got.size // 2
    c2.d_ant = own
