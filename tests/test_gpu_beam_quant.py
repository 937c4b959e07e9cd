"""Quantised int8 beam output on the GPU (include/dcs_beam_quant.h).  Every comparison is byte for
byte, no tolerance: the expectation is the numpy quantiser (helpers/beam_quant_model.py, anchored on the CPU by
tests/test_beam_quant_model.py) applied to what the float call returns on the same context and inputs, which
tests/test_gpu_beamformer_exact.py holds to its own arithmetic.  Every quantised call writes into an exactly sized buffer
with a canary behind it, which must stay untouched."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import bacc_cases as bc
from helpers.bacc_case import DEEP_SHAPES, DEEPEST_SHAPES, T_COEFF, Case
from helpers.beam_quant_model import (expected_with_clipping, expected_without_clipping, gains_with_clipping,
                                      gains_without_clipping, quantise, seeded_weights)
from helpers.device_buffers import closed_after

pytestmark = pytest.mark.gpu

DT_COEFF = 2.5e-6  # the _dt entry points' coefficient time


class QCase(Case):
    """Case plus the quantiser's buffers: the int8 beams (exact size + canary), the gains and the clip counters."""

    def __init__(self, gpu, oracle, A, B, C, nt, **kw):
        super().__init__(gpu, oracle, A, B, C, nt, **kw)
        self.qbytes = C * nt * B * 2
        self.d_q = self.out(self.qbytes)
        self.d_k = self.alloc(B * 4)
        self.d_clip = self.alloc(B * 8)

    def call_q8(self, weighted=False, count=True, dt=None, stream=None):
        kw = {"t_coeff": T_COEFF} if dt is None else {"dt_coeff": dt}
        self.g.beamform_accumulated_q8(self.d_ant, self.ant.nbytes, self.d_k, self.d_q, self.qbytes, self.nt,
                                       d_weights=self.d_w if weighted else None, d_clip_count=self.d_clip if count else None,
                                       stream=stream, **kw)

    def read_q8(self):
        return self.read(self.d_q, self.qbytes, np.int8, self.shape)

    def counts(self):
        n = np.empty(self.B, dtype=np.uint64)
        self.gpu.memcpy_dtoh(n, self.d_clip)
        return n

    def q8(self, gains, w=None, count=True, dt=None, zero=True):
        """One quantised call from clean buffers: (int8 beams, counters or None)."""
        gpu = self.gpu
        self.refill(self.d_q)
        gpu.memcpy_htod(self.d_k, np.ascontiguousarray(gains, dtype=np.float32))
        if zero:
            gpu.memset(self.d_clip, 0, self.B * 8)
        if w is not None:
            gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
        self.call_q8(weighted=w is not None, count=count, dt=dt)
        gpu.synchronize()
        return self.read_q8(), (self.counts() if count else None)


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(QCase, gpu, oracle))


def same(got, exp):
    """None, or where the first differing byte is."""
    bad = np.flatnonzero(got.ravel() != exp.ravel())
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{bad.size} of {got.size} bytes differ; first at {np.unravel_index(i, got.shape)}: got {got.ravel()[i]}, expected {exp.ravel()[i]}"


@pytest.mark.parametrize("weighted", bc.weighted_of(bc.QUANT + "test_quantised_output_is_the_model_of_the_float_output"))
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_quantised_output_is_the_model_of_the_float_output"))
def test_quantised_output_is_the_model_of_the_float_output(gpu, oracle, case, A, B, C, nt, weighted):
    c = case(A, B, C, nt)
    w = seeded_weights(B, A) if weighted else None
    for dt in (None, DT_COEFF):  # the index and the _dt entry points
        v = c.floats(w, dt)
        assert np.all(np.isfinite(v))
        for expected in (expected_without_clipping, expected_with_clipping):
            k, exp, n_exp = expected(v)
            got, n = c.q8(k, w, dt=dt)
            assert same(got, exp) is None, (expected.__name__, dt, same(got, exp))
            assert np.array_equal(n, n_exp), (expected.__name__, dt, n, n_exp)
            got0, _ = c.q8(k, w, count=False, dt=dt)  # no counters: the same bytes
            assert same(got0, exp) is None, (expected.__name__, dt, "no counters", same(got0, exp))


@pytest.mark.parametrize("weighted", bc.weighted_of(bc.QUANT + "test_quantised_output_with_several_blocks_per_wave"))
@pytest.mark.parametrize("A,B,C,nt,depth", bc.shapes_of(bc.QUANT + "test_quantised_output_with_several_blocks_per_wave", raw=True))
def test_quantised_output_with_several_blocks_per_wave(gpu, oracle, case, record_property, A, B, C, nt, depth, weighted):
    """The shapes above give every wave one sample block (helpers/bacc_cases.py says why); here a wave has a live second block
    in its pairs and several pairs, and its byte counters run across them.  One time form per shape, in turn.  The launch
    itself, read from a captured graph, must prove `depth` blocks on some wave and be the one helpers/launch_forms.py plans."""
    c = case(A, B, C, nt)
    w = seeded_weights(B, A) if weighted else None
    dt = DT_COEFF if DEEP_SHAPES.index((A, B, C, nt, depth)) % 2 else None
    v = c.floats(w, dt)
    assert np.all(np.isfinite(v))
    for expected in (expected_without_clipping, expected_with_clipping):
        k, exp, n_exp = expected(v)
        got, n = c.q8(k, w, dt=dt)
        assert same(got, exp) is None, (expected.__name__, dt, same(got, exp))
        assert np.array_equal(n, n_exp), (expected.__name__, dt, n, n_exp)
    got0, _ = c.q8(k, w, count=False, dt=dt)  # no counters: the same bytes
    assert same(got0, exp) is None, ("no counters", dt, same(got0, exp))
    record_property("gridDim.x, blockDim.x, blocks proven on some wave",
                    c.prove_depth(depth, lambda s: c.call_q8(weighted=weighted, dt=dt, stream=s), kind=bc.QW if weighted else bc.Q))
    if (A, B, C, nt, depth) in DEEPEST_SHAPES and not weighted:
        # a gain that clips every component: a lane's byte counters go as high as the geometry lets them (4 per pair of
        # blocks and register).  No component is 0 (asserted: the inputs are seeded), so every product is beyond 127
        assert np.all(v != 0) and np.abs(v).min() * 1e30 > 127 and np.abs(v).max() * 1e30 < np.finfo(np.float32).max
        got, n = c.q8(np.full(B, 1e30, np.float32), dt=dt)
        assert np.all(n == C * nt * 2), n
        assert np.all(np.abs(got.astype(np.int16)) == 127) and np.array_equal(got > 0, v > 0)
        # a NaN pair (the whole table in the slow class): its beam -128 and counted in every pair of blocks
        nb = B // 2
        t = c.table.copy().reshape(B, A)
        t["fDelay_s"][nb, A // 3] = np.nan
        c.set_table(t.ravel())
        v2 = c.floats(dt=dt)
        assert np.all(np.isnan(v2[:, :, nb])) and np.all(np.isfinite(np.delete(v2, nb, axis=2)))
        k = gains_with_clipping(np.delete(v2, nb, axis=2))
        k = np.insert(k, nb, np.float32(1.0))
        exp, n_exp = quantise(v2, k)
        got, n = c.q8(k, dt=dt)
        assert same(got, exp) is None, ("NaN pair", same(got, exp))
        assert np.array_equal(n, n_exp) and n[nb] == C * nt * 2 and np.all(got[:, :, nb] == -128), (n, n_exp)


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_counters_add_up_and_stay_zero_without_clipping"))
def test_counters_add_up_and_stay_zero_without_clipping(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    v = c.floats()
    k = gains_without_clipping(v)
    kc = gains_with_clipping(v)
    k[1::3] = kc[1::3]  # every third beam clips, the others cannot
    exp, n_exp = quantise(v, k)
    assert np.all(n_exp[1::3] > 0) and np.all(np.delete(n_exp, np.s_[1::3]) == 0)
    got, n = c.q8(k)
    assert same(got, exp) is None, same(got, exp)
    assert np.array_equal(n, n_exp), (n, n_exp)
    got, n = c.q8(k, zero=False)  # a second call adds to the first
    assert same(got, exp) is None and np.array_equal(n, 2 * n_exp), (n, n_exp)
    # counters that start from a value keep it
    start = (np.arange(B, dtype=np.uint64) + 1) * np.uint64(1 << 33)
    gpu.memcpy_htod(c.d_clip, start)
    got, n = c.q8(k, zero=False)
    assert np.array_equal(n, start + n_exp)


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_special_gains_weights_and_delay_values_touch_their_beam_only"))
def test_special_gains_weights_and_delay_values_touch_their_beam_only(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    w1 = seeded_weights(B, A)
    v = c.floats(w1)
    k = gains_with_clipping(v)
    ref, n_ref = c.q8(k, w1)
    exp, n_exp = quantise(v, k)
    assert same(ref, exp) is None and np.array_equal(n_ref, n_exp)
    per_beam = C * nt * 2
    for b, gain in ((0, 0.0), (B - 1, np.inf), (B // 2, np.nan), (1, -np.inf), (min(5, B - 1), -0.0)):
        k2 = k.copy()
        k2[b] = gain
        got, n = c.q8(k2, w1)
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
    # a beam whose weights are all zero is 0 whatever its gain is
    zb = B // 3
    w2 = w1.copy()
    w2[zb] = 0.0
    v2 = c.floats(w2)
    assert np.all(v2[:, :, zb] == 0)
    got, n = c.q8(k, w2)
    exp2, n_exp2 = quantise(v2, k)
    assert same(got, exp2) is None and np.array_equal(n, n_exp2)
    assert np.all(got[:, :, zb] == 0) and n[zb] == 0
    others = [i for i in range(B) if i != zb]
    assert np.array_equal(got[:, :, others], ref[:, :, others]) and np.array_equal(n[others], n_ref[others])
    # slow-class NaN pairs: the table is in the slow class in both runs (a NaN pair in beam nb0); NaN pairs in a second
    # beam turn that beam to -128, every component counted, and leave the others as they were
    nb0, nb1 = B - 1, 0
    t0 = c.table.copy().reshape(B, A)
    t0["fDelay_s"][nb0, A // 2] = np.nan
    c.set_table(t0.ravel())
    v3 = c.floats()
    assert np.all(np.isnan(v3[:, :, nb0])) and np.all(np.isfinite(np.delete(v3, nb0, axis=2)))
    base, n_base = c.q8(k)
    exp3, n_exp3 = quantise(v3, k)
    assert same(base, exp3) is None and np.array_equal(n_base, n_exp3)
    assert np.all(base[:, :, nb0] == -128) and n_base[nb0] == per_beam
    if B > 1:
        t1 = t0.copy()
        t1["fPhase_rad"][nb1, 0] = np.nan
        t1["fDelayRate_sps"][nb1, A - 1] = np.inf
        c.set_table(t1.ravel())
        v4 = c.floats()
        got, n = c.q8(k)
        exp4, n_exp4 = quantise(v4, k)
        assert same(got, exp4) is None and np.array_equal(n, n_exp4)
        assert np.all(got[:, :, nb1] == -128) and n[nb1] == per_beam
        others = [i for i in range(B) if i != nb1]
        assert np.array_equal(got[:, :, others], base[:, :, others]) and np.array_equal(n[others], n_base[others])


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_null_weights_equal_all_ones_weights"))
def test_null_weights_equal_all_ones_weights(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    k = gains_with_clipping(c.floats())
    plain, n_plain = c.q8(k)
    ones, n_ones = c.q8(k, np.ones((B, A), np.float32))
    assert np.array_equal(plain, ones) and np.array_equal(n_plain, n_ones) and n_plain.sum() > 0


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_int8_beams_at_an_address_that_is_8_byte_aligned_only"))
def test_int8_beams_at_an_address_that_is_8_byte_aligned_only(gpu, oracle, case, A, B, C, nt):
    """d_beams_q8 has the float call's rule: 8-byte alignment is enough, 4 is refused."""
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    c = case(A, B, C, nt)
    k = gains_with_clipping(c.floats())
    ref, n_ref = c.q8(k)
    d_big = c.out(c.qbytes + 16)
    gpu.memset(c.d_clip, 0, B * 8)
    c.g.beamform_accumulated_q8(c.d_ant, c.ant.nbytes, c.d_k, int(d_big) + 8, c.qbytes, nt, t_coeff=T_COEFF, d_clip_count=c.d_clip)
    gpu.synchronize()
    host = c.read(d_big)
    assert np.all(host[:8] == 0xA5) and np.all(host[8 + c.qbytes:] == 0xA5)
    assert np.array_equal(host[8:8 + c.qbytes].view(np.int8).reshape(c.shape), ref) and np.array_equal(c.counts(), n_ref)
    with pytest.raises(DcsError) as e:
        c.g.beamform_accumulated_q8(c.d_ant, c.ant.nbytes, c.d_k, int(d_big) + 4, c.qbytes, nt, t_coeff=T_COEFF)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # one byte short
        c.g.beamform_accumulated_q8(c.d_ant, c.ant.nbytes, c.d_k, int(d_big), c.qbytes - 1, nt, t_coeff=T_COEFF)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_captured_call_picks_up_new_gains_on_replay"))
def test_captured_call_picks_up_new_gains_on_replay(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    w = seeded_weights(B, A)
    v = c.floats(w)
    k1, k2 = gains_with_clipping(v), gains_without_clipping(v)
    ref1, n1 = c.q8(k1, w)  # (also the plain calls the capture rule asks for first)
    ref2, n2 = c.q8(k2, w)
    assert n1.sum() > 0 and n2.sum() == 0
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.call_q8(weighted=True, stream=s.handle)
    for k, ref, n_ref in ((k1, ref1, n1), (k2, ref2, n2), (k1, ref1, n1)):
        gpu.memcpy_htod(c.d_k, k, stream=s.handle, sync=False)
        c.refill(c.d_q, stream=s.handle)
        gpu.memset(c.d_clip, 0, B * 8, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(c.read_q8(), ref) and np.array_equal(c.counts(), n_ref)
    graph.close()


def test_fp32_chain_form_is_refused_and_the_stream_stays_usable(gpu, oracle, case):
    from dc_sand_amd._lib import DCS_ERR_UNSUPPORTED, DcsError

    c = case(64, 16, 2, 32)
    k = gains_with_clipping(c.floats())
    ref, n_ref = c.q8(k)
    c.g.set_tuning(math_mode=8)
    s = gpu.Stream()
    c.refill(c.d_q)
    gpu.memset(c.d_clip, 0, c.B * 8)
    gpu.synchronize()
    for weighted in (False, True):
        for dt in (None, 0.0):
            with pytest.raises(DcsError) as e:
                c.call_q8(weighted=weighted, dt=dt, stream=s.handle)
            assert e.value.status == DCS_ERR_UNSUPPORTED
    s.synchronize()
    assert np.all(c.read(c.d_q) == 0xA5) and np.all(c.counts() == 0)  # nothing was enqueued
    c.g.set_tuning()
    c.call_q8(stream=s.handle)  # the same stream, the default form again
    s.synchronize()
    assert np.array_equal(c.read_q8(), ref) and np.array_equal(c.counts(), n_ref)


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.QUANT + "test_beam_slices_reproduce_the_full_call"))
def test_beam_slices_reproduce_the_full_call(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd.beam_quant import BeamQuantGains
    from dc_sand_amd.sharding import beam_range, local_parameters, slice_table

    full = case(A, B, C, nt)
    v = full.floats()
    k = gains_with_clipping(v)
    ref, n_ref = full.q8(k)
    qg = BeamQuantGains(full.bp)
    for b in range(B):
        qg.set(b, k[b])
    qg.upload()
    table_ab = np.ascontiguousarray(full.table.reshape(B, A).T).ravel()  # slice_table's [a][b] layout
    for rank in range(3):
        sh = beam_range(B, 3, rank)
        lp = local_parameters(full.bp, sh)
        local_ab = slice_table(table_ab, full.bp, sh).reshape(A, sh.n_beams)
        part = case(A, sh.n_beams, C, nt, table=np.ascontiguousarray(local_ab.T).ravel())
        assert part.bp.NR_BEAMS == lp.NR_BEAMS
        part.set_ant(full.ant)
        part.refill(part.d_q)
        part.g.beamform_accumulated_q8(part.d_ant, part.ant.nbytes, qg.device_ptr(sh.beam_lo), part.d_q, part.qbytes, nt,
                                       t_coeff=T_COEFF, d_clip_count=qg.clip_count_ptr(sh.beam_lo))
        gpu.synchronize()
        assert np.array_equal(part.read_q8(), ref[:, :, sh.beam_lo:sh.beam_hi]), rank
        part.close()
    assert np.array_equal(qg.clip_counts(reset=True), n_ref)
    assert np.all(qg.clip_counts() == 0)
    qg.free()
