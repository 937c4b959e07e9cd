"""Detected beam power on the GPU (include/dcs_beam_power.h).  Every comparison is bit for bit where
the expectation is finite, NaN for NaN otherwise (payloads are not compared), no tolerance: the expectation is the numpy
model (helpers/beam_power_model.py, anchored on the CPU by tests/test_beam_power_model.py) applied to what the float call
returns on the same context and inputs, which tests/test_gpu_beamformer_exact.py holds to its own arithmetic.  Every call
writes into an exactly sized buffer with a canary behind it, which must stay untouched."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import bacc_cases as bc
from helpers.bacc_case import DEEP_SHAPES, DEEPEST_SHAPES, T_COEFF, Case
from helpers.beam_power_model import block_power, integrate, same_bits
from helpers.beam_quant_model import seeded_weights
from helpers.device_buffers import closed_after
from helpers.integrate_cases import FORM_N, FORM_NBLK

pytestmark = pytest.mark.gpu

DT_COEFF = 2.5e-6  # the _dt entry points' coefficient time
TINY = np.finfo(np.float32).tiny


class PCase(Case):
    """Case plus the detector's buffers: the block powers and the spectra (exact sizes + canaries)."""

    def __init__(self, gpu, oracle, A, B, C, nt, **kw):
        super().__init__(gpu, oracle, A, B, C, nt, **kw)
        self.nblk = nt // 16
        self.pshape = (C, self.nblk, B)
        self.pbytes = C * self.nblk * B * 4
        self.d_p = self.out(self.pbytes)
        self.d_s = self.out(self.pbytes)  # spectra: at most one per block

    def call_power(self, weighted=False, dt=None, t_coeff=T_COEFF, stream=None):
        kw = {"t_coeff": t_coeff} if dt is None else {"dt_coeff": dt}
        self.g.beamform_accumulated_power(self.d_ant, self.ant.nbytes, self.d_p, self.pbytes, self.nt,
                                          d_weights=self.d_w if weighted else None, stream=stream, **kw)

    def read_power(self):
        return self.read(self.d_p, self.pbytes, np.float32, self.pshape)

    def power(self, w=None, dt=None, t_coeff=T_COEFF):
        """One detecting call from a clean buffer."""
        gpu = self.gpu
        self.refill(self.d_p)
        if w is not None:
            gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
        self.call_power(weighted=w is not None, dt=dt, t_coeff=t_coeff)
        gpu.synchronize()
        return self.read_power()

    def sbytes(self, n):
        return (self.nblk // n) * self.C * self.B * 4

    def call_integrate(self, n, accumulate=False, stream=None):
        self.g.integrate_block_power(self.d_p, self.pbytes, self.nblk, n, self.d_s, self.sbytes(n), accumulate=accumulate,
                                     stream=stream)

    def read_spectra(self, n):
        return self.read(self.d_s, self.sbytes(n), np.float32, (self.nblk // n, self.C, self.B))

    def spectra(self, n, accumulate=False, prior=None):
        """One integration of what d_p holds; without ``accumulate`` from a clean buffer, with ``prior`` from that."""
        gpu = self.gpu
        if not accumulate:
            self.refill(self.d_s)
        if prior is not None:
            self.refill(self.d_s)
            gpu.memcpy_htod(self.d_s, np.ascontiguousarray(prior, dtype=np.float32))
        self.call_integrate(n, accumulate)
        gpu.synchronize()
        return self.read_spectra(n)


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(PCase, gpu, oracle))


@pytest.mark.parametrize("weighted", bc.weighted_of(bc.POWER + "test_block_power_is_the_model_of_the_float_output"))
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_block_power_is_the_model_of_the_float_output"))
def test_block_power_is_the_model_of_the_float_output(gpu, oracle, case, A, B, C, nt, weighted):
    c = case(A, B, C, nt)
    w = seeded_weights(B, A) if weighted else None
    for dt in (None, DT_COEFF):  # the index and the _dt entry points
        v = c.floats(w, dt)
        exp = block_power(v)
        # a trivial expectation must not pass: finite, and 100 distinct values (every value distinct where the tensor has
        # fewer than 100: four of the shapes have 12 to 96 block powers in all)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(exp)) and np.all(exp > 0)
        assert np.unique(v).size >= 100
        assert np.unique(exp).size >= min(100, exp.size), (np.unique(exp).size, exp.size)
        got = c.power(w, dt)
        assert same_bits(got, exp) is None, (dt, same_bits(got, exp))


@pytest.mark.parametrize("weighted", bc.weighted_of(bc.POWER + "test_block_power_with_several_blocks_per_wave"))
@pytest.mark.parametrize("A,B,C,nt,depth", bc.shapes_of(bc.POWER + "test_block_power_with_several_blocks_per_wave", raw=True))
def test_block_power_with_several_blocks_per_wave(gpu, oracle, case, record_property, A, B, C, nt, depth, weighted):
    """The shapes above give every wave one sample block (helpers/bacc_cases.py says why); here a wave has a live second block
    in its pairs and several pairs.  One time form per shape, in turn; then the integrator over many workgroups, every block
    its own spectrum and all blocks in one.  The launch itself, read from a captured graph, must prove `depth` blocks on
    some wave and be the one helpers/launch_forms.py plans."""
    c = case(A, B, C, nt)
    w = seeded_weights(B, A) if weighted else None
    dt = DT_COEFF if DEEP_SHAPES.index((A, B, C, nt, depth)) % 2 else None
    v = c.floats(w, dt)
    exp = block_power(v)
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(exp)) and np.all(exp > 0)
    assert np.unique(exp[::7]).size >= 100
    got = c.power(w, dt)
    assert same_bits(got, exp) is None, (dt, same_bits(got, exp))
    for n in (1, c.nblk):
        sp = c.spectra(n)
        assert same_bits(sp, integrate(got, n)) is None, (n, same_bits(sp, integrate(got, n)))
    record_property("gridDim.x, blockDim.x, blocks proven on some wave",
                    c.prove_depth(depth, lambda s: c.call_power(weighted=weighted, dt=dt, stream=s), kind=bc.PW if weighted else bc.P))
    if (A, B, C, nt, depth) in DEEPEST_SHAPES and not weighted:
        # a NaN pair (the whole table in the slow class): its beam NaN in every pair of blocks, the others the model's
        nb = B // 2
        t = c.table.copy().reshape(B, A)
        t["fDelay_s"][nb, A // 3] = np.nan
        c.set_table(t.ravel())
        v2 = c.floats(dt=dt)
        assert np.all(np.isnan(v2[:, :, nb])) and np.all(np.isfinite(np.delete(v2, nb, axis=2)))
        got = c.power(dt=dt)
        assert same_bits(got, block_power(v2)) is None, ("NaN pair", same_bits(got, block_power(v2)))
        assert np.all(np.isnan(got[:, :, nb]))


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_special_weights_and_delay_values_touch_their_beam_only"))
def test_special_weights_and_delay_values_touch_their_beam_only(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    w1 = seeded_weights(B, A)
    v = c.floats(w1)
    ref = c.power(w1)
    assert same_bits(ref, block_power(v)) is None and np.all(np.isfinite(ref))
    # a beam whose weights are all zero is 0
    zb = B // 3
    w2 = w1.copy()
    w2[zb] = 0.0
    v2 = c.floats(w2)
    assert np.all(v2[:, :, zb] == 0)
    got = c.power(w2)
    assert same_bits(got, block_power(v2)) is None, same_bits(got, block_power(v2))
    assert np.all(got[:, :, zb] == 0)
    others = [i for i in range(B) if i != zb]
    assert same_bits(got[:, :, others], ref[:, :, others]) is None
    # a non-finite weight makes its own beam NaN and leaves the others as they were
    for b, a, bad in ((0, 0, np.nan), (B - 1, A - 1, np.inf), (B // 2, A // 2, -np.inf)):
        w3 = w1.copy()
        w3[b, a] = bad
        v3 = c.floats(w3)
        assert np.all(np.isnan(v3[:, :, b]))
        got = c.power(w3)
        assert same_bits(got, block_power(v3)) is None, (b, bad, same_bits(got, block_power(v3)))
        assert np.all(np.isnan(got[:, :, b]))
        others = [i for i in range(B) if i != b]
        assert same_bits(got[:, :, others], ref[:, :, others]) is None, (b, bad)
    # slow-class NaN pairs: the table is in the slow class in both runs (a NaN pair in beam nb0); non-finite pairs in a
    # second beam turn that beam to NaN and leave the others as they were
    nb0, nb1 = B - 1, 0
    t0 = c.table.copy().reshape(B, A)
    t0["fDelay_s"][nb0, A // 2] = np.nan
    c.set_table(t0.ravel())
    v4 = c.floats()
    assert np.all(np.isnan(v4[:, :, nb0])) and np.all(np.isfinite(np.delete(v4, nb0, axis=2)))
    base = c.power()
    assert same_bits(base, block_power(v4)) is None, same_bits(base, block_power(v4))
    assert np.all(np.isnan(base[:, :, nb0])) and np.all(np.isfinite(np.delete(base, nb0, axis=2)))
    t1 = t0.copy()
    t1["fPhase_rad"][nb1, 0] = np.nan
    t1["fDelayRate_sps"][nb1, A - 1] = np.inf
    c.set_table(t1.ravel())
    v5 = c.floats()
    got = c.power()
    assert same_bits(got, block_power(v5)) is None, same_bits(got, block_power(v5))
    assert np.all(np.isnan(got[:, :, nb1]))
    others = [i for i in range(B) if i != nb1]
    assert same_bits(got[:, :, others], base[:, :, others]) is None


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_null_weights_equal_all_ones_weights"))
def test_null_weights_equal_all_ones_weights(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    plain = c.power()
    ones = c.power(np.ones((B, A), np.float32))
    assert same_bits(plain, ones) is None and np.all(np.isfinite(plain)) and np.unique(plain).size >= min(100, plain.size)
    assert same_bits(plain, block_power(c.floats())) is None


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_subnormal_squares_are_not_flushed"))
def test_subnormal_squares_are_not_flushed(gpu, oracle, case, A, B, C, nt):
    """Per-beam scales that put |v|^2 of some beams below the smallest normal number: the block powers of those beams are
    sums of subnormal numbers and still the model's."""
    c = case(A, B, C, nt)
    w = seeded_weights(B, A)
    w[0::3] *= np.float32(1e-23)  # |v| ~ 1e-20: every square subnormal
    w[1::3] *= np.float32(3e-22)  # |v| ~ 1e-19: squares on both sides of the smallest normal number
    v = c.floats(w)
    assert np.all(np.isfinite(v))
    exp = block_power(v)
    sq = (v * v).astype(np.float32)
    assert np.count_nonzero((sq > 0) & (sq < TINY)) >= 100  # subnormal squares ...
    sub = (exp > 0) & (exp < TINY)
    assert np.count_nonzero(sub) >= exp.size // 6 and np.all(sub[:, :, 0::3])  # ... and subnormal sums, all nonzero
    assert np.count_nonzero(exp >= TINY) >= exp.size // 3
    got = c.power(w)
    assert same_bits(got, exp) is None, same_bits(got, exp)


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_block_power_at_an_address_that_is_4_byte_aligned_only"))
def test_block_power_at_an_address_that_is_4_byte_aligned_only(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    c = case(A, B, C, nt)
    ref = c.power()
    assert same_bits(ref, block_power(c.floats())) is None
    d_big = c.out(c.pbytes + 16)
    c.g.beamform_accumulated_power(c.d_ant, c.ant.nbytes, int(d_big) + 4, c.pbytes, nt, t_coeff=T_COEFF)
    gpu.synchronize()
    host = c.read(d_big)
    assert np.all(host[:4] == 0xA5) and np.all(host[4 + c.pbytes:] == 0xA5)
    assert same_bits(host[4:4 + c.pbytes].view(np.float32).reshape(c.pshape), ref) is None
    # ... and integrated from there, into spectra that are 4-byte aligned only
    d_sp = c.out(c.pbytes + 16)
    c.g.integrate_block_power(int(d_big) + 4, c.pbytes, c.nblk, c.nblk, int(d_sp) + 4, c.sbytes(c.nblk))
    gpu.synchronize()
    host = c.read(d_sp)
    nb = c.sbytes(c.nblk)
    assert np.all(host[:4] == 0xA5) and np.all(host[4 + nb:] == 0xA5)
    assert same_bits(host[4:4 + nb].view(np.float32).reshape(1, C, B), integrate(ref, c.nblk)) is None
    with pytest.raises(DcsError) as e:
        c.g.beamform_accumulated_power(c.d_ant, c.ant.nbytes, int(d_big) + 2, c.pbytes, nt, t_coeff=T_COEFF)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # one byte short
        c.g.beamform_accumulated_power(c.d_ant, c.ant.nbytes, int(d_big), c.pbytes - 1, nt, t_coeff=T_COEFF)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # spectra one byte short
        c.g.integrate_block_power(int(d_big) + 4, c.pbytes, c.nblk, c.nblk, int(d_sp), nb - 1)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # block powers one byte short
        c.g.integrate_block_power(int(d_big) + 4, c.pbytes - 1, c.nblk, c.nblk, int(d_sp), nb)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_integration_is_the_ordered_sum"))
def test_integration_is_the_ordered_sum(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    c = case(A, B, C, nt)
    w = seeded_weights(B, A)
    P = c.power(w)
    assert same_bits(P, block_power(c.floats(w))) is None
    for n in (1, 2, c.nblk):
        got = c.spectra(n)
        exp = integrate(P, n)
        assert np.all(np.isfinite(exp)) and np.unique(exp).size >= min(100, exp.size)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        # accumulate: the sums start from what the spectra hold
        prior = np.random.default_rng(n).uniform(0.0, float(P.max()), size=exp.shape).astype(np.float32)
        got = c.spectra(n, accumulate=True, prior=prior)
        assert same_bits(got, integrate(P, n, prior=prior)) is None, (n, "accumulate")
    # one integration across two calls with different coefficient times: the model's running sum
    n = c.nblk
    P1 = c.power(w, t_coeff=T_COEFF)
    first = c.spectra(n)
    P2 = c.power(w, t_coeff=T_COEFF + 16)
    assert same_bits(P1, P2) is not None  # other coefficients, other powers
    both = c.spectra(n, accumulate=True)
    assert same_bits(first, integrate(P1, n)) is None
    assert same_bits(both, integrate(P2, n, prior=integrate(P1, n))) is None, same_bits(both, integrate(P2, n, prior=integrate(P1, n)))
    assert same_bits(both, integrate(np.concatenate([P1, P2], axis=1), 2 * n)) is None  # = one integration of both calls' blocks
    # a bad blocks_per_spectrum is refused, nothing is enqueued, and the stream stays usable
    s = gpu.Stream()
    c.refill(c.d_s)
    gpu.synchronize()
    for bad in (0, c.nblk + 1, 3 if c.nblk % 3 else 5):
        with pytest.raises(DcsError) as e:
            c.g.integrate_block_power(c.d_p, c.pbytes, c.nblk, bad, c.d_s, c.pbytes, stream=s.handle)
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, bad
    s.synchronize()
    assert np.all(c.read(c.d_s) == 0xA5)
    c.call_integrate(2, stream=s.handle)
    s.synchronize()
    assert same_bits(c.read_spectra(2), integrate(P2, 2)) is None


def test_integration_takes_every_unrolled_trip_and_tail_in_order(gpu, oracle, case):
    """The float integrator adds a lane's blocks in order, four to an unrolled trip: n = 1 .. 5, 8, 9, 16 and 17 give no trip,
    one and two whole trips, each with and without a tail, plain (the loop starts at the second block) and accumulating (at
    the first): helpers/launch_forms.integrate_trips; tests/test_launch_forms.py.  The block powers are given, not detected:
    magnitudes spread over nine decades, so that the sum depends on its order -- the ordered sum differs from the sum of the
    same blocks taken backwards, and from the exact sum rounded once."""
    B, C = 3, 2
    c = case(4, B, C, FORM_NBLK * 16)
    rng = np.random.default_rng(4)
    P = (rng.uniform(1.0, 2.0, size=c.pshape) * 10.0 ** rng.uniform(-3, 6, size=c.pshape)).astype(np.float32)
    gpu.memcpy_htod(c.d_p, P)
    for n in FORM_N:
        exp = integrate(P, n)
        assert exp.shape == (FORM_NBLK // n, C, B) and np.all(np.isfinite(exp)) and np.unique(exp).size >= 100
        if n > 2:
            groups = P.reshape(C, FORM_NBLK // n, n, B)
            backwards = integrate(groups[:, :, ::-1].reshape(P.shape), n)
            once = groups.astype(np.float64).sum(axis=2).transpose(1, 0, 2).astype(np.float32)
            assert same_bits(exp, backwards) is not None and same_bits(exp, once) is not None, n
        got = c.spectra(n)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        prior = (rng.uniform(1.0, 2.0, size=exp.shape) * 10.0 ** rng.uniform(-3, 6, size=exp.shape)).astype(np.float32)
        want = integrate(P, n, prior=prior)
        got = c.spectra(n, accumulate=True, prior=prior)
        assert same_bits(got, want) is None, (n, "accumulate", same_bits(got, want))
    assert same_bits(c.read_power(), P) is None  # the blocks are as they were given


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_captured_calls_pick_up_new_samples_on_replay"))
def test_captured_calls_pick_up_new_samples_on_replay(gpu, oracle, case, A, B, C, nt):
    """Both calls in one hipGraph (the process's default queue count is left as it is), replayed with new samples in the
    same buffer."""
    c = case(A, B, C, nt)
    w = seeded_weights(B, A)
    n = 2
    ants = [c.ant] + [np.random.default_rng(100 + i).integers(-128, 128, size=c.ant.shape, dtype=np.int8) for i in range(2)]
    refs = []
    for ant in ants:  # (also the plain calls the capture rule asks for first)
        c.set_ant(ant)
        P = c.power(w)
        assert same_bits(P, block_power(c.floats(w))) is None
        refs.append((P, integrate(P, n)))
    assert same_bits(refs[0][0], refs[1][0]) is not None
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.call_power(weighted=True, stream=s.handle)
        c.call_integrate(n, stream=s.handle)
    for i in (1, 2, 0, 1):
        gpu.memcpy_htod(c.d_ant, ants[i], stream=s.handle, sync=False)
        c.refill(c.d_p, stream=s.handle)
        c.refill(c.d_s, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert same_bits(c.read_power(), refs[i][0]) is None and same_bits(c.read_spectra(n), refs[i][1]) is None, i
    graph.close()


def test_fp32_chain_form_is_refused_and_the_stream_stays_usable(gpu, oracle, case):
    from dc_sand_amd._lib import DCS_ERR_UNSUPPORTED, DcsError

    c = case(64, 16, 2, 32)
    ref = c.power()
    assert same_bits(ref, block_power(c.floats())) is None
    c.g.set_tuning(math_mode=8)
    s = gpu.Stream()
    c.refill(c.d_p)
    gpu.synchronize()
    for weighted in (False, True):
        for dt in (None, 0.0):
            with pytest.raises(DcsError) as e:
                c.call_power(weighted=weighted, dt=dt, stream=s.handle)
            assert e.value.status == DCS_ERR_UNSUPPORTED
    s.synchronize()
    assert np.all(c.read(c.d_p) == 0xA5)  # nothing was enqueued
    c.g.set_tuning()
    c.call_power(stream=s.handle)  # the same stream, the default form again
    s.synchronize()
    assert same_bits(c.read_power(), ref) is None


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.POWER + "test_beam_slices_reproduce_the_full_call"))
def test_beam_slices_reproduce_the_full_call(gpu, oracle, case, A, B, C, nt):
    from dc_sand_amd.sharding import beam_range, local_parameters, slice_table

    full = case(A, B, C, nt)
    ref = full.power()
    assert same_bits(ref, block_power(full.floats())) is None
    ref_s = integrate(ref, full.nblk)
    table_ab = np.ascontiguousarray(full.table.reshape(B, A).T).ravel()  # slice_table's [a][b] layout
    for rank in range(3):
        sh = beam_range(B, 3, rank)
        lp = local_parameters(full.bp, sh)
        local_ab = slice_table(table_ab, full.bp, sh).reshape(A, sh.n_beams)
        part = case(A, sh.n_beams, C, nt, table=np.ascontiguousarray(local_ab.T).ravel())
        assert part.bp.NR_BEAMS == lp.NR_BEAMS
        part.set_ant(full.ant)
        assert same_bits(part.power(), ref[:, :, sh.beam_lo:sh.beam_hi]) is None, rank
        assert same_bits(part.spectra(part.nblk), ref_s[:, :, sh.beam_lo:sh.beam_hi]) is None, rank
        part.close()
