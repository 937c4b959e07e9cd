"""The Stokes detection of two polarisations' 8-bit beams on the GPU (include/dcs_stokes.h).  No
tolerance anywhere: the block Stokes parameters are compared as integers and the spectra as float bits with the numpy model
(helpers/stokes_model.py, anchored on the CPU by tests/test_stokes_model.py).  Both beam tensors are exactly sized, so their
last row ends where the allocation ends, and every output is exactly sized with a canary behind it, which must stay
untouched."""
from functools import partial

import numpy as np
import pytest

from conftest import rand_table
from helpers import filterbank_model, hip_graph
from helpers.device_buffers import Context, closed_after
from helpers.filterbank_model import same_bits  # bit for bit; two NaNs agree (their payload is the implementation's)
from helpers.integrate_cases import FORM_N, FORM_NBLK
from helpers.stokes_model import block_stokes, integrate

pytestmark = pytest.mark.gpu

BOTH = (4, 1)


def seeded_beams(B, C, nt, seed=0):
    """(x, y): full-range int8 with -128 and 127 at the first and the last byte of each."""
    rng = np.random.default_rng(1000 * B + C + seed)
    x = rng.integers(-128, 128, size=(C, nt // 16, B, 16, 2), dtype=np.int8)
    y = rng.integers(-128, 128, size=(C, nt // 16, B, 16, 2), dtype=np.int8)
    x.reshape(-1)[0], x.reshape(-1)[-1] = -128, 127
    y.reshape(-1)[0], y.reshape(-1)[-1] = 127, -128
    return x, y


def filled(shape, re, im):
    a = np.empty(shape, dtype=np.int8)
    a[..., 0], a[..., 1] = re, im
    return a


class SCase(Context):
    """One context of B beams and C channels (no delay table: the detection has no coefficients), the two beam tensors
    and the two outputs, sized for IQUV; with nr_stokes = 1 the canary begins where the smaller tensor ends."""

    def __init__(self, gpu, B, C, nt, seed=0, same_pointer=False):
        from dc_sand_amd.generator import block_stokes_bytes, quantised_beams_bytes, stokes_spectra_bytes

        super().__init__(gpu, C, B=B, NR_SAMPLES_PER_CHANNEL=nt)
        self.nt, self.nblk = nt, nt // 16
        self.x, self.y = seeded_beams(B, C, nt, seed)
        self.bbytes = quantised_beams_bytes(self.bp, nt)
        assert self.bbytes == self.x.nbytes == C * nt * B * 2
        self.d_x = self.alloc(self.bbytes)
        self.d_y = self.d_x if same_pointer else self.alloc(self.bbytes)
        self.sbytes = lambda ns: block_stokes_bytes(self.bp, nt, ns)
        self.spectra_bytes = lambda n, ns: stokes_spectra_bytes(self.bp, self.nblk, n, ns)
        assert self.sbytes(4) == C * self.nblk * B * 16 and self.sbytes(1) == C * self.nblk * B * 4
        self.d_bs = self.out(self.sbytes(4))
        self.d_s = self.out(self.sbytes(4))  # spectra: at most one per block

    def put_beams(self):
        self.gpu.memcpy_htod(self.d_x, self.x)
        if self.d_y is not self.d_x:
            self.gpu.memcpy_htod(self.d_y, self.y)

    def call_block(self, ns, stream=None):
        self.g.stokes_block(self.d_x, self.d_y, self.bbytes, self.d_bs, self.sbytes(ns), self.nt, nr_stokes=ns, stream=stream)

    def read_block(self, ns):
        return self.read(self.d_bs, self.sbytes(ns), np.int32, (self.C, self.nblk, self.B, ns))

    def block(self, ns):
        """One call from a clean output buffer."""
        self.put_beams()
        self.refill(self.d_bs)
        self.call_block(ns)
        self.gpu.synchronize()
        return self.read_block(ns)

    def set_block(self, block):
        """The integration's input given by the test."""
        ns = block.shape[-1]
        assert block.dtype == np.int32 and block.nbytes == self.sbytes(ns)
        self.refill(self.d_bs)
        self.gpu.memcpy_htod(self.d_bs, np.ascontiguousarray(block))

    def call_integrate(self, n, ns, accumulate=False, stream=None):
        self.g.integrate_stokes(self.d_bs, self.sbytes(ns), self.nblk, n, ns, self.d_s, self.spectra_bytes(n, ns),
                                accumulate=accumulate, stream=stream)

    def read_spectra(self, n, ns):
        return self.read(self.d_s, self.spectra_bytes(n, ns), np.float32, (self.nblk // n, self.C, self.B, ns))

    def spectra(self, n, ns, prior=None):
        """One integration of what d_bs holds from a clean buffer, accumulating where there is a ``prior``."""
        self.refill(self.d_s)
        if prior is not None:
            self.gpu.memcpy_htod(self.d_s, np.ascontiguousarray(prior, dtype=np.float32))
        self.call_integrate(n, ns, accumulate=prior is not None)
        self.gpu.synchronize()
        return self.read_spectra(n, ns)

    def check_block(self, what=""):
        """Both nr_stokes against the model of the case's x and y; returns the IQUV expectation."""
        exp = block_stokes(self.x, self.y, 4)
        for ns in BOTH:
            got = self.block(ns)
            want = exp[..., :ns]
            assert got.dtype == want.dtype and np.array_equal(got, want), (what, ns, np.argwhere(got != want)[:4])
        return exp


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(SCase, gpu))


@pytest.fixture
def context(gpu):
    yield from closed_after(partial(Context, gpu))


# one row; a few; exactly one wave of rows and one more; one workgroup of lanes and one more; N = 105, odd and no multiple
# of any rows-per-lane choice; many blocks
SHAPES = [(1, 1, 16), (3, 5, 48), (64, 1, 16), (65, 1, 16), (257, 1, 16), (7, 3, 80), (16, 2, 1600)]


@pytest.mark.parametrize("B,C,nt", SHAPES)
def test_block_stokes_is_the_model(gpu, case, B, C, nt):
    c = case(B, C, nt)
    exp = c.check_block()
    assert np.unique(exp).size >= min(100, exp.size), (np.unique(exp).size, exp.size)  # no trivial expectation


# The kernel's grid is capped at 2048 workgroups of 4 waves, and a wave carries 128 rows (2 per lane) per trip: 512 rows per
# workgroup, 2048 * 512 = 1048576 rows in the grid's first trip.  SHAPES have 3200 rows at the most.  B = 64, C = 8 has
# 32 nt rows, so nt = 32784 is the smallest with more: 1049088 rows of 32 bytes, 32.02 MiB per tensor; the 512 rows over
# are one workgroup's second trip.  The test reads the grid from the captured launch instead of trusting these figures: if the
# cap or the rows per lane grow, it fails and asks for a larger nt instead of testing nothing.
LOOPING_SHAPE = (64, 8, 32784)


def test_block_stokes_when_a_wave_takes_a_second_trip(gpu, case, record_property):
    B, C, nt = LOOPING_SHAPE
    c = case(B, C, nt)
    rows = C * c.nblk * B
    assert c.bbytes < 64 << 20
    exp = block_stokes(c.x, c.y, 4)
    assert np.unique(exp).size >= 100
    c.put_beams()
    for ns in BOTH:
        s = gpu.Stream()
        nodes = hip_graph.launches(s, lambda: c.call_block(ns, stream=s.handle))
        s.synchronize()
        assert len(nodes) == 1, nodes
        grid, block = nodes[0]
        assert grid[1] == grid[2] == 1 and block[1] == block[2] == 1 and block[0] % 64 == 0, nodes
        record_property(f"nr_stokes {ns}: gridDim.x, blockDim.x, rows", (grid[0], block[0], rows))
        # 2 rows per lane per trip is the kernel's; with fewer the second trip is only surer
        assert grid[0] * block[0] * 2 < rows, f"{grid[0]} workgroups of {block[0]} lanes take {rows} rows in one trip: raise nt"
        c.refill(c.d_bs)
        c.call_block(ns)
        gpu.synchronize()
        got = c.read_block(ns)
        assert np.array_equal(got, exp[..., :ns]), (ns, np.argwhere(got != exp[..., :ns])[:4])


EDGE = (3, 2, 32)


def test_all_minus_128(gpu, case):
    c = case(*EDGE)
    c.x = np.full_like(c.x, -128)
    c.y = np.full_like(c.y, -128)
    exp = c.check_block()
    assert np.all(exp == np.array([1 << 20, 0, 1 << 20, 0], dtype=np.int32))


def test_the_pair_that_makes_ci_extreme(gpu, case):
    c = case(*EDGE)
    c.x, c.y = filled(c.x.shape, -128, 127), filled(c.x.shape, 127, -128)
    exp = c.check_block()
    p = 16 * (128 * 128 + 127 * 127)
    assert np.all(exp == np.array([2 * p, 0, 2 * 16 * 2 * (-128 * 127), 2 * 16 * (127 * 127 - 128 * 128)], dtype=np.int32))
    # each product of Ci at its own extreme, the other one 0: V = +2^19 and -2^19, and -128 is negated nowhere
    c.x, c.y = filled(c.x.shape, 0, -128), filled(c.x.shape, -128, 0)
    assert np.all(c.check_block() == np.array([1 << 19, 0, 0, 1 << 19], dtype=np.int32))
    c.x, c.y = c.y, c.x
    assert np.all(c.check_block() == np.array([1 << 19, 0, 0, -(1 << 19)], dtype=np.int32))


def test_the_sign_of_v(gpu, case):
    c = case(*EDGE)
    c.x, c.y = filled(c.x.shape, 0, 1), filled(c.x.shape, 1, 0)  # x = i, y = 1: V = +2 per sample
    assert np.all(c.check_block() == np.array([32, 0, 0, 32], dtype=np.int32))


def test_both_polarisations_the_same_pointer(gpu, case):
    c = case(*EDGE, same_pointer=True)
    c.y = c.x
    exp = c.check_block()
    pxx = (c.x.astype(np.int64) ** 2).sum(axis=(3, 4))
    assert np.array_equal(exp[..., 0], 2 * pxx) and np.array_equal(exp[..., 2], 2 * pxx)
    assert not exp[..., 1].any() and not exp[..., 3].any() and np.unique(pxx).size == pxx.size


def test_one_hot_every_byte_of_a_row_is_used_once_with_its_partner(gpu, case):
    """x one-hot against y all ones, and the other way round, for each of the 32 byte positions of one row in the middle:
    the hot byte v = 3 + position shows as v^2 in I and Q, as v in U, and in V with the sign of its place ((re, im) of x:
    (-, +); of y: (+, -)); every other row stays what all ones against zeros give."""
    c = case(*EDGE)
    rows = c.C * c.nblk * c.B
    hot_row = rows // 2 + 1
    for pos in range(32):
        v = 3 + pos
        hot = np.zeros((rows, 32), dtype=np.int8)
        hot[hot_row, pos] = v
        hot = hot.reshape(c.x.shape)
        ones = np.ones_like(hot)
        sign = 1 if pos % 2 else -1  # an imaginary part of x counts +, a real part -
        for x, y, q_sign, v_sign in ((hot, ones, 1, sign), (ones, hot, -1, -sign)):
            c.x, c.y = x, y
            exp = c.check_block((pos, q_sign)).reshape(rows, 4)
            assert exp[hot_row].tolist() == [v * v + 32, q_sign * (v * v - 32), 2 * v, 2 * v_sign * v], (pos, exp[hot_row])
            others = np.delete(exp, hot_row, axis=0)
            assert np.all(others == np.array([32, -32 * q_sign, 0, 0])), pos


def planted_block(C, nblk, B, ns, seed):
    """Block values as the block call makes them (|v| <= 2^20), and planted larger ones whose sums pass 2^24 and are no
    floats, positive in I and negative in the last Stokes parameter."""
    rng = np.random.default_rng(seed)
    block = rng.integers(-(1 << 20), (1 << 20) + 1, size=(C, nblk, B, ns), dtype=np.int64).astype(np.int32)
    block[0, :, 0, 0] = (1 << 23) + 1 + np.arange(nblk) ** 2
    block[C - 1, :, B - 1, ns - 1] = -(1 << 23) - 1 - np.arange(nblk) ** 2
    return block


@pytest.mark.parametrize("ns", BOTH)
def test_integration_is_the_exact_sum_rounded_once(gpu, case, ns):
    """(B, C, nblk) = (7, 3, 12): with IQUV 1008, 504, 336 and 84 output elements for n = 1, 2, 3 and 12 -- three workgroups
    of 256 lanes and a partial fourth, one and a partial second, a partial one -- and a quarter of that with I."""
    B, C, nt = 7, 3, 192
    c = case(B, C, nt)
    block = planted_block(C, c.nblk, B, ns, seed=ns)
    c.set_block(block)
    for n in (1, 2, 3, c.nblk):
        exp = integrate(block, n)
        assert np.unique(exp).size >= min(100, exp.size)
        got = c.spectra(n, ns)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        S = block.astype(np.int64).reshape(C, c.nblk // n, n, B, ns).sum(axis=2).transpose(1, 0, 2, 3)
        if n > 1:  # sums beyond 2^24 that are no floats, of both signs: the one rounding is exercised
            inexact = (np.abs(S) > 1 << 24) & (exp.astype(np.float64) != S)
            assert (inexact & (S > 0)).any() and (inexact & (S < 0)).any()
        if ns == 4:
            assert all((S[..., s] < 0).any() for s in (1, 2, 3))  # negative Q, U and V
        # accumulate from a seeded prior that holds NaN, Inf, -Inf and -0.0
        prior = np.random.default_rng(n).uniform(-3e7, 3e7, size=exp.shape).astype(np.float32)
        prior.reshape(-1)[1:5] = [np.nan, np.inf, -np.inf, -0.0]
        want = integrate(block, n, prior=prior)
        assert np.isnan(want.ravel()[1]) and np.isinf(want.ravel()[2:4]).all()
        got = c.spectra(n, ns, prior=prior)
        assert same_bits(got, want) is None, (n, "accumulate", same_bits(got, want))
    # -0.0 + (+0.0) is +0.0: an exact sum of zero on a prior of -0.0
    zeros = np.zeros_like(block)
    c.set_block(zeros)
    prior = np.full((1, C, B, ns), -0.0, dtype=np.float32)
    got = c.spectra(c.nblk, ns, prior=prior)
    assert same_bits(got, integrate(zeros, c.nblk, prior=prior)) is None and not np.signbit(got).any()


def test_integration_takes_every_unrolled_trip_and_tail(gpu, case):
    """The int32 integrator takes a lane's n words eight to a trip: n = 1 .. 5 (a tail alone), 8 and 16 (one and two whole
    trips), 9 and 17 (a tail behind them), plain and accumulating, over full-range words of both signs
    (helpers/launch_forms.integrate_trips; tests/test_launch_forms.py)."""
    B, C, ns = 3, 2, 4
    c = case(B, C, FORM_NBLK * 16)
    block = np.random.default_rng(6).integers(-(1 << 31), 1 << 31, size=(C, FORM_NBLK, B, ns), dtype=np.int64).astype(np.int32)
    c.set_block(block)
    for n in FORM_N:
        exp = integrate(block, n)
        assert exp.shape == (FORM_NBLK // n, C, B, ns) and np.unique(exp).size >= 100
        got = c.spectra(n, ns)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        prior = np.random.default_rng(n).uniform(-3e9, 3e9, size=exp.shape).astype(np.float32)
        want = integrate(block, n, prior=prior)
        got = c.spectra(n, ns, prior=prior)
        assert same_bits(got, want) is None, (n, "accumulate", same_bits(got, want))


def test_refusals_enqueue_nothing_and_empty_calls_succeed(gpu, case):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    c = case(3, 2, 32)
    c.put_beams()
    c.refill(c.d_bs)
    c.refill(c.d_s)
    gpu.synchronize()
    g = c.g
    bad_calls = []
    for ns in BOTH:
        sb = c.sbytes(ns)
        bad_calls += [
            lambda ns=ns, sb=sb: g.stokes_block(c.d_x, c.d_y, c.bbytes - 1, c.d_bs, sb, c.nt, nr_stokes=ns),  # beams one byte short
            lambda ns=ns, sb=sb: g.stokes_block(c.d_x, c.d_y, c.bbytes, c.d_bs, sb - 1, c.nt, nr_stokes=ns),  # output one byte short
            lambda ns=ns, sb=sb: g.stokes_block(int(c.d_x) + 8, c.d_y, c.bbytes, c.d_bs, sb, c.nt, nr_stokes=ns),  # 8-byte aligned only
            lambda ns=ns, sb=sb: g.stokes_block(c.d_x, int(c.d_y) + 4, c.bbytes, c.d_bs, sb, c.nt, nr_stokes=ns),
            lambda ns=ns, sb=sb: g.stokes_block(c.d_x, c.d_y, c.bbytes, c.d_bs, sb, c.nt + 8, nr_stokes=ns),
            lambda ns=ns, sb=sb: g.integrate_stokes(c.d_bs, sb - 1, c.nblk, 1, ns, c.d_s, c.spectra_bytes(1, ns)),
            lambda ns=ns, sb=sb: g.integrate_stokes(c.d_bs, sb, c.nblk, 1, ns, c.d_s, c.spectra_bytes(1, ns) - 1),
            lambda ns=ns, sb=sb: g.integrate_stokes(c.d_bs, sb, c.nblk, 0, ns, c.d_s, c.spectra_bytes(1, ns)),
            lambda ns=ns, sb=sb: g.integrate_stokes(c.d_bs, sb, c.nblk, c.nblk + 1, ns, c.d_s, c.spectra_bytes(1, ns)),
        ]
    bad_calls += [
        lambda: g.stokes_block(c.d_x, c.d_y, c.bbytes, c.d_bs, c.sbytes(4), c.nt, nr_stokes=2),
        lambda: g.stokes_block(c.d_x, c.d_y, c.bbytes, int(c.d_bs) + 4, c.sbytes(4), c.nt, nr_stokes=4),  # IQUV wants 16 bytes
        lambda: g.integrate_stokes(c.d_bs, c.sbytes(4), c.nblk, 1, 3, c.d_s, c.spectra_bytes(1, 4)),
        lambda: g.integrate_stokes(c.d_bs, c.sbytes(4), c.nblk, 1, 4, int(c.d_s) + 8, c.spectra_bytes(1, 4)),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    # nt == 0 and nr_blocks == 0 succeed and enqueue nothing, with empty buffers too
    for ns in BOTH:
        g.stokes_block(c.d_x, c.d_y, 0, c.d_bs, 0, 0, nr_stokes=ns)
        g.integrate_stokes(c.d_bs, 0, 0, 5, ns, c.d_s, 0)
    gpu.synchronize()
    for d in (c.d_bs, c.d_s):
        assert np.all(c.read(d) == 0xA5)
    c.check_block()  # the context and the device are as usable as before


@pytest.mark.parametrize("ns", BOTH)
def test_captured_first_calls_pick_up_new_bytes_on_replay(gpu, case, ns):
    """Both calls in one hipGraph as the first calls on a fresh context -- nothing allocates, so nothing has to be run outside
    the capture first -- replayed with new bytes in the same buffers."""
    B, C, nt, n = 5, 3, 64, 2
    c = case(B, C, nt)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.call_block(ns, stream=s.handle)
        c.call_integrate(n, ns, stream=s.handle)
    pairs = [(c.x, c.y)] + [seeded_beams(B, C, nt, seed=100 + i) for i in range(2)]
    refs = [block_stokes(x, y, ns) for x, y in pairs]
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    for i in (1, 2, 0):
        gpu.memcpy_htod(c.d_x, pairs[i][0], stream=s.handle, sync=False)
        gpu.memcpy_htod(c.d_y, pairs[i][1], stream=s.handle, sync=False)
        c.refill(c.d_bs, stream=s.handle)
        c.refill(c.d_s, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(c.read_block(ns), refs[i]), i
        assert same_bits(c.read_spectra(n, ns), integrate(refs[i], n)) is None, i
    graph.close()


def test_end_to_end_from_two_antenna_tensors_to_stokes_filterbanks(gpu, context):
    """Two complex-product 8-bit beamformer calls on different antenna tensors with shared gains; the block Stokes parameters
    of the very bytes they wrote; the spectra; and the 8-bit filterbanks of the 4 B = 12 series, series 4 b + s Stokes s of
    beam b, against helpers/filterbank_model.py bit for bit."""
    from dc_sand_amd.generator import (block_stokes_bytes, filterbank_bytes, filterbank_scales_bytes, quantised_beams_bytes,
                                       spectra_sums_bytes, stokes_spectra_bytes)

    A, B, C, nt, ns, n = 8, 3, 2, 32, 4, 1
    nblk, T, NB = nt // 16, nt // 16 // n, ns * B
    c = context(C, A, B, NR_SAMPLES_PER_CHANNEL=nt)
    bp, g, read = c.bp, c.g, c.read
    g.upload_delays(rand_table(bp.n_pairs, seed=A + B))
    rng = np.random.default_rng(7)
    ants = [rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8) for _ in range(2)]
    # |sum_a w_a x_a| <= A * 128 * sqrt(2) with |w| = 1: this gain cannot clip, and spreads the beams over the int8 range
    gains = np.full(B, 127.0 / (A * 128 * 1.5), dtype=np.float32)
    d_k = c.upload(gains)
    qbytes = quantised_beams_bytes(bp, nt)
    d_ant, d_q, q = [], [], []
    for ant in ants:
        d_ant.append(c.upload(ant))
        d_q.append(c.alloc(qbytes))
        g.beamform_accumulated_complex_q8(d_ant[-1], ant.nbytes, d_k, d_q[-1], qbytes, nt, t_coeff=9)
        gpu.synchronize()
        host = np.empty((C, nblk, B, 16, 2), dtype=np.int8)
        gpu.memcpy_dtoh(host, d_q[-1])
        q.append(host)
    assert np.unique(q[0]).size >= 30 and np.unique(q[1]).size >= 30 and not np.array_equal(q[0], q[1])

    sb, pb = block_stokes_bytes(bp, nt, ns), stokes_spectra_bytes(bp, nblk, n, ns)
    ub, kb, fb = spectra_sums_bytes(bp, NB), filterbank_scales_bytes(bp, NB), filterbank_bytes(bp, NB, T)
    d_bs, d_s, d_sums, d_scales, d_fb = (c.out(x) for x in (sb, pb, ub, kb, fb))
    g.stokes_block(d_q[0], d_q[1], qbytes, d_bs, sb, nt, nr_stokes=ns)
    g.integrate_stokes(d_bs, sb, nblk, n, ns, d_s, pb)
    g.spectra_sums(d_s, pb, T, NB, d_sums, ub)
    g.filterbank_scales(d_sums, ub, T, NB, 20.0, d_scales, kb)
    g.filterbank_q8(d_s, pb, T, NB, d_scales, 128.0, d_fb, fb, T)
    gpu.synchronize()
    exp_block = block_stokes(q[0], q[1], ns)
    got_block = read(d_bs, sb, np.int32, (C, nblk, B, ns))
    assert np.array_equal(got_block, exp_block), np.argwhere(got_block != exp_block)[:4]
    assert np.unique(exp_block).size >= 24 and all((exp_block[..., s] < 0).any() for s in (1, 2, 3))
    spectra = integrate(exp_block, n).reshape(T, C, NB)
    assert same_bits(read(d_s, pb, np.float32, (T, C, NB)), spectra) is None
    sums = filterbank_model.spectra_sums(spectra)
    assert same_bits(read(d_sums, ub, np.float64, (C, NB, 2)), sums) is None
    scale = filterbank_model.scales(sums, T, 20.0)
    assert same_bits(read(d_scales, kb, np.float32, (C, NB, 2)), scale) is None
    exp_fb, _ = filterbank_model.filterbank(spectra, scale, 128.0)
    got_fb = read(d_fb, fb, np.uint8, (NB, T, C))
    assert same_bits(got_fb, exp_fb) is None and np.unique(exp_fb).size >= 2
    # series 4 b + s is Stokes s of beam b
    by_beam_and_stokes = filterbank_model.quantise(spectra.reshape(T, C * B, ns), scale.reshape(C * B, ns, 2), 128.0)[0].reshape(T, C, B, ns)
    for b in range(B):
        for s in range(ns):
            assert np.array_equal(got_fb[ns * b + s], by_beam_and_stokes[:, :, b, s]), (b, s)
