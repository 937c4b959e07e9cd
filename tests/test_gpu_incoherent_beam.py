"""The incoherent beam on the GPU (include/dcs_incoherent_beam.h).  No tolerance anywhere: the block
powers are compared as integers and the spectra as float bits with the numpy model (helpers/incoherent_model.py, anchored
on the CPU by tests/test_incoherent_model.py).  The sample buffer is exactly sized, so its last row ends where the
allocation ends, and every output is exactly sized with a canary behind it, which must stay untouched."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import stokes_model
from helpers.device_buffers import Context, closed_after
from helpers.incoherent_cases import FORM_LOOPING_SHAPES, FORM_SHAPES, LOOPING_SHAPES, SHAPES
from helpers.integrate_cases import FORM_N, FORM_NBLK
from helpers.incoherent_model import block_power, full_range_words, integrate, same_bits

pytestmark = pytest.mark.gpu

SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, 1.0, -3.0, 1e-45], dtype=np.float32)


def seeded_samples(A, C, nt, seed=0):
    ant = np.random.default_rng(1000 * A + C + seed).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    ant.reshape(-1)[0], ant.reshape(-1)[-1] = -128, 127
    return ant


def seeded_flags(A, seed=0):
    """Some antennas off (+0 or -0), the others on with every kind of value that is not 0."""
    rng = np.random.default_rng(A + seed)
    return SPECIALS[rng.integers(0, SPECIALS.size, size=A)] if A > 1 else np.array([0.5], np.float32)


class ICase(Context):
    """One context of A antennas and C channels (no delay table: the incoherent beam has no coefficients), its samples
    and its two outputs."""

    def __init__(self, gpu, A, C, nt, seed=0):
        from dc_sand_amd.generator import incoherent_block_power_bytes, incoherent_spectra_bytes

        super().__init__(gpu, C, A, NR_SAMPLES_PER_CHANNEL=nt)
        self.nt, self.nblk = nt, nt // 16
        self.spectra_bytes = lambda n: incoherent_spectra_bytes(self.bp, self.nblk, n)
        self.ant = seeded_samples(A, C, nt, seed)
        self.d_ant = self.alloc(self.ant.nbytes)
        self.pbytes = incoherent_block_power_bytes(self.bp, nt)
        assert self.pbytes == C * self.nblk * 4
        self.d_p = self.out(self.pbytes)
        self.d_s = self.out(self.pbytes)  # spectra: at most one per block
        self.d_w = self.alloc(A * 4)

    def set_ant(self, ant):
        self.ant = ant
        self.gpu.memcpy_htod(self.d_ant, ant)

    def call_power(self, weighted=False, stream=None):
        self.g.incoherent_block_power(self.d_ant, self.ant.nbytes, self.d_p, self.pbytes, self.nt,
                                      d_weights=self.d_w if weighted else None, stream=stream)

    def read_power(self):
        return self.read(self.d_p, self.pbytes, np.uint32, (self.C, self.nblk))

    def power(self, w=None):
        """One call from a clean output buffer."""
        gpu = self.gpu
        gpu.memcpy_htod(self.d_ant, self.ant)
        self.refill(self.d_p)
        if w is not None:
            gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
        self.call_power(weighted=w is not None)
        gpu.synchronize()
        return self.read_power()

    def set_power(self, P):
        """The integration's input given by the test."""
        assert P.dtype == np.uint32 and P.shape == (self.C, self.nblk)
        self.refill(self.d_p)
        self.gpu.memcpy_htod(self.d_p, np.ascontiguousarray(P))

    def call_integrate(self, n, accumulate=False, stream=None):
        self.g.integrate_incoherent_power(self.d_p, self.pbytes, self.nblk, n, self.d_s, self.spectra_bytes(n),
                                          accumulate=accumulate, stream=stream)

    def read_spectra(self, n):
        return self.read(self.d_s, self.spectra_bytes(n), np.float32, (self.nblk // n, self.C))

    def spectra(self, n, accumulate=False, prior=None):
        """One integration of what d_p holds; without ``accumulate`` from a clean buffer, with ``prior`` from that."""
        gpu = self.gpu
        if not accumulate or prior is not None:
            self.refill(self.d_s)
        if prior is not None:
            gpu.memcpy_htod(self.d_s, np.ascontiguousarray(prior, dtype=np.float32))
        self.call_integrate(n, accumulate)
        gpu.synchronize()
        return self.read_spectra(n)


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(ICase, gpu))


@pytest.mark.parametrize("A,C,nt", SHAPES + FORM_SHAPES)
def test_block_power_is_the_model(gpu, case, A, C, nt):
    c = case(A, C, nt)
    exp = block_power(c.ant)
    assert np.unique(exp).size >= min(100, exp.size), (np.unique(exp).size, exp.size)  # no trivial expectation
    got = c.power()
    assert got.dtype == exp.dtype and np.array_equal(got, exp), np.argwhere(got != exp)[:4]
    w = seeded_flags(A)
    got = c.power(w)
    assert np.array_equal(got, block_power(c.ant, w)), np.argwhere(got != block_power(c.ant, w))[:4]


@pytest.mark.parametrize("A,C,nt,rows_per_trip", LOOPING_SHAPES + FORM_LOOPING_SHAPES)
def test_block_power_when_a_wave_takes_a_second_trip(gpu, case, record_property, A, C, nt, rows_per_trip):
    """The launch geometry, read from a captured graph (nothing allocates, so the capture may come first), must prove the
    second trip: its waves, each carrying `rows_per_trip` rows per trip, cannot hold the rows in one."""
    c = case(A, C, nt)
    rows = C * c.nblk
    assert rows % rows_per_trip != 0 or rows_per_trip == 1
    s = gpu.Stream()
    nodes = hip_graph.launches(s, lambda: c.call_power(stream=s.handle))
    s.synchronize()
    assert len(nodes) == 1, nodes
    grid, block = nodes[0]
    assert grid[1] == grid[2] == 1 and block[1] == block[2] == 1 and block[0] % 64 == 0, nodes
    waves = grid[0] * (block[0] // 64)
    record_property("gridDim.x, blockDim.x, rows", (grid[0], block[0], rows))
    assert waves * rows_per_trip < rows, f"{grid[0]} workgroups of {block[0]} lanes take {rows} rows in one trip: raise the channel count"
    exp = block_power(c.ant)
    assert np.unique(exp).size >= 100
    got = c.power()
    assert got.dtype == exp.dtype and np.array_equal(got, exp), np.argwhere(got != exp)[:4]
    w = seeded_flags(A)
    exp = block_power(c.ant, w)
    got = c.power(w)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:4]


def test_integration_over_several_workgroups(gpu, case):
    """(33, 70, 128): 560 spectra values with one block per spectrum -- three workgroups of 256 lanes, the last one partial --
    and 280 with two, plain and accumulating from a seeded prior."""
    A, C, nt = 33, 70, 128
    c = case(A, C, nt)
    P = c.power()
    assert np.array_equal(P, block_power(c.ant))
    for n, total in ((1, 560), (2, 280)):
        exp = integrate(P, n)
        assert exp.size == total and np.unique(exp).size >= 100
        got = c.spectra(n)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        prior = np.random.default_rng(n).uniform(0.0, float(exp.max()), size=exp.shape).astype(np.float32)
        got = c.spectra(n, accumulate=True, prior=prior)
        assert same_bits(got, integrate(P, n, prior=prior)) is None, (n, "accumulate", same_bits(got, integrate(P, n, prior=prior)))


def test_integration_takes_every_unrolled_trip_and_tail(gpu, case):
    """The unit-stride uint32 integrator takes a lane's n words eight to a trip: n = 1 .. 5 (a tail alone), 8 and 16 (one and
    two whole trips), 9 and 17 (a tail behind them), plain and accumulating, over full-range words whose exact sums need
    all 64 bits of the running sum (helpers/launch_forms.integrate_trips; tests/test_launch_forms.py)."""
    C = 2
    c = case(1, C, FORM_NBLK * 16)
    P = np.random.default_rng(8).integers(0, 1 << 32, size=(C, FORM_NBLK), dtype=np.uint64).astype(np.uint32)
    P[0, :17] = 0xFFFFFFFF
    c.set_power(P)
    for n in FORM_N:
        exp = integrate(P, n)
        assert exp.shape == (FORM_NBLK // n, C) and np.unique(exp).size >= 100
        got = c.spectra(n)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        prior = np.random.default_rng(n).uniform(0.0, float(exp.max()), size=exp.shape).astype(np.float32)
        want = integrate(P, n, prior=prior)
        got = c.spectra(n, accumulate=True, prior=prior)
        assert same_bits(got, want) is None, (n, "accumulate", same_bits(got, want))


@pytest.mark.parametrize("A,C,nt", [(37, 2, 32), (130, 2, 32)])
def test_weights_are_flags(gpu, case, A, C, nt):
    c = case(A, C, nt)
    ref = block_power(c.ant)
    assert np.array_equal(c.power(), ref) and np.array_equal(c.power(np.ones(A, np.float32)), ref)  # NULL = all ones
    assert not c.power(np.zeros(A, np.float32)).any()
    assert not c.power(np.full(A, -0.0, np.float32)).any()
    # one antenna at a time, every antenna: that antenna's own sum (an index error cannot hide)
    x = c.ant.astype(np.int64)
    own = (x * x).sum(axis=(3, 4))  # [C][K][A]
    assert np.unique(own).size >= 100
    total = np.zeros_like(ref, dtype=np.int64)
    for a in range(A):
        w = np.zeros(A, np.float32)
        w[a] = SPECIALS[2 + a % (SPECIALS.size - 2)]  # some value that is not 0
        got = c.power(w)
        assert np.array_equal(got, own[:, :, a]), a
        total += got
    assert np.array_equal(total, ref)
    # seeded flags with -0.0, NaN, the infinities and 0.5 among them
    for seed in range(3):
        w = seeded_flags(A, seed)
        on = w != 0
        assert 0 < on.sum() < A and np.isnan(w).any() and np.isinf(w).any() and (w == 0.5).any() and np.signbit(w[w == 0]).any()
        assert np.array_equal(c.power(w), block_power(c.ant, w)), seed


def test_full_scale_needs_all_32_and_64_bits(gpu, case):
    A, C, nt, n = 256, 1, 640, 40
    c = case(A, C, nt)
    c.ant = np.full_like(c.ant, -128)
    got = c.power()
    assert np.all(got == 1 << 27)
    s = c.spectra(n)
    assert s.shape == (1, 1) and float(s[0, 0]) == float(5 << 30) and 5 << 30 > 1 << 32
    assert same_bits(s, integrate(got, n)) is None


def test_words_with_bit_31_set_are_unsigned(gpu, case):
    """Full-range words, which the detection never makes (it ends at 2^27): the 64-bit sum and its conversion are unsigned.
    The same bits read as int32 give other spectra, so a signed sum or a conversion through a signed type would show."""
    P = full_range_words()
    C, K = P.shape
    c = case(1, C, K * 16)
    c.set_power(P)
    for n in (1, 2, 3, 12):
        exp = integrate(P, n)
        signed = stokes_model.integrate(P.view(np.int32).reshape(C, K, 1, 1), n).reshape(K // n, C)
        assert (signed != exp).any(axis=1).all(), n
        got = c.spectra(n)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        prior = np.random.default_rng(n).uniform(0.0, float(exp.max()), size=exp.shape).astype(np.float32)
        got = c.spectra(n, accumulate=True, prior=prior)
        assert same_bits(got, integrate(P, n, prior=prior)) is None, (n, "accumulate", same_bits(got, integrate(P, n, prior=prior)))


@pytest.mark.parametrize("A,C,nt", [(64, 5, 256), (256, 2, 96)])
def test_integration_is_the_exact_sum_rounded_once(gpu, case, A, C, nt):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    c = case(A, C, nt)
    P = c.power()
    assert np.array_equal(P, block_power(c.ant))
    for n in (1, 2, c.nblk):
        got = c.spectra(n)
        exp = integrate(P, n)
        assert np.unique(exp).size >= min(100, exp.size)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
        if n > 1:  # sums that are no floats: the one rounding is exercised
            S = P.astype(np.int64).reshape(C, c.nblk // n, n).sum(axis=2).T
            assert np.any(exp.astype(np.float64) != S)
        # accumulate from a seeded prior
        prior = np.random.default_rng(n).uniform(0.0, float(exp.max()), size=exp.shape).astype(np.float32)
        got = c.spectra(n, accumulate=True, prior=prior)
        assert same_bits(got, integrate(P, n, prior=prior)) is None, (n, "accumulate")
    # one integration across two calls with different samples
    n = c.nblk
    first = c.spectra(n)
    c.ant = seeded_samples(A, C, nt, seed=5)
    P2 = c.power()
    assert np.array_equal(P2, block_power(c.ant)) and not np.array_equal(P2, P)
    both = c.spectra(n, accumulate=True)
    assert same_bits(first, integrate(P, n)) is None
    assert same_bits(both, integrate(P2, n, prior=integrate(P, n))) is None
    # a bad blocks_per_spectrum and buffers one byte short are refused, nothing is enqueued, the stream stays usable
    s = gpu.Stream()
    c.refill(c.d_s)
    c.refill(c.d_p)
    gpu.synchronize()
    for bad in (0, c.nblk + 1, 3 if c.nblk % 3 else 5):
        with pytest.raises(DcsError) as e:
            c.g.integrate_incoherent_power(c.d_p, c.pbytes, c.nblk, bad, c.d_s, c.pbytes, stream=s.handle)
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, bad
    with pytest.raises(DcsError) as e:  # block powers one byte short
        c.g.integrate_incoherent_power(c.d_p, c.pbytes - 1, c.nblk, 2, c.d_s, c.spectra_bytes(2), stream=s.handle)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # spectra one byte short
        c.g.integrate_incoherent_power(c.d_p, c.pbytes, c.nblk, 2, c.d_s, c.spectra_bytes(2) - 1, stream=s.handle)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # samples one byte short
        c.g.incoherent_block_power(c.d_ant, c.ant.nbytes - 1, c.d_p, c.pbytes, nt, stream=s.handle)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # block powers one byte short
        c.g.incoherent_block_power(c.d_ant, c.ant.nbytes, c.d_p, c.pbytes - 1, nt, stream=s.handle)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(DcsError) as e:  # samples not 16-byte aligned
        c.g.incoherent_block_power(int(c.d_ant) + 8, c.ant.nbytes, c.d_p, c.pbytes, nt, stream=s.handle)
    assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    s.synchronize()
    for d in (c.d_s, c.d_p):
        assert np.all(c.read(d) == 0xA5)
    c.call_power(stream=s.handle)
    c.call_integrate(2, stream=s.handle)
    s.synchronize()
    assert np.array_equal(c.read_power(), P2) and same_bits(c.read_spectra(2), integrate(P2, 2)) is None


@pytest.mark.parametrize("A,C,nt", [(64, 3, 48), (130, 2, 32)])
def test_outputs_at_an_address_that_is_4_byte_aligned_only(gpu, case, A, C, nt):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    c = case(A, C, nt)
    w = seeded_flags(A)
    gpu.memcpy_htod(c.d_ant, c.ant)
    ref = block_power(c.ant, w)
    d_w = c.alloc(A * 4 + 16)
    gpu.memcpy_htod(int(d_w) + 4, w)
    d_big = c.out(c.pbytes + 16)
    c.g.incoherent_block_power(c.d_ant, c.ant.nbytes, int(d_big) + 4, c.pbytes, nt, d_weights=int(d_w) + 4)
    gpu.synchronize()
    host = c.read(d_big)
    assert np.all(host[:4] == 0xA5) and np.all(host[4 + c.pbytes:] == 0xA5)
    assert np.array_equal(host[4:4 + c.pbytes].view(np.uint32).reshape(C, c.nblk), ref)
    # ... and integrated from there, into spectra that are 4-byte aligned only
    d_sp = c.out(c.pbytes + 16)
    nb = c.spectra_bytes(c.nblk)
    c.g.integrate_incoherent_power(int(d_big) + 4, c.pbytes, c.nblk, c.nblk, int(d_sp) + 4, nb)
    gpu.synchronize()
    host = c.read(d_sp)
    assert np.all(host[:4] == 0xA5) and np.all(host[4 + nb:] == 0xA5)
    assert same_bits(host[4:4 + nb].view(np.float32).reshape(1, C), integrate(ref, c.nblk)) is None
    for args in ((int(d_big) + 2, None), (int(d_big), int(d_w) + 2)):  # 2-byte alignment is refused
        with pytest.raises(DcsError) as e:
            c.g.incoherent_block_power(c.d_ant, c.ant.nbytes, args[0], c.pbytes, nt, d_weights=args[1])
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT
    for p_in, p_out in ((int(d_big) + 2, int(d_sp)), (int(d_big), int(d_sp) + 2)):
        with pytest.raises(DcsError) as e:
            c.g.integrate_incoherent_power(p_in, c.pbytes, c.nblk, c.nblk, p_out, nb)
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("A,C,nt", [(64, 3, 64), (130, 3, 64)])
def test_captured_first_calls_pick_up_new_samples_on_replay(gpu, case, A, C, nt):
    """Both calls in one hipGraph as the first calls on a fresh context -- nothing allocates, so nothing has to be run
    outside the capture first -- replayed with new samples in the same buffer (the process's default queue count is
    left as it is)."""
    c = case(A, C, nt)
    n = 2
    w = seeded_flags(A)
    gpu.memcpy_htod(c.d_w, w)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.call_power(weighted=True, stream=s.handle)
        c.call_integrate(n, stream=s.handle)
    ants = [c.ant] + [seeded_samples(A, C, nt, seed=100 + i) for i in range(2)]
    refs = [block_power(ant, w) for ant in ants]
    assert not np.array_equal(refs[0], refs[1])
    for i in (1, 2, 0, 1):
        gpu.memcpy_htod(c.d_ant, ants[i], stream=s.handle, sync=False)
        c.refill(c.d_p, stream=s.handle)
        c.refill(c.d_s, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(c.read_power(), refs[i]), i
        assert same_bits(c.read_spectra(n), integrate(refs[i], n)) is None, i
    graph.close()
