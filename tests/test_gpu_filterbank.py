"""8-bit search filterbanks on the GPU (include/dcs_filterbank.h).  No tolerance anywhere: bytes,
counts and float / double bit patterns are compared with the numpy model (helpers/filterbank_model.py, anchored on the CPU
by tests/test_filterbank_model.py).  The tests supply the float spectra directly -- no beamformer runs, except for the
incoherent spectra of the last test but one.  Every buffer is exactly sized; every output has a 0xA5 canary behind it,
which must stay untouched, and the filterbank rows outside [first, first + nr_spectra) are prefilled and must stay as
they were."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers.device_buffers import Context, closed_after
from helpers.filterbank_model import filterbank, quantise, same_bits, scales, spectra_sums

pytestmark = pytest.mark.gpu

PREFILL = 0x3C
TARGET_STD, LEVEL = 24.0, 128.0


def bandpass(C, B, seed):
    """m_cb, spread over 2^-20 .. 2^20."""
    return np.exp2(np.random.default_rng(77 * C + B + seed).uniform(-20.0, 20.0, size=(C, B))).astype(np.float32)


def seeded_spectra(C, B, T, seed=0):
    """x = m_cb (1 + 0.25 g), g normal: float32 [T][C][B], and m."""
    m = bandpass(C, B, seed)
    g = np.random.default_rng(1000 * C + 10 * B + T + seed).standard_normal((T, C, B))
    return (m[None].astype(np.float64) * (1.0 + 0.25 * g)).astype(np.float32), m


def given_scales(m):
    """The scales of the distribution itself: mu = m, k = target_std / (0.25 m).  y = 128 + 24 g up to rounding, so the
    quantiser clips at |g| > 5.3 and nothing else."""
    return np.stack([m, (np.float64(TARGET_STD) / (0.25 * m.astype(np.float64))).astype(np.float32)], axis=-1)


def place_specials(x, seed=0):
    """NaN, +-Inf, +-0, a subnormal and a negative at seeded positions (a quarter of the elements at the most); the mask."""
    x = x.copy()
    n = min(7, x.size // 4)
    pos = np.random.default_rng(x.size + seed).choice(x.size, size=n, replace=False)
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, None]
    flat = x.reshape(-1)
    for p, v in zip(pos, values):
        flat[p] = -abs(flat[p]) if v is None else np.float32(v)
    mask = np.zeros(x.size, bool)
    mask[pos] = True
    return x, mask.reshape(x.shape)


class FCase(Context):
    """One context of C channels (no delay table: the filterbank has no coefficients; nr_beams is an argument), and the
    device buffers of one (C, B, T) case, exactly sized, outputs with a canary behind."""

    def __init__(self, gpu, C, B, T, out_spectra=None, first=0, spectra_offset=0, stations=1):
        from dc_sand_amd.generator import filterbank_bytes, filterbank_scales_bytes, spectra_sums_bytes

        super().__init__(gpu, C, A=stations)
        self.B, self.T, self.first = B, T, first
        self.out_spectra = T + first if out_spectra is None else out_spectra
        self.xbytes = T * C * B * 4
        self.sums_bytes, self.scales_bytes = spectra_sums_bytes(self.bp, B), filterbank_scales_bytes(self.bp, B)
        self.fb_bytes = filterbank_bytes(self.bp, B, self.out_spectra)
        assert (self.sums_bytes, self.scales_bytes, self.fb_bytes) == (C * B * 16, C * B * 8, B * self.out_spectra * C)
        self.d_x = int(self.alloc(self.xbytes + spectra_offset)) + spectra_offset  # the last spectrum ends where the allocation ends
        self.d_sums, self.d_scales = self.out(self.sums_bytes), self.out(self.scales_bytes)
        self.d_fb, self.d_clips = self.out(self.fb_bytes, PREFILL), self.out(B * 8, 0)
        gpu.synchronize()

    def put(self, d, a):
        self.gpu.memcpy_htod(d, np.ascontiguousarray(a))

    def call_sums(self, accumulate=False, stream=None, T=None):
        T = self.T if T is None else T
        self.g.spectra_sums(self.d_x, T * self.C * self.B * 4, T, self.B, self.d_sums, self.sums_bytes, accumulate=accumulate,
                            stream=stream)

    def call_scales(self, count, stream=None, target_std=TARGET_STD):
        self.g.filterbank_scales(self.d_sums, self.sums_bytes, count, self.B, target_std, self.d_scales, self.scales_bytes,
                                 stream=stream)

    def call_q8(self, descending=False, counters=True, stream=None):
        self.g.filterbank_q8(self.d_x, self.xbytes, self.T, self.B, self.d_scales, LEVEL, self.d_fb, self.fb_bytes,
                             self.out_spectra, first_spectrum=self.first, descending=descending,
                             d_clip_count=self.d_clips if counters else None, stream=stream)

    def read_sums(self):
        return self.read(self.d_sums, self.sums_bytes, np.float64, (self.C, self.B, 2))

    def read_scales(self):
        return self.read(self.d_scales, self.scales_bytes, np.float32, (self.C, self.B, 2))

    def reset_outputs(self, stream=None):
        self.refill(self.d_fb, stream=stream)
        self.refill(self.d_clips, stream=stream)

    def read_filterbank(self):
        return self.read(self.d_fb, self.fb_bytes, np.uint8, (self.B, self.out_spectra, self.C))

    def read_clips(self):
        return self.read(self.d_clips, self.B * 8, np.uint64, (self.B,))

    def q8(self, descending=False, counters=True):
        """One call from prefilled outputs: the whole buffer and the counters (zero where none were asked for)."""
        self.reset_outputs()
        self.call_q8(descending, counters)
        self.gpu.synchronize()
        return self.read_filterbank(), self.read_clips()

    def expect(self, x, sc, descending=False):
        prefill = np.full((self.B, self.out_spectra, self.C), PREFILL, np.uint8)
        return filterbank(x, sc, LEVEL, descending=descending, out=prefill, first=self.first)


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(FCase, gpu))


def check_bytes(c, x, sc, special, min_distinct=True):
    """Both channel orders with counters, and without counters the same bytes; what the model's expectation must be."""
    exp, counts = c.expect(x, sc)
    written = exp[:, c.first:c.first + c.T]
    n = written.size
    if min_distinct:
        assert np.unique(written).size >= min(50, max(1, n // 8)), (np.unique(written).size, n)  # no trivial expectation
    _, clipped = quantise(x, sc, LEVEL)
    assert not (clipped & ~special).any(), "the model clips outside the specials"
    assert counts.sum() == clipped.sum()
    got, got_counts = c.q8()
    assert same_bits(got, exp) is None, ("ascending", same_bits(got, exp))
    assert np.array_equal(got_counts, counts), (got_counts, counts)
    got, got_counts = c.q8(counters=False)
    assert same_bits(got, exp) is None and not got_counts.any(), "no counters"
    exp_d, counts_d = c.expect(x, sc, descending=True)
    assert np.array_equal(counts_d, counts) and (c.C == 1 or n < 16 or not np.array_equal(exp_d, exp))
    got, got_counts = c.q8(descending=True)
    assert same_bits(got, exp_d) is None, ("descending", same_bits(got, exp_d))
    assert np.array_equal(got_counts, counts)


# The tile is 128 channels x 32 beams: both sides of each boundary, one and several tiles either way, a single element, a
# single beam, beams that are no multiple of 4, channels that are no multiple of 16; the fast form at (128, 32, 2),
# (256, 64, 5), (16, 4, 40) and (144, 36, 33), the last two with the time axis split over workgroups
SHAPES = [(1, 1, 1), (3, 5, 4), (127, 31, 3), (128, 32, 2), (129, 33, 3), (256, 64, 5), (130, 1, 7), (5, 300, 2), (16, 4, 40),
          (144, 36, 33)]


@pytest.mark.parametrize("C,B,T", SHAPES)
def test_sums_scales_and_bytes_are_the_model(gpu, case, C, B, T):
    first = 3 if T > 1 else 0
    c = case(C, B, T, out_spectra=T + first + (2 if first else 0), first=first)
    clean, m = seeded_spectra(C, B, T)
    c.put(c.d_x, clean)
    c.call_sums()
    c.call_scales(T)
    gpu.synchronize()
    sums = spectra_sums(clean)
    assert same_bits(c.read_sums(), sums) is None, same_bits(c.read_sums(), sums)
    assert same_bits(c.read_scales(), scales(sums, T, TARGET_STD)) is None, same_bits(c.read_scales(), scales(sums, T, TARGET_STD))
    x, special = place_specials(clean)
    sc = given_scales(m)
    c.put(c.d_x, x)
    c.put(c.d_scales, sc)
    check_bytes(c, x, sc, special)
    # the sums of the spectra with the specials in them: NaN and Inf go through as the arithmetic takes them
    c.call_sums()
    gpu.synchronize()
    assert same_bits(c.read_sums(), spectra_sums(x)) is None


@pytest.mark.parametrize("C,B,T", [(16, 4, 40), (144, 36, 33), (128, 32, 2)])
def test_fast_shape_whose_spectra_are_4_byte_aligned_only(gpu, case, C, B, T):
    c = case(C, B, T, out_spectra=T + 4, first=1, spectra_offset=4)
    assert c.d_x % 16 == 4
    clean, m = seeded_spectra(C, B, T, seed=1)
    x, special = place_specials(clean, seed=1)
    sc = given_scales(m)
    c.put(c.d_x, x)
    c.put(c.d_scales, sc)
    check_bytes(c, x, sc, special)
    c.call_sums()
    gpu.synchronize()
    assert same_bits(c.read_sums(), spectra_sums(x)) is None


def test_a_workgroup_walks_several_slices_and_the_time_axis_is_split(gpu, case, record_property):
    """From the captured launch geometry, not from the launcher's arithmetic: gridDim.y is the number of runs that the time
    axis is cut into, so a call of T spectra has a workgroup that walks at least three slices where
    2 * gridDim.y < T, and its time axis is split where gridDim.y > 1."""
    seen = {}
    for C, B, T in ((256, 64, 5), (16, 4, 40), (144, 36, 33)):
        c = case(C, B, T)
        clean, m = seeded_spectra(C, B, T, seed=2)
        x, special = place_specials(clean, seed=2)
        sc = given_scales(m)
        c.put(c.d_x, x)
        c.put(c.d_scales, sc)
        s = gpu.Stream()
        nodes = hip_graph.launches(s, lambda: c.call_q8(stream=s.handle))
        s.synchronize()
        assert len(nodes) == 1, nodes
        grid, block = nodes[0]
        assert grid[2] == 1 and block == (256, 1, 1), nodes
        record_property(f"grid of {(C, B, T)}", grid)
        seen[(C, B, T)] = (2 * grid[1] < T, grid[1] > 1)
        check_bytes(c, x, sc, special)
    assert seen[(256, 64, 5)][0], "no case in which one workgroup walks at least 3 slices of an unsplit time axis"
    assert seen[(16, 4, 40)] == (True, True) and seen[(144, 36, 33)] == (True, True), seen


def test_scale_edges(gpu, case):
    """Scales given by the test: k of 0, Inf and NaN and a NaN mu; then a constant channel, which the scales call gives k = 0."""
    C, B, T = 40, 12, 6
    c = case(C, B, T)
    clean, m = seeded_spectra(C, B, T, seed=3)
    sc = given_scales(m)
    sc[1, 2, 1] = 0.0
    sc[5, 0, 1] = np.inf
    sc[7, 11, 1] = np.nan
    sc[39, 4, 0] = np.nan
    sc[20, 3, 1] = -sc[20, 3, 1]  # a negative gain is arithmetic like any other
    special = np.zeros(clean.shape, bool)
    for cc, bb in ((5, 0), (7, 11), (39, 4)):
        special[:, cc, bb] = True
    c.put(c.d_x, clean)
    c.put(c.d_scales, sc)
    check_bytes(c, clean, sc, special)
    exp, counts = c.expect(clean, sc)
    assert np.all(exp[2, :, 1] == 128) and np.all(exp[11, :, 7] == 0) and np.all(exp[4, :, 39] == 0)
    assert set(np.unique(exp[0, :, 5])) <= {0, 255} and counts[0] == T and counts[11] == T and counts[4] == T
    # a constant channel (every beam of channel 9), and a constant (channel, beam)
    x = clean.copy()
    x[:, 9, :] = x[0, 9, :]
    x[:, 30, 5] = np.float32(0.1)
    c.put(c.d_x, x)
    c.call_sums()
    c.call_scales(T)
    gpu.synchronize()
    sums = spectra_sums(x)
    sc = scales(sums, T, TARGET_STD)
    assert same_bits(c.read_sums(), sums) is None
    got = c.read_scales()
    assert same_bits(got, sc) is None, same_bits(got, sc)
    assert np.all(got[9, :, 1] == 0) and got[30, 5, 1] == 0 and np.count_nonzero(got[..., 1] == 0) == B + 1
    # the device's own scales: sample statistics of T = 6 spectra, so nothing is said about clipping here
    fb, _ = c.q8()
    exp, _ = c.expect(x, sc)
    assert same_bits(fb, exp) is None
    assert np.all(fb[:, :, 9] == 128) and np.all(fb[5, :, 30] == 128)


def test_device_divide_and_square_root_are_the_correctly_rounded_ones(gpu, case):
    """4096 seeded sums per count: the scales call against numpy's float64 divide and sqrt, which are correctly rounded."""
    C, B = 64, 64
    c = case(C, B, 1)
    rng = np.random.default_rng(2026)
    for count in (1, 1000, (1 << 40) + 3, (1 << 53) - 1):
        m = np.exp2(rng.uniform(-20, 20, size=(C, B))) * (1 + rng.uniform(size=(C, B)))
        sd = m * np.exp2(rng.uniform(-8, 1, size=(C, B)))
        N = np.float64(count)
        sums = np.stack([m * N, (m * m + sd * sd) * N], axis=-1)
        c.put(c.d_sums, sums)
        c.call_scales(count, target_std=7.3)
        gpu.synchronize()
        got, exp = c.read_scales(), scales(sums, count, 7.3)
        assert np.count_nonzero(exp[..., 1]) > 0.9 * C * B and np.unique(exp[..., 1]).size > 0.8 * C * B
        assert same_bits(got[..., 0], exp[..., 0]) is None, ("mu: the divide", count, same_bits(got[..., 0], exp[..., 0]))
        assert same_bits(got[..., 1], exp[..., 1]) is None, ("k: divide, sqrt, divide", count, same_bits(got[..., 1], exp[..., 1]))


def test_accumulate_over_three_calls_and_on_graph_replay(gpu, case):
    C, B = 70, 9
    parts = [seeded_spectra(C, B, T, seed=10 + i)[0] for i, T in enumerate((5, 1, 11))]
    joined = np.concatenate(parts)
    one = case(C, B, joined.shape[0])
    one.put(one.d_x, joined)
    one.call_sums()
    gpu.synchronize()
    whole = one.read_sums()
    assert same_bits(whole, spectra_sums(joined)) is None
    c = case(C, B, 11)
    for i, part in enumerate(parts):
        c.put(c.d_x, part)
        c.call_sums(accumulate=i > 0, T=part.shape[0])
        gpu.synchronize()
    assert same_bits(c.read_sums(), whole) is None, same_bits(c.read_sums(), whole)
    # without accumulate the call starts from {0, 0} whatever the buffer holds (it holds the sums of above)
    c.call_sums()
    gpu.synchronize()
    assert same_bits(c.read_sums(), spectra_sums(parts[2])) is None
    # the accumulating call in a graph, replayed after new spectra are copied into the same buffer
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.call_sums(accumulate=True, stream=s.handle)
    running = spectra_sums(parts[2])
    for i in range(3):
        new = seeded_spectra(C, B, 11, seed=20 + i)[0]
        gpu.memcpy_htod(c.d_x, new, stream=s.handle, sync=False)
        graph.launch(s)
        s.synchronize()
        running = spectra_sums(new, prior=running)
        assert same_bits(c.read_sums(), running) is None, i
    graph.close()


@pytest.mark.parametrize("C,B,T", [(48, 8, 12), (37, 3, 9)])
def test_all_three_calls_captured_as_first_calls_on_a_fresh_context(gpu, case, C, B, T):
    """Nothing allocates, so nothing has to run outside the capture first; replayed with new spectra in the same buffer."""
    c = case(C, B, T, out_spectra=T + 2, first=1)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.call_sums(stream=s.handle)
        c.call_scales(T, stream=s.handle)
        c.call_q8(descending=True, stream=s.handle)
    for i in range(3):
        x = seeded_spectra(C, B, T, seed=30 + i)[0]
        gpu.memcpy_htod(c.d_x, x, stream=s.handle, sync=False)
        c.reset_outputs(stream=s.handle)
        graph.launch(s)
        s.synchronize()
        sums = spectra_sums(x)
        sc = scales(sums, T, TARGET_STD)
        assert same_bits(c.read_sums(), sums) is None, i
        assert same_bits(c.read_scales(), sc) is None, i
        exp, counts = c.expect(x, sc, descending=True)
        assert np.unique(exp).size >= 30
        assert same_bits(c.read_filterbank(), exp) is None, i
        assert np.array_equal(c.read_clips(), counts), i
    graph.close()


def test_buffers_one_byte_short_are_refused_and_nothing_is_enqueued(gpu, case):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    C, B, T = 20, 6, 4
    c = case(C, B, T)
    g = c.g
    c.reset_outputs()
    gpu.synchronize()
    calls = [
        lambda: g.spectra_sums(c.d_x, c.xbytes - 1, T, B, c.d_sums, c.sums_bytes),
        lambda: g.spectra_sums(c.d_x, c.xbytes, T, B, c.d_sums, c.sums_bytes - 1),
        lambda: g.spectra_sums(c.d_x, c.xbytes, T, B + 1, c.d_sums, c.sums_bytes),
        lambda: g.filterbank_scales(c.d_sums, c.sums_bytes - 1, T, B, TARGET_STD, c.d_scales, c.scales_bytes),
        lambda: g.filterbank_scales(c.d_sums, c.sums_bytes, T, B, TARGET_STD, c.d_scales, c.scales_bytes - 1),
        lambda: g.filterbank_q8(c.d_x, c.xbytes - 1, T, B, c.d_scales, LEVEL, c.d_fb, c.fb_bytes, T),
        lambda: g.filterbank_q8(c.d_x, c.xbytes, T, B, c.d_scales, LEVEL, c.d_fb, c.fb_bytes - 1, T),
        lambda: g.filterbank_q8(c.d_x, c.xbytes, T, B, c.d_scales, LEVEL, c.d_fb, c.fb_bytes, T + 1, first_spectrum=1),
        lambda: g.filterbank_q8(c.d_x, c.xbytes, T, B, c.d_scales, LEVEL, c.d_fb, c.fb_bytes, T, first_spectrum=1),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    gpu.synchronize()
    assert np.all(c.read_filterbank() == PREFILL) and not c.read_clips().any()
    assert np.all(c.read(c.d_sums) == 0xA5)


def test_incoherent_spectra_with_one_beam(gpu, case):
    """nr_beams = 1 on real output of integrate_incoherent_power at 64 antennas and 7 channels."""
    from dc_sand_amd.generator import incoherent_block_power_bytes, incoherent_spectra_bytes

    A, C, n, T = 64, 7, 2, 12
    nt = 16 * n * T
    c = case(C, 1, T, stations=A)
    ant = np.random.default_rng(64).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    ant[3] //= 4  # a bandpass: channel 3 is 12 dB down
    d_ant = c.upload(ant)
    pbytes, sbytes = incoherent_block_power_bytes(c.bp, nt), incoherent_spectra_bytes(c.bp, nt // 16, n)
    assert sbytes == c.xbytes
    d_p = c.alloc(pbytes)
    c.g.incoherent_block_power(d_ant, ant.nbytes, d_p, pbytes, nt)
    c.g.integrate_incoherent_power(d_p, pbytes, nt // 16, n, c.d_x, sbytes)
    c.call_sums()
    c.call_scales(T)
    gpu.synchronize()
    x = np.empty((T, C, 1), np.float32)
    gpu.memcpy_dtoh(x, c.d_x)
    assert np.all(x > 0) and x[:, 3].max() < x[:, 2].min() / 8
    sums = spectra_sums(x)
    sc = scales(sums, T, TARGET_STD)
    assert same_bits(c.read_sums(), sums) is None
    assert same_bits(c.read_scales(), sc) is None
    assert np.all(sc[..., 1] > 0)
    for desc in (False, True):
        fb, clips = c.q8(descending=desc)
        exp, counts = c.expect(x, sc, descending=desc)
        assert np.unique(exp).size >= 20 and abs(float(exp.mean()) - LEVEL) < 1.0  # the bandpass is taken out
        assert same_bits(fb, exp) is None and np.array_equal(clips, counts), desc


@pytest.mark.parametrize("C,B,T", [(129, 33, 3), (128, 32, 4)])
def test_a_nan_leaves_every_other_channel_and_beam_bit_identical(gpu, case, C, B, T):
    c = case(C, B, T)
    clean, _ = seeded_spectra(C, B, T, seed=40)
    cc, bb = C - 2, B // 2

    def run(x):
        c.put(c.d_x, x)
        c.call_sums()
        c.call_scales(T)
        fb, clips = c.q8()
        return c.read_sums(), c.read_scales(), fb, clips

    ref = run(clean)
    x = clean.copy()
    x[T // 2, cc, bb] = np.nan
    got = run(x)
    other = np.ones((C, B), bool)
    other[cc, bb] = False
    for r, g_ in zip(ref[:2], got[:2]):
        assert same_bits(g_[other], r[other]) is None and np.all(np.isnan(g_[cc, bb, 0]))
    assert got[1][cc, bb, 1] == 0  # a NaN variance gives k = 0
    fb_other = np.ones((B, T, C), bool)
    fb_other[bb, :, cc] = False
    assert np.array_equal(got[2][fb_other], ref[2][fb_other]) and np.all(got[2][bb, :, cc] == 0)
    assert got[3][bb] == ref[3][bb] + T and np.array_equal(np.delete(got[3], bb), np.delete(ref[3], bb))
    sums = spectra_sums(x)
    assert same_bits(got[0], sums) is None and same_bits(got[1], scales(sums, T, TARGET_STD)) is None
