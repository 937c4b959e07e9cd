"""The polyphase channeliser on the GPU (include/dcs_channeliser.h).  Every output is compared with
the numpy model (helpers/channeliser_model.py, anchored on the CPU by tests/test_channeliser_model.py) bit for bit: there is no
tolerance.  Input rows sit in strides whose padding holds other data than the rows (a read across a row shows); outputs are
prefilled with a canary behind them, and the blocks and inputs outside a call's window must keep their prefill."""
import numpy as np
import pytest

from dc_sand_amd import channeliser
from helpers import channeliser_model as model
from helpers.channeliser_cases import QUANTISED_CASES, SIZES
from helpers import correlator_model, ddc_model, hip_graph
from helpers.device_buffers import Context
from helpers.examples import run_example

pytestmark = pytest.mark.gpu

F = np.float32
PREFILL = 0xA5


def nan_table(N):
    """twiddles(N) with the two entries that the network never uses set to NaN: no NaN may come out."""
    W = channeliser.twiddles(N)
    W[0], W[N // 4] = np.nan, np.nan
    return W


class ChCase(Context):
    """A context (its sizes play no part: the channeliser takes every size as an argument) and the means to run one call from
    host arrays."""

    def __init__(self, gpu, C=1, A=1, nt=16):
        super().__init__(gpu, C, A, NR_SAMPLES_PER_CHANNEL=nt)

    def put_input(self, z, pairs, in_pad=24):
        """z float32 [ni][>= pairs][2] -> (device pointer, bytes, stride): every row in a stride of in_pad more pairs, which
        hold the NEXT row's data shifted and offset; the last row ends where the allocation ends."""
        z = np.asarray(z, dtype=F)[:, :pairs]
        ni = z.shape[0]
        stride = pairs + in_pad
        host = np.empty((ni, stride, 2), dtype=F)
        host[:, :pairs] = z
        host[:, pairs:] = np.roll(z, -1, axis=0)[:, 5:5 + in_pad] + F(1.0)
        flat = host.reshape(-1, 2)[:(ni - 1) * stride + pairs]
        return self.upload(flat), flat.nbytes, stride

    def run(self, z, h, W, N, P, ns, order=0, gains=None, d_counts=None, out_blocks=None, first_block=0, out_inputs=None,
            first_input=0, d_out=None, in_pad=24):
        """One call into a prefilled tensor [N][out_blocks][out_inputs][16][2] (a new one unless d_out is given), which is
        returned whole: float32, or int8 where gains are given."""
        from dc_sand_amd.generator import channelised_bytes, channeliser_in_pairs

        ni = np.asarray(z).shape[0]
        out_blocks = ns // 16 if out_blocks is None else out_blocks
        out_inputs = ni if out_inputs is None else out_inputs
        pairs = channeliser_in_pairs(N, P, ns)
        d_in, in_bytes, stride = self.put_input(z, pairs, in_pad)
        q8 = gains is not None
        obytes = channelised_bytes(N, out_blocks, out_inputs, q8)
        if d_out is None:
            d_out = self.out(obytes)
        d_h, d_w = self.upload(np.asarray(h, dtype=F)), self.upload(np.asarray(W, dtype=F))
        if q8:
            self.g.channelise_q8(d_in, in_bytes, stride, ni, ns, N, P, d_h, d_w, self.upload(np.asarray(gains, dtype=F)), d_out,
                                 obytes, out_blocks, out_inputs, first_block, first_input, order, d_clip_count=d_counts)
        else:
            self.g.channelise(d_in, in_bytes, stride, ni, ns, N, P, d_h, d_w, d_out, obytes, out_blocks, out_inputs, first_block,
                              first_input, order)
        self.gpu.synchronize()
        self.last_out = d_out
        return self.read(d_out, obytes, np.int8 if q8 else F, (N, out_blocks, out_inputs, 16, 2))

    def counters(self, ni):
        return self.upload(np.zeros(ni, dtype=np.uint64))

    def read_counters(self, d, ni):
        n = np.empty(ni, dtype=np.uint64)
        self.gpu.memcpy_dtoh(n, d)
        return n


@pytest.fixture
def case(gpu):
    c = ChCase(gpu)
    yield c
    c.close()


def window_is(got, exp, first_block=0, first_input=0):
    """The call's window of the tensor ``got`` is ``exp`` bit for bit and every other byte its prefill; None, or what differs."""
    nb, ni = exp.shape[1], exp.shape[2]
    win = got[:, first_block:first_block + nb, first_input:first_input + ni]
    if got.dtype == np.int8:
        bad = None if np.array_equal(win, exp) else np.argwhere(win != exp)[:4].tolist()
    else:
        bad = model.same_bits(win, exp)
    if bad is not None:
        return ("window", bad)
    rest = got.copy().view(np.uint8)
    rest[:, first_block:first_block + nb, first_input:first_input + ni] = PREFILL
    return None if np.all(rest == PREFILL) else ("written outside the window", np.argwhere(rest != PREFILL)[:4].tolist())


# ---- 1. float output and placement: every N (every stage count and grouping), P in {1, 2, 5, 16}, 16, 32 and 48 spectra, 1, 3
# and 5 inputs (the remainders of the workgroups' groups of 4, 2 and 1 inputs), both orders


@pytest.mark.parametrize("N", SIZES)
def test_the_float_output_is_the_model_in_its_place(case, N):
    W = nan_table(N)
    extra = [(5, 16), (1, 48), (3, 48), (5, 32)]
    k = 0
    for p, P in enumerate((1, 2, 5, 16)):
        for ni, ns in [(1, 16), (3, 32), (5, 48), extra[p]]:
            order = k & 1
            k += 1
            z = model.seeded_input(ni, (ns + P - 1) * N, seed=1000 * N + 10 * P + ni)
            h = model.seeded_taps(N, P, seed=N + P)
            exp = model.tensor(model.channelise(z, h, W, N, P, ns, order))
            assert not np.isnan(exp).any() and np.unique(exp).size > exp.size // 4  # no trivial expectation
            got = case.run(z, h, W, N, P, ns, order, out_blocks=ns // 16 + 2, first_block=1, out_inputs=ni + 2, first_input=1)
            bad = window_is(got, exp, 1, 1)
            assert bad is None, (N, P, ni, ns, order, bad)
            if k % 4 == 1:  # the same call filling its tensor: first_block = first_input = 0, the last run ends at the canary
                assert window_is(case.run(z, h, W, N, P, ns, order), exp) is None, (N, P, ni, ns, order)


@pytest.mark.parametrize("N", (128, 1024))
def test_two_calls_that_fill_a_tensor_are_one_call(case, N):
    from dc_sand_amd.generator import channelised_bytes

    P, ni, ns = 5, 5, 48
    W = channeliser.twiddles(N)
    z = model.seeded_input(ni, (ns + P - 1) * N, seed=N)
    h = model.seeded_taps(N, P, seed=N + 1)
    whole = case.run(z, h, W, N, P, ns, order=1)
    assert model.same_bits(whole, model.tensor(model.channelise(z, h, W, N, P, ns, 1))) is None
    # by blocks: spectra 0 .. 15, then 16 .. 47 from the row advanced by 16 N pairs (the last (P - 1) N presented again)
    d = case.out(channelised_bytes(N, ns // 16, ni))
    case.run(z, h, W, N, P, 16, order=1, out_blocks=ns // 16, d_out=d)
    parts = case.run(z[:, 16 * N:], h, W, N, P, 32, order=1, out_blocks=ns // 16, first_block=1, d_out=d)
    assert model.same_bits(parts, whole) is None
    # by inputs: 0 and 1, then 2 .. 4
    d = case.out(channelised_bytes(N, ns // 16, ni))
    case.run(z[:2], h, W, N, P, ns, order=1, out_inputs=ni, d_out=d)
    parts = case.run(z[2:], h, W, N, P, ns, order=1, out_inputs=ni, first_input=2, d_out=d)
    assert model.same_bits(parts, whole) is None


# ---- 2. quantised output


@pytest.mark.parametrize("N,P,ni,ns", QUANTISED_CASES)
def test_the_quantised_output_is_the_model_and_the_float_output_quantised(case, N, P, ni, ns):
    W = channeliser.twiddles(N)
    z = model.seeded_input(ni, (ns + P - 1) * N, seed=N + P)
    h = model.seeded_taps(N, P, seed=N)
    X = model.channelise(z, h, W, N, P, ns)
    gains = model.case_gains(X, N)
    exp_q, exp_n = model.quantise(model.tensor(X), gains)
    share = float(exp_n.sum()) / exp_q.size
    print(f"N = {N}, P = {P}: the model clips {100 * share:.1f} % and uses {np.unique(exp_q).size} byte values")
    assert 0.05 <= share <= 0.4 and np.unique(exp_q).size == 255  # on the model, before the GPU is looked at
    d_n = case.counters(ni)
    got_q = case.run(z, h, W, N, P, ns, gains=gains, d_counts=d_n)
    assert np.array_equal(got_q, exp_q), np.argwhere(got_q != exp_q)[:4].tolist()
    assert np.array_equal(case.read_counters(d_n, ni), exp_n)
    got_f = case.run(z, h, W, N, P, ns)
    assert np.array_equal(got_q, model.quantise(got_f, gains)[0])  # "quantise what the float call returns"
    # NULL counters: the same bytes; a second counted call: the counters accumulate
    assert np.array_equal(case.run(z, h, W, N, P, ns, gains=gains), exp_q)
    case.run(z, h, W, N, P, ns, gains=gains, d_counts=d_n)
    assert np.array_equal(case.read_counters(d_n, ni), 2 * exp_n)


def test_the_quantiser_on_exact_ties_and_special_gains(case):
    N = 256
    z = np.tile(np.array([1.0, -1.0], dtype=F), (2, 16 * N, 1))
    z[1] *= F(-1.0)
    ones, W = np.ones(N, dtype=F), channeliser.twiddles(N)
    T = model.tensor(model.channelise(z, ones, W, N, 1, 16))
    assert np.all(T[0, 0, 0] == np.array([256.0, -256.0], dtype=F)) and not T[1:].any()
    for y, q, clipped in ((2.5, 2, False), (3.5, 4, False), (-2.5, -2, False), (126.5, 126, False), (127.5, 127, True),
                          (-127.5, -127, True), (0.0, 0, False), (np.inf, 127, True), (np.nan, -128, True)):
        gains = np.full((2, N), y / 256.0, dtype=F)
        exp_q, exp_n = model.quantise(T, gains)
        if np.isfinite(y):
            assert exp_q[0, 0, 0, 0].tolist() == [q, -q] and exp_q[0, 0, 1, 0].tolist() == [-q, q] and not exp_q[1:].any()
            assert exp_n.tolist() == [32 if clipped else 0] * 2
        else:  # 0 * Inf and anything * NaN are NaN: -128 everywhere but (for Inf) in channel 0, and all of it clipped
            assert exp_q[0, 0, 0, 0].tolist() == ([q, -q] if np.isinf(y) else [-128, -128]) and np.all(exp_q[1:] == -128)
            assert exp_n.tolist() == [N * 32] * 2
        d_n = case.counters(2)
        got = case.run(z, ones, W, N, 1, 16, gains=gains, d_counts=d_n)
        assert np.array_equal(got, exp_q), y
        assert np.array_equal(case.read_counters(d_n, 2), exp_n), y


# ---- 3. special values


def test_nan_inf_denormals_and_negative_zeros_go_where_the_network_says(case):
    N, P, ni, ns = 128, 2, 2, 16
    W, h = channeliser.twiddles(N), model.seeded_taps(N, P, seed=8)
    z = model.seeded_input(ni, (ns + P - 1) * N, seed=9)
    z[0, 5 * N + 17, 0] = np.nan   # column 17 of spectra 4 and 5 of input 0, re
    z[1, 9 * N + 3, 1] = np.inf    # column 3 of spectra 8 and 9 of input 1, im
    X = model.channelise(z, h, W, N, P, ns)
    bad = ~np.isfinite(X)
    assert bad[0, 4:6].any(axis=-1).all() and bad[1, 8:10].any(axis=-1).all()  # it reaches every channel of its two spectra
    assert not bad[0, :4].any() and not bad[0, 6:].any() and not bad[1, :8].any() and not bad[1, 10:].any()
    assert np.isnan(X[1, 8:10]).any() and np.isinf(X[1, 8:10]).any()  # Inf - Inf and 0 Inf on the way
    assert window_is(case.run(z, h, W, N, P, ns), model.tensor(X)) is None
    gains = np.ones((ni, N), dtype=F)
    d_n = case.counters(ni)
    exp_q, exp_n = model.quantise(model.tensor(X), gains)
    assert (exp_q == -128).any()
    assert np.array_equal(case.run(z, h, W, N, P, ns, gains=gains, d_counts=d_n), exp_q)
    assert np.array_equal(case.read_counters(d_n, ni), exp_n)
    # tiny inputs: the products, the sums and the outputs are denormals, and kept
    tiny = (model.seeded_input(ni, (ns + P - 1) * N, seed=10) * F(1e-43)).astype(F)
    X = model.channelise(tiny, h, W, N, P, ns)
    denormal = (X != 0) & (np.abs(X) < np.finfo(F).tiny)
    assert denormal.mean() > 0.9
    assert window_is(case.run(tiny, h, W, N, P, ns), model.tensor(X)) is None
    # negative zeros: all of them, and a mixture, through taps of both signs
    signs = 0
    for zz in (np.full((ni, (ns + P - 1) * N, 2), -0.0, dtype=F), np.where(z > 0, F(0.0), F(-0.0)).astype(F)):
        X = model.channelise(zz, h, W, N, P, ns)
        assert not X.any()
        signs += int(np.signbit(X).sum())
        assert window_is(case.run(zz, h, W, N, P, ns), model.tensor(X)) is None
    assert signs > 0  # some zeros of the outputs are negative, and compared as such
    # one tap, positive: every -0.0 stays -0.0 through the FIR, and the sums of the network are of equal zeros
    X = model.channelise(np.full((1, 16 * N, 2), -0.0, dtype=F), np.ones(N, dtype=F), W, N, 1, 16)
    assert np.signbit(X[:, :, 0]).all()
    assert window_is(case.run(np.full((1, 16 * N, 2), -0.0, dtype=F), np.ones(N, dtype=F), W, N, 1, 16), model.tensor(X)) is None


# ---- 4. any table


@pytest.mark.parametrize("N", (64, 512, 2048))
def test_any_table_and_any_taps_are_served(case, N):
    P, ni, ns = 3, 2, 16
    rng = np.random.default_rng(N)
    W = rng.uniform(-1.5, 1.5, size=(N // 2, 2)).astype(F)  # no unit moduli, no symmetry
    W[0], W[N // 4] = np.nan, np.nan
    z, h = model.seeded_input(ni, (ns + P - 1) * N, seed=N + 2), rng.standard_normal(P * N).astype(F)
    X = model.channelise(z, h, W, N, P, ns)
    assert np.isfinite(X).all()
    got = case.run(z, h, W, N, P, ns)
    assert not np.isnan(got).any()
    assert window_is(got, model.tensor(X)) is None


# ---- 5. what needs the context


def test_refusals_enqueue_nothing_and_empty_calls_succeed(case, gpu):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError
    from dc_sand_amd.generator import channelised_bytes

    N, P, ni, ns = 64, 3, 2, 16
    pairs = (ns + P - 1) * N
    z, h, W = model.seeded_input(ni, pairs, seed=4), model.seeded_taps(N, P, seed=5), channeliser.twiddles(N)
    d_in, d_h, d_w = case.upload(z), case.upload(h), case.upload(W)
    obytes = channelised_bytes(N, 1, ni)
    d_out = case.out(obytes)
    g = case.g
    ok = dict(d_in=d_in, in_bytes=z.nbytes, in_stride=pairs, nr_inputs=ni, nr_spectra=ns, nr_channels=N, nr_taps=P, d_taps=d_h,
              d_twiddles=d_w, d_out=d_out, out_bytes=obytes, out_blocks=1, out_inputs=ni)
    bad = [dict(in_bytes=z.nbytes - 1), dict(out_bytes=obytes - 1), dict(d_in=int(d_in) + 4), dict(d_out=int(d_out) + 8),
           dict(d_twiddles=int(d_w) + 4), dict(d_taps=int(d_h) + 2), dict(nr_channels=96), dict(nr_channels=32), dict(nr_taps=0),
           dict(nr_taps=17), dict(nr_spectra=8), dict(order=2), dict(in_stride=pairs - 1), dict(first_block=1), dict(first_input=1),
           dict(d_in=None), dict(d_taps=None), dict(d_twiddles=None), dict(d_out=None), dict(nr_spectra=32)]
    for i, change in enumerate(bad):
        with pytest.raises(DcsError) as e:
            g.channelise(**{**ok, **change})
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    d_g, d_q = case.upload(np.ones((ni, N), dtype=F)), case.out(obytes // 4)
    okq = {**ok, "d_gains": d_g, "d_out_q8": d_q, "out_bytes": obytes // 4}
    del okq["d_out"]
    for i, change in enumerate([dict(d_gains=None), dict(d_gains=int(d_g) + 2), dict(d_clip_count=int(d_g) + 4), dict(out_bytes=obytes // 4 - 1)]):
        with pytest.raises(DcsError) as e:
            g.channelise_q8(**{**okq, **change})
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    g.channelise(**{**ok, "nr_spectra": 0, "d_in": None, "in_bytes": 0})  # nothing to do
    g.channelise(**{**ok, "nr_inputs": 0, "d_in": None, "d_taps": None, "d_twiddles": None})
    g.channelise_q8(**{**okq, "nr_spectra": 0, "d_gains": None})
    gpu.synchronize()
    assert np.all(case.read(d_out) == PREFILL) and np.all(case.read(d_q) == PREFILL)
    g.channelise(**ok)  # the context and the device are as usable as before
    gpu.synchronize()
    got = case.read(d_out, dtype=F, shape=(N, 1, ni, 16, 2))
    assert model.same_bits(got, model.tensor(model.channelise(z, h, W, N, P, ns))) is None


# ---- 6. capture and replay


def test_captured_first_calls_follow_new_input_gains_and_counters_on_replay(gpu):
    """Both calls in one hipGraph as the first calls on a fresh context -- nothing allocates -- replayed with new input and
    new gains in the same buffers and the counters zeroed."""
    from dc_sand_amd.generator import channelised_bytes

    c = ChCase(gpu)
    try:
        N, P, ni, ns = 256, 4, 3, 32
        pairs = (ns + P - 1) * N
        W, h = channeliser.twiddles(N), model.seeded_taps(N, P, seed=21)
        sets = []
        for i in range(3):
            z = model.seeded_input(ni, pairs, seed=30 + i)
            X = model.channelise(z, h, W, N, P, ns, order=1)
            sets.append((z, X, (model.case_gains(X, N) * F(1.0 + 0.25 * i)).astype(F)))
        d_in, d_g, d_n = c.alloc(ni * pairs * 8), c.alloc(ni * N * 4), c.alloc(ni * 8)
        d_h, d_w = c.upload(h), c.upload(W)
        fbytes, qbytes = channelised_bytes(N, ns // 16, ni), channelised_bytes(N, ns // 16, ni, q8=True)
        d_f, d_q = c.out(fbytes), c.out(qbytes)
        s = gpu.Stream()
        with hip_graph.capture(s) as graph:
            c.g.channelise(d_in, ni * pairs * 8, pairs, ni, ns, N, P, d_h, d_w, d_f, fbytes, ns // 16, ni, order=1, stream=s.handle)
            c.g.channelise_q8(d_in, ni * pairs * 8, pairs, ni, ns, N, P, d_h, d_w, d_g, d_q, qbytes, ns // 16, ni, order=1,
                              d_clip_count=d_n, stream=s.handle)
        seen = []
        for i in (1, 2, 0):
            z, X, gains = sets[i]
            gpu.memcpy_htod(d_in, z, stream=s.handle, sync=False)
            gpu.memcpy_htod(d_g, gains, stream=s.handle, sync=False)
            gpu.memset(d_n, 0, ni * 8, stream=s.handle)
            c.refill(d_f, stream=s.handle)
            c.refill(d_q, stream=s.handle)
            graph.launch(s)
            s.synchronize()
            exp_q, exp_n = model.quantise(model.tensor(X), gains)
            assert model.same_bits(c.read(d_f, fbytes, F, (N, ns // 16, ni, 16, 2)), model.tensor(X)) is None, i
            got_q = c.read(d_q, qbytes, np.int8, (N, ns // 16, ni, 16, 2))
            assert np.array_equal(got_q, exp_q), i
            assert np.array_equal(c.read_counters(d_n, ni), exp_n) and exp_n.all(), i
            seen.append(got_q)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
        graph.close()
    finally:
        c.close()


# ---- 7. the chain: down-converter -> channeliser -> correlator, bit for bit against the three models chained


def test_ddc_channelise_q8_correlate_is_the_three_models_chained(gpu):
    from dc_sand_amd.generator import block_visibilities_bytes, channelised_bytes, ddc_digits_bytes, ddc_out_bytes

    N, P, A, ns, T = 64, 2, 3, 32, 64
    nr_out = (ns + P - 1) * N  # the pairs a row of the channeliser reads
    c = ChCase(gpu, C=N, A=A, nt=ns)
    try:
        rng = np.random.default_rng(77)
        x = rng.integers(-128, 128, size=(A, 16 * (nr_out - 1) + T), dtype=np.int8)
        taps = rng.integers(-2000, 2001, size=(1, T, 2))
        bands = [(0x0EF00000, 0x12345678, 2.0 ** -8)]
        y = ddc_model.ddc(x, taps, bands, nr_out)  # [1][A][nr_out][2]
        h, W = channeliser.pfb_taps(N, P), channeliser.twiddles(N)
        X = model.channelise(y[0], h, W, N, P, ns, order=1)
        gains = model.case_gains(X, N)
        ant, _ = model.quantise(model.tensor(X), gains)  # int8 [N][ns / 16][A][16][2]: the sample tensor
        assert np.unique(ant).size > 200
        vis = correlator_model.visibilities(ant, 2)

        d_x, d_taps, d_digits = c.upload(x), c.upload(taps.astype(np.int32)), c.alloc(ddc_digits_bytes(T))
        ybytes, abytes, vbytes = ddc_out_bytes(A, nr_out), channelised_bytes(N, ns // 16, A, q8=True), block_visibilities_bytes(c.bp, ns, 2)
        d_y, d_ant, d_vis = c.out(ybytes), c.out(abytes), c.out(vbytes)
        d_h, d_w, d_g = c.upload(h), c.upload(W), c.upload(gains)
        c.g.ddc_tap_digits(d_taps, T, 1, d_digits, ddc_digits_bytes(T))
        c.g.ddc(d_x, x.nbytes, x.shape[1], A, nr_out, d_digits, ddc_digits_bytes(T), T, bands, d_y, ybytes, nr_out)
        c.g.channelise_q8(d_y, ybytes, nr_out, A, ns, N, P, d_h, d_w, d_g, d_ant, abytes, ns // 16, A, order=1)
        c.g.correlate_block(d_ant, abytes, d_vis, vbytes, ns, 2)
        gpu.synchronize()
        assert np.array_equal(c.read(d_ant, abytes, np.int8, ant.shape), ant)
        assert np.array_equal(c.read(d_vis, vbytes, np.int32, vis.shape), vis)
    finally:
        c.close()


# ---- 8. the example


def test_the_example_verifies_itself(gpu):
    assert "OK" in run_example("f_engine.py", timeout=120)
