"""The numpy model of the polyphase channeliser (helpers/channeliser_model.py; include/dcs_channeliser.h), anchored three ways
-- on a scalar loop over np.float32 that follows the header's steps literally, on the exact FIR and FFT in fp64 within the
stated bound, and on cases whose result is known exactly -- and the host-only design functions of dc_sand_amd/channeliser.py.
No GPU and no built library needed."""
import numpy as np
import pytest

from dc_sand_amd import channeliser
from helpers import channeliser_model as model

F = np.float32


def scalar_channelise(z, h, W, N, P, nr_spectra):
    """The five steps of the header for one input, one np.float32 operation at a time: [nr_spectra][N][2]."""
    L = N.bit_length() - 1
    out = np.empty((nr_spectra, N, 2), dtype=F)
    with np.errstate(all="ignore"):
        for n in range(nr_spectra):
            y = []
            for r in range(N):  # 1. the FIR, taps in order
                acc = [F(h[r]) * F(z[n * N + r][0]), F(h[r]) * F(z[n * N + r][1])]
                for p in range(1, P):
                    zz = z[(n + p) * N + r]
                    acc = [F(acc[0] + F(h[p * N + r]) * F(zz[0])), F(acc[1] + F(h[p * N + r]) * F(zz[1]))]
                y.append(acc)
            v = [y[int(format(i, f"0{L}b")[::-1], 2)] for i in range(N)]  # 2. the permutation
            for s in range(1, L + 1):  # 3. the stages
                m = 1 << (s - 1)
                for g in range(0, N, 2 * m):
                    for j in range(m):
                        a, b = v[g + j], v[g + j + m]
                        q = j * N // (2 * m)
                        if j == 0:
                            t = [b[0], b[1]]
                        elif q == N // 4:
                            t = [b[1], -b[0]]
                        else:
                            wr, wi = F(W[q][0]), F(W[q][1])
                            t = [F(F(wr * b[0]) - F(wi * b[1])), F(F(wr * b[1]) + F(wi * b[0]))]
                        v[g + j] = [F(a[0] + t[0]), F(a[1] + t[1])]
                        v[g + j + m] = [F(a[0] - t[0]), F(a[1] - t[1])]
            out[n] = np.array(v, dtype=F)  # 4. X[k] = v[k]
    return out


@pytest.mark.parametrize("P", (1, 3))
def test_the_model_is_the_scalar_loop_bit_for_bit(P):
    N, ns = 64, 16
    rng = np.random.default_rng(P)
    z = rng.standard_normal(((ns + P - 1) * N, 2)).astype(F)
    h = model.seeded_taps(N, P, seed=10 + P)
    W = rng.uniform(-1.0, 1.0, size=(N // 2, 2)).astype(F)  # any table
    W[0], W[N // 4] = np.nan, np.nan                         # and its two entries that are never used
    got = model.channelise(z[None], h, W, N, P, ns)[0]
    assert not np.isnan(got).any()
    assert model.same_bits(got, scalar_channelise(z, h, W, N, P, ns)) is None
    assert model.same_bits(model.channelise(z[None], h, W, N, P, ns, order=1)[0], np.roll(got, N // 2, axis=1)) is None


def test_same_bits_tells_zeros_apart_and_lets_nans_agree():
    a = np.array([0.0, np.nan, 1.0], dtype=F)
    assert model.same_bits(a, a.copy()) is None
    assert model.same_bits(a, np.array([-0.0, np.nan, 1.0], dtype=F)) == [[0]]
    b = a.copy()
    b.view(np.uint32)[1] ^= 1  # another payload
    assert model.same_bits(a, b) is None
    assert model.same_bits(a, np.array([0.0, 1.0, 1.0], dtype=F)) == [[1]]


@pytest.mark.parametrize("N,P", ((64, 1), (64, 16), (256, 4), (1024, 8), (2048, 16)))
def test_the_model_is_the_exact_transform_within_the_bound(N, P):
    ns = 16
    z = np.random.default_rng(N + P).standard_normal((1, (ns + P - 1) * N, 2)).astype(F)
    h, W = channeliser.pfb_taps(N, P), channeliser.twiddles(N)
    X = model.channelise(z, h, W, N, P, ns)
    E, M = model.exact(z, h, N, P, ns)
    err = np.abs((X[..., 0].astype(np.float64) + 1j * X[..., 1].astype(np.float64)) - E)
    ratio = float((err / model.bound(N, P, M)[..., None]).max())
    print(f"N = {N}, P = {P}: largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    # a wrong twiddle index passes the bound by orders of magnitude
    wrong = model.network(model.fir(z, h, N, P, ns), np.roll(W, 1, axis=0))
    err = np.abs((wrong[..., 0].astype(np.float64) + 1j * wrong[..., 1].astype(np.float64)) - E)
    assert float((err / model.bound(N, P, M)[..., None]).max()) > 100.0


def test_a_constant_input_gives_n_times_it_in_channel_0_exactly():
    N = 256
    z = np.tile(np.array([3.0, -5.0], dtype=F), (1, 16 * N, 1))
    X = model.channelise(z, np.ones(N, dtype=F), channeliser.twiddles(N), N, 1, 16)
    assert np.all(X[0, :, 0] == np.array([768.0, -1280.0], dtype=F))
    assert not X[0, :, 1:].any()  # every other channel is exactly zero
    X1 = model.channelise(z, np.ones(N, dtype=F), channeliser.twiddles(N), N, 1, 16, order=1)
    assert np.all(X1[0, :, N // 2] == np.array([768.0, -1280.0], dtype=F)) and not np.delete(X1[0], N // 2, axis=1).any()


@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("N,P,k0", ((64, 4, 5), (256, 8, 200), (1024, 2, 512)))
def test_a_tone_peaks_in_its_channel(N, P, k0, order):
    ns = 16
    t = np.arange((ns + P - 1) * N)
    ang = 2.0 * np.pi * ((k0 * t) % N) / N
    z = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(F)[None]
    X = model.channelise(z, channeliser.pfb_taps(N, P), channeliser.twiddles(N), N, P, ns, order)
    power = (X.astype(np.float64) ** 2).sum(axis=3)[0]
    assert np.all(power.argmax(axis=1) == channeliser.channel_of(k0, N, order))
    assert np.all(power.max(axis=1) > 0.9)  # sum h = 1: the tone comes out with the amplitude it went in with


def test_a_series_cut_at_a_block_is_one_call():
    N, P, ns = 128, 5, 48
    z = model.seeded_input(2, (ns + P - 1) * N, seed=3)
    h, W = model.seeded_taps(N, P, seed=4), channeliser.twiddles(N)
    whole = model.channelise(z, h, W, N, P, ns)
    for cut in (16, 32):
        a = model.channelise(z[:, :(cut + P - 1) * N], h, W, N, P, cut)
        b = model.channelise(z[:, cut * N:], h, W, N, P, ns - cut)  # the last (P - 1) N pairs presented again
        assert model.same_bits(np.concatenate([a, b], axis=1), whole) is None
    T = model.tensor(whole)
    assert T.shape == (N, ns // 16, 2, 16, 2) and model.same_bits(T[7, 2, 1, 5], whole[1, 37, 7]) is None


def exact_ties():
    """The exact case with z = (1, -1) / N scaled so that X[0] = (v, -v) for v in the list: (gains, expected bytes, clipped)."""
    return [(2.5, 2, False), (3.5, 4, False), (-2.5, -2, False), (126.5, 126, False), (127.5, 127, True), (-127.5, -127, True)]


def test_the_quantiser_on_exact_ties():
    N = 256
    z = np.tile(np.array([1.0, -1.0], dtype=F), (1, 16 * N, 1))
    T = model.tensor(model.channelise(z, np.ones(N, dtype=F), channeliser.twiddles(N), N, 1, 16))  # X[0] = (256, -256), else 0
    assert np.all(T[0, 0, 0] == np.array([256.0, -256.0], dtype=F))
    for y, q, clipped in exact_ties():
        gains = np.full((1, N), y / 256.0, dtype=F)  # exact: y is a multiple of 1/2 and 256 a power of two
        got, n = model.quantise(T, gains)
        assert np.all(got[0, 0, 0] == np.array([q, -q], dtype=np.int8)), y
        assert not got[1:].any()
        assert int(n[0]) == (32 if clipped else 0), y  # 16 spectra, re and im counted separately


def test_the_quantiser_on_nan_and_on_special_gains():
    T = np.zeros((64, 1, 1, 16, 2), dtype=F)
    T[0, 0, 0, :, 0], T[0, 0, 0, :, 1] = 5.0, -7.0
    T[1, 0, 0, 3, 0] = np.nan
    T[2, 0, 0, 0] = (np.inf, -np.inf)
    one = np.ones((1, 64), dtype=F)
    q, n = model.quantise(T, one)
    assert q[1, 0, 0, 3, 0] == -128 and (q == -128).sum() == 1  # NaN -> -128 and nothing else
    assert q[2, 0, 0, 0].tolist() == [127, -127]
    assert int(n[0]) == 3  # the NaN and both infinities
    q, n = model.quantise(T, 0.0 * one)  # gain 0: zeros; 0 * NaN and 0 * Inf are NaN
    assert not q[0].any() and q[1, 0, 0, 3, 0] == -128 and q[2, 0, 0, 0].tolist() == [-128, -128] and int(n[0]) == 3
    q, n = model.quantise(T, np.inf * one)  # gain Inf: +-127, and -128 where the value is 0
    assert np.all(q[0, 0, 0, :, 0] == 127) and np.all(q[0, 0, 0, :, 1] == -127)
    assert np.all(q[3:] == -128) and int(n[0]) == T.size
    q, n = model.quantise(T, np.nan * one)  # gain NaN: -128
    assert np.all(q == -128) and int(n[0]) == T.size
    gains = one.copy()
    gains[0, 0] = 2.0  # indexed by the output channel
    q, _ = model.quantise(T, gains)
    assert q[0, 0, 0, 0].tolist() == [10, -14]


# ---- the design functions


@pytest.mark.parametrize("N,P", ((64, 1), (64, 16), (512, 4), (2048, 16)))
def test_pfb_taps(N, P):
    h = channeliser.pfb_taps(N, P)
    assert h.dtype == F and h.shape == (P * N,)
    assert np.array_equal(h, h[::-1])  # symmetric, bit for bit
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= P * N * 2.0 ** -24
    i = np.arange(P * N, dtype=np.float64)
    ref = np.hanning(P * N) * np.sinc((i - (P * N - 1) / 2.0) / N)
    ref /= ref.sum()
    assert np.allclose(h, ref, rtol=0, atol=2.0 ** -24 * np.abs(ref).max())  # one rounding to fp32, and the symmetrising
    assert h.argmax() in (P * N // 2 - 1, P * N // 2)
    if P == 1:  # the normalised window: no lobe, every tap non-negative
        assert np.all(h >= 0) and h[0] == 0 and h[-1] == 0
        wide = channeliser.pfb_taps(N, 1, w_cutoff=1e-6)  # the sinc as good as 1: the Hann window over its sum
        assert np.allclose(wide, np.hanning(N) / np.hanning(N).sum(), rtol=0, atol=1e-8)  # sinc(x) >= 1 - 2 x^2: x <= 5e-7


@pytest.mark.parametrize("N", (64, 128, 256, 512, 1024, 2048))
def test_twiddles(N):
    w = channeliser.twiddles(N)
    assert w.dtype == F and w.shape == (N // 2, 2)
    ang = 2.0 * np.pi * np.arange(N // 2) / N
    ref = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(F)
    keep = np.ones(N // 2, dtype=bool)
    keep[[0, N // 4]] = False
    assert np.array_equal(w[keep].view(np.uint32), ref[keep].view(np.uint32))
    assert w[0].tolist() == [1.0, 0.0] and w[N // 4].tolist() == [0.0, -1.0]
    assert np.signbit(w[0, 1]) == False and np.signbit(w[N // 4, 0]) == False  # noqa: E712


def test_channel_of():
    assert channeliser.channel_of(5, 64) == 5 and channeliser.channel_of(5, 64, 1) == 37
    assert channeliser.channel_of(-1, 64) == 63 and channeliser.channel_of(-1, 64, 1) == 31
    assert channeliser.channel_of(np.arange(-32, 32), 64, 1).tolist() == list(range(64))  # ascending in frequency


def test_bad_arguments_raise():
    for N in (0, 32, 63, 96, 4096, 64.5):
        with pytest.raises(ValueError):
            channeliser.twiddles(N)
        with pytest.raises(ValueError):
            channeliser.pfb_taps(N, 4)
        with pytest.raises(ValueError):
            channeliser.channel_of(0, N)
    for P in (0, 17, -1, 2.5):
        with pytest.raises(ValueError):
            channeliser.pfb_taps(64, P)
    for w in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            channeliser.pfb_taps(64, 4, w_cutoff=w)
    with pytest.raises(ValueError):
        channeliser.channel_of(0, 64, order=2)
    with pytest.raises(ValueError):
        channeliser.channel_of(0.5, 64)


# ---- what the GPU tests run of the kernel's instantiations (dc_sand_amd/csrc/bf_channeliser.hip), read from its text


def kernel_text():
    from pathlib import Path

    return (Path(__file__).resolve().parent.parent / "dc_sand_amd" / "csrc" / "bf_channeliser.hip").read_text()


def test_the_gpu_parametrisations_run_all_twelve_instantiations():
    """One kernel per log2 N and per epilogue, and every int8 epilogue has a lane map of its own, made when compiling: the
    GPU tests that hold an output to this model on seeded data must run each of the twelve."""
    import re

    from helpers import channeliser_cases as cc

    cases = re.findall(r"case (\d+)u: return q \? launch<(\d+), true>\(a, stream\) : launch<(\d+), false>\(a, stream\);", kernel_text())
    assert len(cases) == 6 and all(1 << int(L) == int(N) and L == L2 for N, L, L2 in cases)
    every = {(int(L), q) for _, L, _ in cases for q in (False, True)}
    assert len(every) == 12 and cc.instantiations() == every, sorted(every - cc.instantiations())
    # the test's own condition on the model holds for every quantised case: checked there before the GPU is looked at


def test_the_large_tensor_test_walks_items_beyond_the_grid():
    """The launcher caps the grid at kGrid workgroups, which walk the items beyond: tests/test_gpu_channeliser_large.py has
    262145 items, so that walk is run.  The item count is restated from the launcher's text."""
    import re

    from helpers import channeliser_large as cl

    text = kernel_text()
    grid = 1 << int(re.search(r"constexpr uint32_t kGrid = 1u << (\d+);", text).group(1))
    for line in ("constexpr int total_bits(int L) { return L == 6 ? 12 : L == 11 ? 14 : 13; }",
                 "constexpr int spectra_bits(int L) { return total_bits(L) - L < 4 ? total_bits(L) - L : 4; }",
                 "constexpr uint32_t IG = 1u << (LT - L - LS);",
                 "a.groups = (a.nr_inputs + IG - 1u) / IG;",
                 "a.items = (uint64_t)(a.nr_spectra / 16u) * a.groups * (16u >> LS);",
                 "dim3((uint32_t)(a.items < kGrid ? a.items : kGrid))"):
        assert text.count(line) == 1, line
    L = cl.N.bit_length() - 1
    LT = 12 if L == 6 else 14 if L == 11 else 13
    LS = min(LT - L, 4)
    IG = 1 << (LT - L - LS)
    items = (cl.NR_SPECTRA // 16) * ((cl.NI + IG - 1) // IG) * (16 >> LS)
    assert (grid, items) == (65536, 262145) and items > grid and items % grid != 0
