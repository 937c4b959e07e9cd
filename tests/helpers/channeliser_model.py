"""numpy restatement of the stated arithmetic of include/dcs_channeliser.h, vectorised, in float32: the FIR with the taps in
order, the bit reversal, the log2 N stages of the butterfly network with the caller's table (entries 0 and N / 4 never used),
the channel order, the sample tensor's layout and the quantiser of include/dcs_beam_quant.h.  numpy multiplies and adds
float32 arrays with one rounding each and contracts nothing, and keeps denormals.  tests/test_channeliser_model.py anchors it
on a scalar loop, on the exact transform in fp64 and on exact cases; the GPU tests compare the kernels with it bit for bit.
"""
import numpy as np

F32 = np.float32


def same_bits(got, exp):
    """None if the float arrays agree -- two NaNs agree, everything else bit for bit, signed zeros included -- else the
    first differing indices."""
    g, e = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(exp, dtype=F32)
    if g.shape != e.shape:
        return (g.shape, e.shape)
    differ = (g.view(np.uint32) != e.view(np.uint32)) & ~(np.isnan(g) & np.isnan(e))
    return np.argwhere(differ)[:4].tolist() if differ.any() else None


def bitrev(N):
    L = N.bit_length() - 1
    i = np.arange(N)
    r = np.zeros(N, dtype=np.int64)
    for b in range(L):
        r |= ((i >> b) & 1) << (L - 1 - b)
    return r


def fir(z, h, N, P, nr_spectra):
    """z float32 [inputs][>= (nr_spectra + P - 1) N][2], h float32 [P N] -> y float32 [inputs][nr_spectra][N][2]."""
    z = np.asarray(z, dtype=F32)
    h = np.asarray(h, dtype=F32).reshape(P, N)
    rows = z[:, :(nr_spectra + P - 1) * N].reshape(z.shape[0], nr_spectra + P - 1, N, 2)
    with np.errstate(all="ignore"):
        y = h[0][None, None, :, None] * rows[:, 0:nr_spectra]
        for p in range(1, P):
            y = y + h[p][None, None, :, None] * rows[:, p:p + nr_spectra]
    return y


def network(y, W):
    """y float32 [..., N, 2], W float32 [N / 2][2] -> X float32 [..., N, 2], bin k at index k."""
    y = np.asarray(y, dtype=F32)
    W = np.asarray(W, dtype=F32)
    N = y.shape[-2]
    lead = y.shape[:-2]
    v = y[..., bitrev(N), :].copy()
    m = 1
    with np.errstate(all="ignore"):
        while m < N:
            g = v.reshape(lead + (N // (2 * m), 2, m, 2))
            a, b = g[..., 0, :, :], g[..., 1, :, :]
            q = np.arange(m) * (N // (2 * m))
            wr, wi = W[q, 0], W[q, 1]
            t = np.empty_like(b)
            t[..., 0] = wr * b[..., 0] - wi * b[..., 1]
            t[..., 1] = wr * b[..., 1] + wi * b[..., 0]
            t[..., 0, :] = b[..., 0, :]  # j == 0: no arithmetic
            if m >= 2:                   # q == N / 4 at j == m / 2: no arithmetic
                t[..., m // 2, 0] = b[..., m // 2, 1]
                t[..., m // 2, 1] = -b[..., m // 2, 0]
            v = np.stack([a + t, a - t], axis=-3).reshape(lead + (N, 2))
            m *= 2
    return v


def channelise(z, h, W, N, P, nr_spectra, order=0):
    """The float call's values as X float32 [inputs][nr_spectra][N][2], output channel c at index c."""
    X = network(fir(z, h, N, P, nr_spectra), W)
    return np.roll(X, N // 2, axis=2) if order else X


def tensor(X):
    """[inputs][nr_spectra][N][2] -> the output tensor [N][nr_spectra / 16][inputs][16][2] of a call that fills it."""
    ni, ns, N, _ = X.shape
    return np.ascontiguousarray(X.reshape(ni, ns // 16, 16, N, 2).transpose(3, 1, 0, 2, 4))


def quantise(T, gains):
    """T float32 [N][blocks][inputs][16][2], gains float32 [inputs][N] -> (int8 of T's shape, uint64 [inputs] clipped
    components): y = RN(T gain); NaN -> -128; otherwise clamp(rint(y), -127, 127); clipped when NaN or |rint(y)| > 127."""
    T = np.asarray(T, dtype=F32)
    k = np.asarray(gains, dtype=F32).T[:, None, :, None, None]
    with np.errstate(all="ignore"):
        y = (T * k).astype(F32)
        r = np.rint(y)
        nan = np.isnan(y)
        clipped = nan | (np.abs(r) > F32(127.0))
        q = np.where(nan, F32(-128.0), np.clip(r, F32(-127.0), F32(127.0))).astype(np.int8)
    return q, clipped.sum(axis=(0, 1, 3, 4)).astype(np.uint64)


def exact(z, h, N, P, nr_spectra):
    """The exact FIR in fp64 and numpy's fp64 FFT: complex128 [inputs][nr_spectra][N], and the bound's M =
    sum_{p, r} |h[p N + r]| |z[(n + p) N + r]| per (input, spectrum)."""
    zc = np.asarray(z, dtype=np.float64)
    zc = (zc[..., 0] + 1j * zc[..., 1])[:, :(nr_spectra + P - 1) * N].reshape(zc.shape[0], nr_spectra + P - 1, N)
    hh = np.asarray(h, dtype=np.float64).reshape(P, N)
    y = sum(hh[p][None, None, :] * zc[:, p:p + nr_spectra] for p in range(P))
    M = sum(np.abs(hh[p])[None, None, :] * np.abs(zc[:, p:p + nr_spectra]) for p in range(P)).sum(axis=2)
    return np.fft.fft(y, axis=2), M


def bound(N, P, M):
    """(P + 5 log2 N) 2^-24 1.01 M: DESIGN.md section 5.21."""
    return (P + 5 * (N.bit_length() - 1)) * 2.0 ** -24 * 1.01 * M


def seeded_input(ni, pairs, seed, stride_pad=0):
    """Seeded integers in [-2000, 2000] as float32 [ni][pairs + stride_pad][2]; the padding holds other data than the rows."""
    rng = np.random.default_rng(seed)
    return rng.integers(-2000, 2001, size=(ni, pairs + stride_pad, 2)).astype(F32)


def seeded_taps(N, P, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=P * N).astype(F32)


def case_gains(X, N):
    """The gains of the quantised GPU cases: g0 (1 + (c mod 7) / 8) for every input, g0 = 64 / rms of the float output X."""
    rms = float(np.sqrt(np.mean(np.asarray(X, dtype=np.float64) ** 2)))
    g = (64.0 / rms) * (1.0 + (np.arange(N) % 7) / 8.0)
    return np.broadcast_to(g.astype(F32), (X.shape[0], N)).copy()
