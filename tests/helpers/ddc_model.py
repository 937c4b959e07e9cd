"""numpy restatement of the stated arithmetic of include/dcs_ddc.h: the digit split of the taps, the three digit sums in
int64 recombined modulo 2^32, ``dcs_sincos_turn32`` of dc_sand_amd/csrc/bf_math.h operation by operation in fp32, and the
fp32 tail.  tests/test_ddc_model.py anchors it: the sums on Python integers, ``turn32`` bit for bit on the header compiled
for the host and on fp64 ``cos`` / ``sin``, the whole on the reference's ddc.py (tests/golden/ddc/).  The GPU tests compare
the kernel with it bit for bit.

The tolerance against the reference (``reference_tolerance``), per output and on |y_model - y_ref|, is computed from the
fixture, not fixed:

  * the print bound.  The reference filters with the CSV's decimals ``c_j`` and divides by ``sum c``; the model filters with
    the integers ``h_j = rint(c_j 2^17)``.  The numerators differ by at most ``sum_j |c_j 2^17 - h_j| |x[16 m + j]| / sum h``;
    the denominators' ratio ``sum h / (2^17 sum c)`` differs from 1 by the fixture's own figure, times ``|y_ref|``;
  * the tap quantisation.  Each component of ``g[j] = rint(h[j] 2^s e^(-i w j))`` is within 0.5 of its real:
    ``0.5 sum_j |x[16 m + j]| / (sum h 2^s)``.  (That is the bound per component of the sum; the worst case on the modulus is
    sqrt(2) larger.  The test holds the smaller figure.)
  * the float term.  The reference's oscillator (cwg.py) is rounded to complex64, 2^-24 relative per component, so each mixed
    sample is off by at most ``sqrt(2) 2^-24 |x|``: ``sqrt(2) 2^-24 sum_j |h_j| |x[16 m + j]| / sum h`` after the filter; its
    own arithmetic is fp64 (an FFT convolution included: below 10^-12 here, covered by a flat 10^-9).  The model's tail: F =
    RN((float)S) once per component, (c, s) within 2^-22 each, two products, one sum, the product with the gain and the gain's
    own rounding -- ``(|S_re| + |S_im|) gain (2^-22 + 6 2^-24)`` per component, sqrt(2) times that on the modulus.
"""
import numpy as np

F32 = np.float32
PIO2_1 = F32(1.57079637050628662109375)
TURN32_K = PIO2_1 * F32(2.0 ** -30)  # exact scaling of RN(pi / 2)
S1, S2, S3, S4 = (F32(x) for x in (-1.66666671633720397949e-01, 8.33333376795053482056e-03, -1.98412701138295233250e-04,
                                  2.75573142971552442759e-06))
C1, C2, C3, C4 = (F32(x) for x in (4.16666679084300994873e-02, -1.38888892251998186111e-03, 2.48015876422869041562e-05,
                                  -2.75573142971552442759e-07))
MAX_ABS_TAP = 127 * 65793
MAX_ABS_SUM = (1 << 24) - 1


def same_bits(got, exp):
    """None if the float arrays agree bit for bit, else the first differing indices."""
    g, e = np.ascontiguousarray(got, dtype=F32).view(np.uint32), np.ascontiguousarray(exp, dtype=F32).view(np.uint32)
    if g.shape == e.shape and np.array_equal(g, e):
        return None
    return (g.shape, e.shape) if g.shape != e.shape else np.argwhere(g != e)[:4].tolist()


def fma32(a, b, c):
    """fmaf: RN32(a b + c) with ONE rounding.  The product of two fp32 is exact in fp64; the sum is rounded to odd in fp64
    (TwoSum gives its error exactly), and a round-to-odd of 53 >= 2 * 24 + 2 bits followed by RN to 24 bits is RN of the exact
    value."""
    p = np.asarray(a, dtype=F32).astype(np.float64) * np.asarray(b, dtype=F32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, dtype=F32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0.0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


def turn32(u):
    """(sin, cos) float32 of ``u / 2^32`` turns: dcs_sincos_turn32, operation by operation."""
    u = np.asarray(u).astype(np.uint32)
    n = ((u.astype(np.uint64) + (1 << 29)) & 0xFFFFFFFF) >> 30
    r = (u.astype(np.int64) - (n.astype(np.int64) << 30))
    r = ((r + (1 << 31)) % (1 << 32)) - (1 << 31)  # (int32) of the wrapped difference
    assert np.all((r >= -(1 << 29)) & (r < (1 << 29)))
    x = r.astype(F32) * TURN32_K
    s = x * x
    ps = fma32(s, S4, S3)
    ps = fma32(ps, s, S2)
    ps = fma32(ps, s, S1)
    pc = fma32(s, C4, C3)
    pc = fma32(pc, s, C2)
    pc = fma32(pc, s, C1)
    pc = fma32(pc, s, F32(-0.5))
    sr = fma32(s * x, ps, x)
    cr = fma32(s, pc, F32(1.0))
    n = n.astype(np.int64) & 3
    swap, neg = (n & 1) == 1, (n & 2) == 2
    sn = np.where(swap, cr, sr)
    cs = np.where(swap, -sr, cr)
    return np.where(neg, -sn, sn).astype(F32), np.where(neg, -cs, cs).astype(F32)


def split_digits(v):
    """The balanced base-256 digits (d0, d1, d2) int64 of integer taps: ``v = d0 + 256 d1 + 65536 d2`` exactly for
    ``|v| <= 8 355 711``; beyond, the top digit wraps modulo 256."""
    v = np.asarray(v).astype(np.int64)
    d0 = ((v + 128) % 256) - 128
    v1 = (v - d0) // 256
    d1 = ((v1 + 128) % 256) - 128
    v2 = (v1 - d1) // 256
    d2 = ((v2 + 128) % 256) - 128
    return d0, d1, d2


def effective_taps(v):
    """The taps as the digits hold them: ``((v + 8 421 504) mod 2^24) - 8 421 504``."""
    d0, d1, d2 = split_digits(v)
    return d0 + 256 * d1 + 65536 * d2


def windows(x, nr_taps, nr_out):
    """``X[m][j] = x[16 m + j]`` of a row, int64 ``[nr_out][T]``."""
    x = np.asarray(x)
    assert x.dtype == np.int8 and x.ndim == 1 and (nr_out == 0 or x.size >= 16 * (nr_out - 1) + nr_taps)
    idx = 16 * np.arange(nr_out)[:, None] + np.arange(nr_taps)[None, :]
    return x.astype(np.int64)[idx]


def sums_mod32(x, v, nr_out):
    """The words ``S`` int32 ``[nr_out]`` of one row and one tap component ``v`` ``[T]``: the three digit sums, exact in
    int64, combined as s0 + (s1 << 8) + (s2 << 16) modulo 2^32."""
    X = windows(x, len(v), nr_out)
    s0, s1, s2 = (X @ d for d in split_digits(v))
    assert max(np.abs(s).max(initial=0) for s in (s0, s1, s2)) <= 256 * 128 * 128
    w = (s0 + (s1 << 8) + (s2 << 16)) & 0xFFFFFFFF
    return w.astype(np.uint32).view(np.int32)


def phase_words(step, phase0, first_output, nr_out):
    """u(m) = phase0 + 16 (first_output + m) step mod 2^32, on Python integers."""
    return np.array([(int(phase0) + 16 * (int(first_output) + m) * int(step)) % (1 << 32) for m in range(nr_out)], dtype=np.uint32)


def ddc(x, taps, bands, nr_out, first_output=0):
    """The outputs float32 ``[band][input][nr_out][{re, im}]`` of samples int8 ``[input][>= 16 (nr_out - 1) + T]``, taps
    integer ``[band][T][{re, im}]`` and ``bands`` = ``[(phase_step, phase0, gain)]``."""
    x, taps = np.asarray(x), np.asarray(taps)
    assert x.ndim == 2 and taps.ndim == 3 and taps.shape[0] == len(bands) and taps.shape[2] == 2
    out = np.empty((len(bands), x.shape[0], nr_out, 2), dtype=F32)
    for b, (step, phase0, gain) in enumerate(bands):
        sn, cs = turn32(phase_words(step, phase0, first_output, nr_out))
        gain = F32(gain)
        for i in range(x.shape[0]):
            Fre = sums_mod32(x[i], taps[b, :, 0], nr_out).astype(F32)  # RN((float)S)
            Fim = sums_mod32(x[i], taps[b, :, 1], nr_out).astype(F32)
            out[b, i, :, 0] = (Fre * cs + Fim * sn) * gain
            out[b, i, :, 1] = (Fim * cs - Fre * sn) * gain
    return out


def as_complex(y):
    return y[..., 0].astype(np.float64) + 1j * y[..., 1].astype(np.float64)


def reference_tolerance(x, c, h, taps, gain, scale_bits, y_ref):
    """The bound of the module docstring per output, for one row ``x``, the CSV's decimals ``c`` and their integers ``h``
    (both in correlation order), the band's integer ``taps`` ``[T][2]`` and ``gain``, and the reference's outputs."""
    nr_out, T = len(y_ref), len(h)
    X = np.abs(windows(x, T, nr_out)).astype(np.float64)
    hsum = float(np.sum(h))
    c17 = np.asarray(c, dtype=np.float64) * 131072.0
    print_bound = X @ np.abs(c17 - h) / hsum + np.abs(y_ref) * abs(hsum / float(np.sum(c17)) - 1.0)
    quant = 0.5 * X.sum(axis=1) / (hsum * 2.0 ** scale_bits)
    Xs = windows(x, T, nr_out)
    S = np.abs(Xs @ taps[:, 0].astype(np.int64)) + np.abs(Xs @ taps[:, 1].astype(np.int64))
    flt = (np.sqrt(2.0) * 2.0 ** -24 * (X @ np.abs(h).astype(np.float64)) / hsum + 1e-9
           + np.sqrt(2.0) * S * float(gain) * (2.0 ** -22 + 6.0 * 2.0 ** -24))
    return print_bound + quant + flt
