"""Host model of the complex-product beamformer's arithmetic (include/dcs_beam_complex.h), restated
from the header's contract in numpy alone on top of helpers/beamformer_model.py: no GPU, no import of the product.

    F_re = fixed(w_re)        F_ip = fixed(sigma * w_im)        F_in = fixed(-sigma * w_im)        sigma = -1: conjugate
    out_re:  S_d = sum_a digit_d(F_re) * x_re + digit_d(F_in) * x_im        d = 1, 2, 3
    out_im:  S_d = sum_a digit_d(F_re) * x_im + digit_d(F_ip) * x_re
    tail  :  low = RN32(S2 * 256 + S3);  f = RN32(S1 * 65536 + low);  v = RN32(f * inv)   (or * RN32(s_b * inv))

The digits of F_in are those of the negated NUMBER, not the negated digits of F_ip.  Tensors as beamformer_model's:
coefficients fp32 [C][A][B][2], samples int8 [C][nT16][A][16][2], beams fp32 [C][nT16][B][16][2]."""
import numpy as np

from helpers.beamformer_model import F32, INV, digits, fixed

SUM_BOUND = 2 ** 23  # |S_d| <= 2 products * 256 antennas * 128 * 128


def operands(coef, conjugate=False):
    """(F_re, F_ip, F_in), each int64 [C][A][B]: fixed() of the fp32 numbers w_re, sigma * w_im and -sigma * w_im themselves
    (negating an fp32 number is exact)."""
    coef = np.asarray(coef)
    assert coef.dtype == F32 and coef.ndim == 4 and coef.shape[3] == 2
    im = -coef[..., 1] if conjugate else coef[..., 1]
    return fixed(coef[..., 0]), fixed(im), fixed(-im)


def _contract(d, xk):
    """sum_a d[c][a][b] * xk[c][t][a][i] as int64 [C][nT16][B][16]: in float64 (BLAS), where every product and partial sum
    is an integer below 2^53, hence exact whatever the order."""
    w = np.ascontiguousarray(d.transpose(0, 2, 1)).astype(np.float64)[:, None]  # [C][1][B][A]
    return np.matmul(w, np.ascontiguousarray(xk)).astype(np.int64)


def digit_sums(coef, x, conjugate=False):
    """The integer sums (S1, S2, S3), each int64 [C][nT16][B][16][2]."""
    assert x.dtype == np.int8 and x.ndim == 5 and x.shape[3] == 16 and x.shape[4] == 2
    C, A, B, _ = coef.shape
    assert x.shape[0] == C and x.shape[2] == A
    F_re, F_ip, F_in = operands(coef, conjugate)
    xr, xi = x[..., 0].astype(np.float64), x[..., 1].astype(np.float64)
    out = []
    for d_re, d_ip, d_in in zip(digits(F_re), digits(F_ip), digits(F_in)):
        s = np.empty((C, x.shape[1], B, 16, 2), dtype=np.int64)
        s[..., 0] = _contract(d_re, xr) + _contract(d_in, xi)
        s[..., 1] = _contract(d_re, xi) + _contract(d_ip, xr)
        assert np.all(np.abs(s) <= SUM_BOUND)
        out.append(s)
    return out


def low_part(s2, s3):
    """fmaf((float)s2, 256.0f, (float)s3): both conversions exact (|s| <= 2^23 < 2^24), the product and the sum exact in
    float64 (an integer below 2^33), one rounding to fp32."""
    s2, s3 = np.asarray(s2, dtype=np.int64), np.asarray(s3, dtype=np.int64)
    assert np.all(np.abs(s2) <= SUM_BOUND) and np.all(np.abs(s3) <= SUM_BOUND)
    a, b = s2.astype(F32), s3.astype(F32)
    assert np.all(a.astype(np.int64) == s2) and np.all(b.astype(np.int64) == s3)
    return (a.astype(np.float64) * 256.0 + b.astype(np.float64)).astype(F32)


def recombine(s1, s2, s3, scale=None):
    """The fp32 tail with the fma form of the low part."""
    assert np.all(np.abs(s1) <= SUM_BOUND)
    low32 = low_part(s2, s3)
    # the fma in float64: s1 * 65536 (< 2^40) and low32 (an integer below 2^33) add exactly there; one rounding to fp32
    f = (np.asarray(s1).astype(np.float64) * 65536.0 + low32.astype(np.float64)).astype(F32)
    if scale is None:
        return (f * INV).astype(F32)
    with np.errstate(invalid="ignore"):
        fac = (np.asarray(scale, dtype=F32) * INV).astype(F32)  # [B]
        return (f * fac[None, None, :, None, None]).astype(F32)


def complex_model(coef, x, conjugate=False, scale=None):
    """dcs_bf_beamform_accumulated_complex.  coef: the (weighted: w' = RN32(ghat * w)) coefficients; a beam with a
    non-finite coefficient in either component (any channel's row of its own) is NaN in both planes."""
    coef = np.asarray(coef, dtype=F32)
    bad = ~np.isfinite(coef).all(axis=(1, 3))  # [C][B]
    v = recombine(*digit_sums(np.where(np.isfinite(coef), coef, F32(0)), x, conjugate), scale=scale)
    v[np.broadcast_to(bad[:, None, :, None, None], v.shape)] = np.nan
    return v
