"""Inputs that take the complex-product beamformer (include/dcs_beam_complex.h) to the edge its fma
low part exists for: S2 * 256 + S3 beyond int32.  Pure numpy on top of helpers/beamformer_model.py and
helpers/beam_complex_model.py: no GPU, no import of the product.

With every sample -128, low = S2 * 256 + S3 = 128 * (256 * P2 + P3), P_d the sum of -digit_d over the 2 * A operand digits
that meet in a plane.  Leaving int32 needs 256 * P2 + P3 >= 2^24 at A = 256: the 512 middle digits may fall short of -128
by 255 in total at the most, and P3 has to make up 256 times that shortfall.

Unweighted this is out of reach: a unit-modulus coefficient never has the middle digit -128 in both components (F_re^2 +
F_im^2 = K^2 +- O(K) with both F an odd multiple of 32768 plus at most 128 has no solution), so every antenna falls short by
1 at least, 256 in total; tests/test_beam_complex_edges_inputs.py checks both statements over 10^7 phases.  (The negative
side cannot leave int32 whatever the inputs: 127 * 128 < 2^14.)

Weighted it is within reach.  s_b = max_a |g| makes one antenna's ghat +-1, a unit-modulus coefficient that falls short;
the other antennas take any |ghat| < 1:

  * antenna 0, weight 1, at the constant phase PHASE_0: cos has the digits (d1, -128, d3 in [-100, -28]), sin a middle digit
    <= -40 -- (69, -128, -94) and (108, -119, -35) with numpy's cos / sin, a shortfall of 9.  The margins on the low digits
    keep a coefficient one ULP off (half a unit of F) on the same middle digits;
  * antennas 1 .. A - 1, one weight g each, at the constant phase PHASE_REST = fp32(pi / 4): g is the first fp32 value from
    G_FROM upward for which fixed(RN32(g * w)) has the digits (d1, -128, d3 <= -110) in both components of every one of
    these coefficients -- about 110 of the G_SPAN consecutive values do; the first is 0.90397966 with numpy's cos / sin.

With 256 antennas and all samples -128 the model then has S2 = 8387456, S3 = 8372352, low = 2155561088 = 2^31 + 8077440 in
the im plane (the re plane with the conjugate flag); the value there is -41904.375, and the int32 form of the low part,
2^32 too low, would make it -42418.387.  The other plane stays just inside int32 (2139397504).  Which g does it depends on
the very bits of the coefficients, so wrap_gains looks for it in the bits it is given -- on the GPU those of the generator,
known at run time only."""
import numpy as np

from helpers import beam_complex_model
from helpers.beam_complex_model import complex_model
from helpers.beamformer_model import F32, digits, fixed

PHASE_0 = F32(1.0036209)
PHASE_REST = F32(np.pi / 4)
G_FROM = F32(0.9)
G_SPAN = 400000  # consecutive fp32 values scanned from G_FROM upward
INT32_MAX = 2 ** 31 - 1


def phases(A):
    """fPhase_rad per antenna of the wrap table (every beam the same): [A] fp32."""
    p = np.full(A, PHASE_REST, dtype=F32)
    p[0] = PHASE_0
    return p


def standin_coefficients(C, A, B):
    """What a generator within 1 ULP makes of a table with phases(A) and nothing else: numpy's cos / sin, [C][A][B][2]."""
    p = phases(A).astype(np.float64)
    w = np.stack([np.cos(p), np.sin(p)], axis=-1).astype(F32)  # [A][2]
    return np.ascontiguousarray(np.broadcast_to(w[None, :, None, :], (C, A, B, 2)))


def _first_antenna(coef, b):
    """Raises unless antenna 0 of beam b meets the digit conditions in every channel."""
    _, re2, re3 = digits(fixed(coef[:, 0, b, 0]))
    _, im2, _ = digits(fixed(coef[:, 0, b, 1]))
    if not (np.all(re2 == -128) and np.all((re3 >= -100) & (re3 <= -28))):
        raise ValueError(f"beam {b}, antenna 0: cos must have the low digits (-128, -100 .. -28), has ({re2.tolist()}, {re3.tolist()}) "
                         "-- change the inputs (PHASE_0)")
    if not np.all(im2 <= -40):
        raise ValueError(f"beam {b}, antenna 0: sin must have a middle digit <= -40, has {im2.tolist()} -- change the inputs (PHASE_0)")


def _scan(values):
    """The first fp32 g from G_FROM upward with digits (d1, -128, <= -110) of fixed(RN32(g * w)) for every w of values."""
    g = (np.arange(G_SPAN, dtype=np.uint32) + G_FROM.view(np.uint32)).view(F32)
    assert g[0] == G_FROM and np.all(g < 1)
    hit = np.ones(G_SPAN, dtype=bool)
    for w in values:
        _, d2, d3 = digits(fixed((g * F32(w)).astype(F32)))
        hit &= (d2 == -128) & (d3 <= -110)
    idx = np.flatnonzero(hit)
    return (F32(g[idx[0]]), idx.size) if idx.size else (None, 0)


def wrap_gains(coef, beams):
    """{beam: g} for the beams to drive, from the coefficient bits coef [C][A][B][2] of the wrap table."""
    coef = np.asarray(coef)
    assert coef.dtype == F32 and coef.ndim == 4 and coef.shape[3] == 2 and coef.shape[1] >= 2
    out = {}
    for b in beams:
        _first_antenna(coef, b)
        rest = np.unique(coef[:, 1:, b, :])
        if rest.size > 8 or np.any(rest <= 0):
            raise ValueError(f"beam {b}: antennas 1 .. A - 1 must share a few positive coefficient values, have {rest.size} in "
                             f"[{rest.min()!r}, {rest.max()!r}] -- change the inputs (PHASE_REST)")
        g, n = _scan(rest)
        if g is None:
            raise ValueError(f"beam {b}: none of the {G_SPAN} fp32 weights from {G_FROM!r} upward gives the coefficients {rest.tolist()} "
                             "the digits (d1, -128, <= -110) -- change the inputs (G_FROM, G_SPAN)")
        out[b] = g
    return out


def wrap_weights(coef, beams, sign=1.0):
    """Weights [B][A] fp32: sign * (1, g, g, ..., g) in the beams to drive (s_b = 1, ghat the weights themselves), 1 elsewhere."""
    B, A = coef.shape[2], coef.shape[1]
    w = np.ones((B, A), dtype=F32)
    for b, g in wrap_gains(coef, beams).items():
        w[b, 0], w[b, 1:] = F32(sign), F32(sign) * g
    return w


def exact_low(s2, s3):
    """S2 * 256 + S3 itself (int64)."""
    return np.asarray(s2, dtype=np.int64) * 256 + np.asarray(s3, dtype=np.int64)


def int32_low_part(s2, s3):
    """(float)(s2 * 256 + s3) in int32 arithmetic, wrapping as the device's would: the element-wise kernels' form, which
    the complex kernels must NOT use.  The tests use it only to show that the two forms differ at the chosen inputs."""
    low = exact_low(s2, s3)
    wrapped = ((low + 2 ** 31) % 2 ** 32) - 2 ** 31
    return wrapped.astype(np.int32).astype(F32)


def int32_model(coef, x, conjugate=False, scale=None):
    """complex_model with int32_low_part in place of low_part, and nothing else changed."""
    saved = beam_complex_model.low_part
    beam_complex_model.low_part = int32_low_part
    try:
        return complex_model(coef, x, conjugate, scale=scale)
    finally:
        beam_complex_model.low_part = saved
