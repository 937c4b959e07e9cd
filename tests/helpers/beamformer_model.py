"""Host models of the two beamformers' arithmetic, restated from the headers' contracts (include/dcs_beamformer.h,
include/dcs_beam_weights.h, the comment above fixed_word in dc_sand_amd/csrc/bf_beamform_mfma.hip) in numpy alone: no GPU,
no import of the product.  Given the exact bits of the fp32 coefficients a call used, everything a beamformer does after
the coefficient is integer arithmetic or single fp32 operations, which numpy reproduces bit for bit.

Tensors: coefficients fp32 [C][A][B][2] (one time) or [nt][C][A][B][2] (the generator's output order), samples int8
[C][nT16][A][16][2], beams fp32 [C][nT16][B][16][2]; plane 0 = (cos, re), plane 1 = (sin, im), the reference's
element-wise product."""
import numpy as np

F32 = np.float32
FIX_SCALE = 8355711  # 0x7F7F7F: the largest three-digit number with digits in [-128, 127] is 127 * 65793
INV = F32(1.0) / F32(FIX_SCALE)  # RN32(1 / 8355711f): numpy's fp32 divide is correctly rounded


def fixed(w):
    """rint(clip(RN32(w * 8355711f), -8355711, 8355711)) as int64, ties to even.  w: fp32, finite."""
    w = np.asarray(w, dtype=F32)
    assert np.all(np.isfinite(w))
    p = w * F32(FIX_SCALE)  # fp32 x fp32 -> one fp32 rounding
    assert p.dtype == F32
    p = np.clip(p, F32(-FIX_SCALE), F32(FIX_SCALE))
    return np.rint(p).astype(np.int64)  # np.rint: round half to even


def digits(F):
    """Three signed digits d1, d2, d3 in [-128, 127] with d1 * 65536 + d2 * 256 + d3 == F (balanced base 256)."""
    F = np.asarray(F, dtype=np.int64)
    d3 = ((F + 128) & 255) - 128
    r = (F - d3) >> 8  # exact: F - d3 is a multiple of 256
    d2 = ((r + 128) & 255) - 128
    d1 = (r - d2) >> 8
    for d in (d1, d2, d3):
        assert np.all((d >= -128) & (d <= 127))
    assert np.all(d1 * 65536 + d2 * 256 + d3 == F)
    return d1, d2, d3


def digit_sums(coef, x):
    """The integer sums (s1, s2, s3), each int64 [C][nT16][B][16][2]: s_d = sum_a digit_d(fixed(coef[c][a][b][k])) *
    x[c][t][a][i][k]."""
    coef = np.asarray(coef)
    assert coef.dtype == F32 and coef.ndim == 4 and x.dtype == np.int8 and x.ndim == 5
    C, A, B, _ = coef.shape
    assert x.shape[0] == C and x.shape[2] == A and x.shape[3] == 16 and x.shape[4] == 2 and coef.shape[3] == 2
    # the contraction runs in float64 (BLAS): every product and partial sum is an integer below 2^53 there, hence exact
    # whatever the order; tests/test_beamformer_model.py checks the sums against Python integers
    xf = x.astype(np.float64)
    out = []
    for d in digits(fixed(coef)):  # [C][A][B][2]
        s = np.empty((C, x.shape[1], B, 16, 2), dtype=np.int64)
        for k in range(2):
            w = np.ascontiguousarray(d[:, :, :, k].transpose(0, 2, 1)).astype(np.float64)[:, None]  # [C][1][B][A]
            s[..., k] = np.matmul(w, np.ascontiguousarray(xf[..., k]))  # [C][nT16][A][16] -> [C][nT16][B][16]
        out.append(s)
    return out


def recombine(s1, s2, s3, scale=None):
    """The fp32 tail: low = RN32(s2 * 256 + s3) (integer sum, then one conversion), f = RN32(s1 * 65536 + low) (one fma),
    result RN32(f * inv), inv = RN32(1 / 8355711f) -- or RN32(f * RN32(s_b * inv)), scale = s_b per beam [B]."""
    low = s2 * 256 + s3
    assert np.all(np.abs(low) < 2 ** 31) and np.all(np.abs(s1) < 2 ** 24)  # int32 on the device; s1 converts exactly
    low32 = low.astype(F32)  # int64 -> fp32: round to nearest even
    # the fma in float64: s1 * 65536 (< 2^40) and low32 (< 2^31, an integer) add exactly there; one rounding to fp32
    f = (s1.astype(np.float64) * 65536.0 + low32.astype(np.float64)).astype(F32)
    if scale is None:
        return (f * INV).astype(F32)
    fac = (np.asarray(scale, dtype=F32) * INV).astype(F32)  # [B]
    return (f * fac[None, None, :, None, None]).astype(F32)


def acc_model(coef, x, scale=None):
    """dcs_bf_beamform_accumulated's int8 matrix-core form.  coef: the (weighted: w' = RN32(ghat * w)) coefficients."""
    return recombine(*digit_sums(coef, x), scale=scale)


def acc_model_nonfinite(coef, x, scale=None):
    """acc_model for a (weighted) coefficient tensor that may hold NaN / Inf (the slow class: an infinite or NaN delay
    value).  include/dcs_beamformer.h: "A coefficient that is not finite makes every sample of its beam NaN in the plane
    concerned, as in the verifier's sum (NaN * 0 = NaN)" -- so the non-finite coefficients are zeroed for the digit sums
    and every sample of a (channel, beam, plane) whose coefficient column (over the antennas) holds one is NaN."""
    coef = np.asarray(coef, dtype=F32)
    bad = ~np.isfinite(coef)  # [C][A][B][2]
    out = acc_model(np.where(bad, F32(0), coef), x, scale=scale)
    column = bad.any(axis=1)  # [C][B][2]
    out[np.broadcast_to(column[:, None, :, None, :], out.shape)] = F32(np.nan)
    return out


def zero_weight_coefficients(coef, weights):
    """include/dcs_beam_weights.h: "An antenna whose weight is 0 (either sign) contributes nothing, even where its delay
    values are not finite (its coefficient is made from zero terms)": (cos 0, sin 0) = (1, 0) wherever weights[b][a] == 0.
    coef [...][A][B][2], weights [B][A]; a copy."""
    out = np.array(coef, dtype=F32)
    out[..., np.asarray(weights, dtype=F32).T == 0, :] = (F32(1), F32(0))
    return out


def weighted_coefficients(coef, ghat):
    """w' = RN32(ghat[b][a] * w) for coef [...][A][B][2], ghat [B][A]."""
    g = np.asarray(ghat, dtype=F32).T[..., None]  # [A][B][1]
    return (g * np.asarray(coef, dtype=F32)).astype(F32)


def fused_model(coef_t, x, ghat=None, scale=None):
    """dcs_bf_generate_and_beamform: an fp32 running sum from +0.0f, acc = RN32(acc + RN32(w * x)) for a = 0 .. A-1, the
    coefficient of every sample's own time; weighted: w' = RN32(ghat * w) first and RN32(s_b * acc) last."""
    coef_t = np.asarray(coef_t)
    assert coef_t.dtype == F32 and coef_t.ndim == 5 and x.dtype == np.int8
    nt, C, A, B, _ = coef_t.shape
    assert x.shape == (C, nt // 16, A, 16, 2) and nt % 16 == 0
    xs = x.astype(F32).transpose(0, 1, 3, 2, 4).reshape(C, nt, A, 2)  # [c][t][a][2]
    acc = np.zeros((nt, C, B, 2), dtype=F32)
    for a in range(A):
        w = coef_t[:, :, a, :, :]  # [t][c][b][2]
        if ghat is not None:
            w = (np.asarray(ghat, dtype=F32)[:, a][None, None, :, None] * w).astype(F32)
        xa = xs[:, :, a, :].transpose(1, 0, 2)[:, :, None, :]  # [t][c][1][2]
        acc = (acc + (w * xa).astype(F32)).astype(F32)
    if scale is not None:
        acc = (np.asarray(scale, dtype=F32)[None, None, :, None] * acc).astype(F32)
    return np.ascontiguousarray(acc.reshape(nt // 16, 16, C, B, 2).transpose(2, 0, 3, 1, 4))


def normalise(weights):
    """s_b and ghat as include/dcs_beam_weights.h defines them (fp32, correctly rounded): s_b = max_a |g[b][a]| (NaN when
    a weight is not finite), ghat = RN32(g / s_b), 0 where s_b == 0."""
    w = np.asarray(weights, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs(w).max(axis=1)
        s = np.where(np.all(np.isfinite(w), axis=1), s, F32(np.nan)).astype(F32)
        gh = np.where(s[:, None] == 0, F32(0), w / s[:, None]).astype(F32)
    return s, gh


def pair_terms(table, dt, nr_channels, sampling_period):
    """(fRateTerm, fPhase0) of every pair of `table` at fDeltaTime dt: the verifier's lines (BCT.cu:320-325) in fp32 with
    its one fp64 chain, as oracle.bf_oracle.generate_numpy states them."""
    f, d = np.float32, np.float64
    dt = f(dt)
    denom = f(f(sampling_period) * f(nr_channels))
    rate = table["fDelayRate_sps"].astype(f)
    d_delay = (rate * dt).astype(f)
    k = (rate + d_delay).astype(f)
    n2 = ((table["fDelay_s"].astype(f) + d_delay).astype(f).astype(d) * d(nr_channels / 2.0) * d(f(np.pi)) / d(denom)).astype(f)
    d_phase = (table["fPhaseRate_radps"].astype(f) * dt).astype(f)
    phase0 = ((table["fPhase_rad"].astype(f) - n2).astype(f) + d_phase).astype(f)
    return k, phase0


def all_pairs_fast(table, dts, nr_channels, sampling_period):
    """True when every pair at every fDeltaTime of `dts` is in a fast class, with margin: a bound on |fRotation| over
    the channels (|fRateTerm| * pi * (C - 1) / D, 0.1 % on top, + |fPhase0|) below 32000 and the rate term zero or within
    2^-60 .. 2^60 (the constant divide's range).  Only then do the beamformers (which switch a whole table, resp.
    16-sample block, to the slow path) and the generator (which switches per wave) make coefficients the same way from the
    table as it is.  (Tables with a slow-class pair: pair_classes and interleave_with_filler, below, which
    tests/test_gpu_beamformer_exact_slow.py uses to get the slow path's bits from the same generator.)"""
    d = np.float64
    denom = d(np.float32(np.float32(sampling_period) * np.float32(nr_channels)))
    scale = np.pi * max(nr_channels - 1, 0) / denom * 1.001
    for dt in np.atleast_1d(np.asarray(dts, dtype=np.float32)):
        k, p0 = pair_terms(table, dt, nr_channels, sampling_period)
        ka = np.abs(k.astype(d))
        if not np.all(np.isfinite(ka)) or not np.all(np.isfinite(p0)):
            return False
        if not np.all((ka == 0) | ((ka >= 2.0 ** -60) & (ka < 2.0 ** 60))):
            return False
        if not np.all(ka * scale + np.abs(p0.astype(d)) < 32000.0):
            return False
    return True


FAST_LOW, FAST_HIGH, SLOW, UNCLEAR = 0, 1, 2, 3
FILLER_PHASE = 40000.0  # a filler pair: fPhase_rad = 40000, the other three values zero -- finite and plainly slow
FILLER_PHASE_HIGH = 20000.0  # ... and one that is plainly of the full-degree fast class


def pair_classes(table, dts, nr_channels, sampling_period):
    """int8 [len(dts)][len(table)]: the class of every pair at every fDeltaTime -- FAST_LOW, FAST_HIGH or SLOW, as
    dcs_pair_class (dc_sand_amd/csrc/bf_math.h) decides it from pair_terms in fp32 with the host's fRotBoundScale
    (pi_f32 * (C - 1) / D * 1.0001, rounded to fp32) -- or UNCLEAR where a restatement should not be trusted to the bit:
    the bound |fRateTerm| * scale + |fPhase0| within 0.5 % of 32000 or of 500, or a non-zero rate term whose exponent is
    one of the two on either side of an edge of dcs_rate_in_fast_range (2^-61, 2^-60, 2^60, 2^61).  A non-finite term is
    plainly SLOW.  A weighted call makes the coefficient of a pair of weight 0 from zero terms: pass flagged_table()."""
    f, d = np.float32, np.float64
    denom = f(f(sampling_period) * f(nr_channels))
    with np.errstate(all="ignore"):
        scale = f(d(nr_channels - 1) * d(f(np.pi)) / d(denom) * 1.0001)
        if not scale >= 0:
            scale = f(np.inf)
    dts = np.atleast_1d(np.asarray(dts, dtype=f))
    out = np.empty((dts.size, table.size), dtype=np.int8)
    for i, dt in enumerate(dts):
        with np.errstate(all="ignore"):
            k, p0 = pair_terms(table, dt, nr_channels, sampling_period)
            bound = ((np.abs(k) * scale).astype(f) + np.abs(p0)).astype(f)
        e = (np.ascontiguousarray(k).view(np.uint32) >> 23) & 0xFF
        in_range = (k == 0) | ((e >= 127 - 60) & (e <= 127 + 60))
        cls = np.where(~in_range | ~(bound < f(32000)), SLOW, np.where(bound < f(500), FAST_LOW, FAST_HIGH)).astype(np.int8)
        with np.errstate(invalid="ignore"):
            near = (np.abs(bound.astype(d) - 32000.0) <= 160.0) | (np.abs(bound.astype(d) - 500.0) <= 2.5)
        edge = (k != 0) & np.isin(e, (127 - 61, 127 - 60, 127 + 60, 127 + 61))
        cls[near | edge] = UNCLEAR
        out[i] = cls
    return out


def flagged_table(table, weights):
    """The table [b * A + a] as a weighted call sees it: the entries of the pairs of weight 0 zeroed (terms (0, 0))."""
    out = table.copy()
    out[np.asarray(weights, dtype=F32).ravel() == 0] = np.zeros((), dtype=table.dtype)
    return out


def interleave_with_filler(table_ab, A, B, phase=FILLER_PHASE):
    """The generator's table [a * B + b] of B beams as one of 2 B beams, [a * 2 B + b']: beam 2 b is beam b, beam 2 b + 1 a
    filler (fPhase_rad = ``phase``, the other three values zero).  Every second pair is then slow, so every run of two or
    more consecutive pairs holds one and every form of the generator (which decides per 64 / 128 / 256 consecutive pairs)
    makes all its pairs with coeff_slow.  With FILLER_PHASE_HIGH every second pair is of the full-degree fast class
    instead, and a table without a slow pair is made with the full-degree polynomials throughout -- as a beamformer makes
    it when ONE of its pairs is of that class."""
    assert table_ab.shape == (A * B,)
    out = np.zeros((A, 2 * B), dtype=table_ab.dtype)
    out[:, 0::2] = table_ab.reshape(A, B)
    out["fPhase_rad"][:, 1::2] = F32(phase)
    return out.ravel()


def real_beams(coef2):
    """[...][2 B][2] of an interleaved table -> [...][B][2] of the beams that are not fillers (a view)."""
    assert coef2.shape[-2] % 2 == 0 and coef2.shape[-1] == 2
    return coef2[..., 0::2, :]


def first_difference_or_nan(got, exp):
    """first_difference where ``exp`` may hold NaN: NaN (of any payload) in ``got`` exactly where ``exp`` has NaN, the
    uint32 views equal everywhere else.  None, or a message."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == F32 and exp.dtype == F32, (got.shape, exp.shape, got.dtype, exp.dtype)
    nan = np.isnan(exp)
    wrong = np.flatnonzero((np.isnan(got) != nan).ravel())
    if wrong.size:
        i = int(wrong[0])
        at = tuple(int(v) for v in np.unravel_index(i, got.shape))
        return (f"NaN in {int(np.isnan(got).sum())} places, expected in {int(nan.sum())}; first difference at {at} "
                f"(c, block, beam, sample, plane): got {got.ravel()[i]!r}, expected {exp.ravel()[i]!r}")
    return first_difference(np.where(nan, F32(0), got), np.where(nan, F32(0), exp))


def first_difference(got, exp):
    """None when the uint32 views agree; else a message naming the first differing flat index, both values and the
    (c, block, beam, sample, plane) it decodes to."""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == F32 and exp.dtype == F32, (got.shape, exp.shape, got.dtype, exp.dtype)
    g, e = got.view(np.uint32).ravel(), exp.view(np.uint32).ravel()
    bad = np.flatnonzero(g != e)
    if bad.size == 0:
        return None
    i = int(bad[0])
    c, blk, beam, sample, plane = (int(v) for v in np.unravel_index(i, got.shape))
    return (f"{bad.size} of {g.size} words differ; first at {i} = (c {c}, block {blk}, beam {beam}, sample {sample}, plane {plane}): "
            f"got {got.ravel()[i]!r} (0x{int(g[i]):08x}), expected {exp.ravel()[i]!r} (0x{int(e[i]):08x})")
