/*
 * dcs_beam_complex_quant.h -- 8-bit complex voltage beams of the true complex product: the tied-array beams of
 * dcs_beam_complex.h, requantised per beam in the beamformer kernel's epilogue exactly as dcs_beam_quant.h requantises the
 * element-wise ones.  This is what a deployed tied-array beamformer ships, and the one quantised tensor that is meaningful
 * as the d_antenna of a second beamformer: sub-array beams that point somewhere, then beams of those beams
 * (examples/hierarchical_beams.py).  The call writes 2 bytes per (beam, sample) instead of the float call's 8, and the fp32
 * beams never reach memory.
 *
 * Library: dc_sand_amd/csrc/libdcs_beam_complex_quant.so, a companion of libdcs_beamformer.so built with it from the same
 * tree (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 *
 * Tensors: d_antenna and d_weights (NULL: unweighted) as dcs_beam_complex.h; flags: bit 0 is DCS_BF_COMPLEX_CONJ
 * (sum_a conj(w_a) x_a), no other bit is defined.  d_beams_q8 (int8 [nr_channels][nt / 16][nr_beams][16][{re, im}],
 * C * nt * B * 2 bytes, 8-byte aligned: the antenna tensor's order), d_quant_gains ([nr_beams] fp32, 4-byte aligned) and
 * d_clip_count ([nr_beams] unsigned long long, 8-byte aligned, or NULL) as dcs_beam_quant.h.  Gains and counters are read
 * and written when the work runs on the stream, not when the call is made: a captured graph picks up new gains on replay.
 * A context that holds a slice of the beams passes d_global_gains + beam_offset and d_global_counts + beam_offset.
 *
 * The numerical contract is that of dcs_beam_quant.h with another v.  Let v be the fp32 value
 * that dcs_bf_beamform_accumulated_complex[_dt] writes for that plane, beam and sample with the same d_weights and flags,
 * bit for bit (dcs_beam_complex.h defines it), and k_b the beam's gain.  Then
 *   y = RN(v * k_b)      one fp32 multiply of its own: the bytes are exactly "quantise what the complex float call returns";
 *   y is NaN:            q = -128, and nothing else produces -128;
 *   otherwise:           q = clamp(rint(y), -127, 127), ties to even, so +-Inf gives +-127;
 *   clipped:             y is NaN, or |rint(y)| > 127.
 * d_clip_count[b] grows by the number of clipped components of beam b in the call, re and im counted separately; the
 * caller zeroes it.  NULL: no counting, the same output bytes.  Gains have no special cases -- the multiply decides.  A row
 * with a non-finite coefficient in either component is NaN in both planes of the float call, so it is -128 in both planes
 * here and counts as clipped in both.  d_weights == NULL and all-ones weights give the same bytes.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, NULL gains, a NULL output,
 * gains or non-NULL weights not 4-byte aligned, a non-NULL counter array not 8-byte aligned, d_beams_q8 not 8-byte aligned,
 * nt % 16 != 0, a bit of flags other than DCS_BF_COMPLEX_CONJ.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued: a
 * context made by a libdcs_beamformer.so of another build, and the fp32 fma-chain form (dcs_bf_tuning.math_mode bit 3).
 * Everything else as the float call (sizes, the antenna tensor's alignment, more than 256 antennas); buffers smaller than
 * the tensors above are DCS_ERR_INVALID_ARGUMENT.  Capture: under the rule of the float call, as dcs_beam_weights.h states
 * it (a first call on a context allocates, and so does a first weighted one: make one outside the capture).
 */
#ifndef DCS_BEAM_COMPLEX_QUANT_H
#define DCS_BEAM_COMPLEX_QUANT_H

#include "dcs_beam_complex.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* dcs_bf_beamform_accumulated_complex with int8 output: coefficients of time index t_coeff */
int dcs_bf_beamform_accumulated_complex_q8(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                           size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                           const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                           unsigned long long *d_clip_count, void *stream);
/* the same with the coefficients' fDeltaTime given */
int dcs_bf_beamform_accumulated_complex_q8_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                              size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                              const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                              unsigned long long *d_clip_count, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_BEAM_COMPLEX_QUANT_H */
