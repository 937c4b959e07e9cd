/*
 * dcs_beam_quant.h -- quantised int8 beam output, with per-beam gains and clip counters, for the matrix-core beamformer
 * of dcs_beamformer.h (dcs_bf_beamform_accumulated*): what a deployed tied-array beamformer ships is 8-bit complex,
 * requantised per beam with a quantisation gain, and the count of clipped values is what an operator sets that gain by.
 * The requantisation happens in the beamformer kernel's epilogue, so the call writes 2 bytes per (beam, sample) instead
 * of 8 and the fp32 beams never reach memory.
 *
 * Library: dc_sand_amd/csrc/libdcs_beam_quant.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 *
 * Tensors: d_antenna as dcs_bf_beamform_accumulated.  d_beams_q8 is int8 [nr_channels][nt / 16][nr_beams][16][{re, im}],
 * C * nt * B * 2 bytes: the antenna tensor's order with beams in place of antennas, so a quantised beam tensor can be the
 * d_antenna of a second beamformer.  It has the alignment rule of the float call's d_beams (8 bytes).
 * d_weights: NULL (unweighted) or per-input beam weights exactly as dcs_beam_weights.h describes them.
 * d_quant_gains: device memory, [nr_beams] fp32, 4-byte aligned.  d_clip_count: device memory, [nr_beams] unsigned long
 * long, 8-byte aligned, or NULL.  Gains and counters are read and written when the work runs on the stream, not when
 * the call is made: new gains copied into the same buffer on the same stream apply from the next call on, and a captured
 * graph picks them up on replay.  A context that holds a slice of the beams (beam_offset .. beam_offset + nr_beams - 1
 * of a global table) passes d_global_gains + beam_offset and d_global_counts + beam_offset.
 *
 * The numerical contract.  Let v be the fp32 value that dcs_bf_beamform_accumulated[_dt] (or,
 * with weights, dcs_bf_beamform_accumulated_weighted[_dt]) writes for that plane, beam and sample, bit for bit, and k_b
 * the beam's gain.  Then
 *   y = RN(v * k_b)      one fp32 multiply of its own, not folded into any other factor: the bytes are exactly
 *                        "quantise what the float call returns";
 *   y is NaN:            q = -128, and nothing else produces -128;
 *   otherwise:           q = clamp(rint(y), -127, 127), ties to even, so +-Inf gives +-127;
 *   clipped:             y is NaN, or |rint(y)| > 127.
 * d_clip_count[b] grows by the number of clipped components of beam b in the call, re and im counted separately; the
 * caller zeroes it.  NULL: no counting, the same output bytes.  Gains have no special cases -- the multiply decides: a
 * gain of 0 gives zeros, a gain of Inf gives +-127 (and -128 where v is 0), a NaN gain gives -128.  Beams whose float
 * result is NaN (a non-finite delay value or weight) come out as -128 and count as clipped.  d_weights == NULL and
 * all-ones weights give the same bytes.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, NULL gains, gains or
 * non-NULL weights not 4-byte aligned, a non-NULL counter array not 8-byte aligned, nt % 16 != 0.  Then, with
 * DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so of another build, and the fp32
 * fma-chain form (dcs_bf_tuning.math_mode bit 3).  Everything else as the float call (sizes, alignments, more than 256
 * antennas).  Capture: under the rule of the unweighted call, as dcs_beam_weights.h states it (a first call on a context
 * allocates, and so does a first weighted one: make one outside the capture).
 */
#ifndef DCS_BEAM_QUANT_H
#define DCS_BEAM_QUANT_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* dcs_bf_beamform_accumulated[_weighted] with int8 output: coefficients of time index t_coeff */
int dcs_bf_beamform_accumulated_q8(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                   size_t antenna_bytes, const float *d_weights, const float *d_quant_gains,
                                   int8_t *d_beams_q8, size_t beams_bytes, unsigned long long *d_clip_count, void *stream);
/* the same with the coefficients' fDeltaTime given */
int dcs_bf_beamform_accumulated_q8_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                      size_t antenna_bytes, const float *d_weights, const float *d_quant_gains,
                                      int8_t *d_beams_q8, size_t beams_bytes, unsigned long long *d_clip_count, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_BEAM_QUANT_H */
