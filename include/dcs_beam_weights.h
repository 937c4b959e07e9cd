/*
 * dcs_beam_weights.h -- per-input beam weights for the two beamformers of dcs_beamformer.h: one real weight per
 * antenna and beam, applied where the coefficients are made (no extra pass over the samples).  What a deployed
 * tied-array beamformer sets with `?beam-weights <beam-stream> w_1 ... w_A`: weight 0 flags a dead antenna, other
 * values taper the array.
 *
 * Library: dc_sand_amd/csrc/libdcs_beam_weights.so, a companion of libdcs_beamformer.so built with it from the same
 * tree (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 *
 * The weights: d_weights is device memory, [nr_beams][nr_stations] fp32 (the beamformers' table order, b * A + a; one
 * row = one ?beam-weights request), 4-byte aligned.  It is read when the work runs on the stream, not when the call is
 * made: new weights copied into the same buffer on the same stream apply from the next call on, and a captured graph
 * picks them up on replay.  A context that holds a slice of the beams (beam_offset .. beam_offset + nr_beams - 1 of a
 * global table) passes d_global_weights + beam_offset * nr_stations.
 *
 * The numerical contract, per beam b:
 *   s_b = max_a |g[b][a]|, ghat[b][a] = RN(g[b][a] / s_b) (0 where s_b == 0); a weight that is not finite makes s_b NaN.
 *   Each coefficient w becomes w' = RN(ghat * w), and the beam's result is multiplied by s_b once, at the end:
 *   - dcs_bf_generate_and_beamform_weighted[_dt]: sum += RN(w' * x) in antenna order (separate multiply and add), then
 *     RN(s_b * sum);
 *   - dcs_bf_beamform_accumulated_weighted[_dt]: the fixed-point digits are those of rint(w' * 8355711), and the exact
 *     integer sums are scaled by RN(s_b * RN(1 / 8355711)) instead of RN(1 / 8355711).
 *   An antenna whose weight is 0 (either sign) contributes nothing, even where its delay values are not finite (its
 *   coefficient is made from zero terms); a beam whose weights are all 0 is 0; a beam with a weight that is not finite is
 *   NaN in both planes, the other beams are unaffected.  All weights 1: bit-identical to the unweighted call; every
 *   weight of a beam 2^k: exactly 2^k times the unweighted result.
 *
 * Arguments and tensors as the unweighted calls (nt % 16 == 0, t0 % 16 == 0, sizes and alignments), plus d_weights:
 * NULL or misaligned is DCS_ERR_INVALID_ARGUMENT.  Capture: under the rule of the unweighted calls (a first call on a
 * context allocates, so make one outside the capture); a call is two launches (pre-pass, beamformer) per launch of the
 * unweighted call.  dcs_bf_beamform_accumulated_weighted* with the fp32 fma-chain form (dcs_bf_tuning.math_mode bit 3)
 * returns DCS_ERR_UNSUPPORTED and enqueues nothing.  A context made by a libdcs_beamformer.so of another build returns
 * DCS_ERR_UNSUPPORTED.
 */
#ifndef DCS_BEAM_WEIGHTS_H
#define DCS_BEAM_WEIGHTS_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* dcs_bf_generate_and_beamform[_dt] with weights */
int dcs_bf_generate_and_beamform_weighted(dcs_bf_context *ctx, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                          size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                          void *stream);
int dcs_bf_generate_and_beamform_weighted_dt(dcs_bf_context *ctx, const float *dt, uint32_t nt, const int8_t *d_antenna,
                                             size_t antenna_bytes, const float *d_weights, float *d_beams,
                                             size_t beams_bytes, void *stream);

/* dcs_bf_beamform_accumulated[_dt] with weights (the int8 matrix-core form) */
int dcs_bf_beamform_accumulated_weighted(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                         size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                         void *stream);
int dcs_bf_beamform_accumulated_weighted_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                            size_t antenna_bytes, const float *d_weights, float *d_beams,
                                            size_t beams_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_BEAM_WEIGHTS_H */
