/*
 * dcs_beam_complex.h -- the true complex product in the matrix-core beamformer of dcs_beamformer.h: tied-array beams.
 * dcs_bf_beamform_accumulated forms the reference's element-wise product, sum_a (cos * re_a, sin * im_a).  A beam that
 * points somewhere is the complex sum, sum_a w_a * x_a (or, with DCS_BF_COMPLEX_CONJ, sum_a conj(w_a) * x_a: the steering
 * convention most users need), and that is what the calls below form -- with the same samples in, the same tensors out,
 * the same coefficient making and twice the matrix instructions.  The detected form writes the block powers of
 * dcs_beam_power.h, so dcs_bf_integrate_block_power and the filterbank calls of dcs_filterbank.h consume it unchanged.
 *
 * Library: dc_sand_amd/csrc/libdcs_beam_complex.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 *
 * Tensors: d_antenna, d_weights (NULL: unweighted) and d_beams (float [C][nt / 16][B][16][{re, im}], 8-byte aligned) as
 * dcs_beam_weights.h describes them; d_block_power (float [C][nt / 16][B], 4-byte aligned) as dcs_beam_power.h does.
 *
 * The numerical contract.
 *
 * Definitions.  For one channel, beam b and sample t:
 *   w_a = (w_re, w_im) are the fp32 coefficients the float call would use.  With weights they are w' = RN(ghat * w) per
 *   component, and the result is scaled by RN(s_b * inv) instead of inv, exactly as dcs_beam_weights.h defines them.
 *   x_a = (x_re, x_im) are the int8 samples.
 *   sigma = +1, or sigma = -1 with flag DCS_BF_COMPLEX_CONJ.
 *
 *   F_re = fixed(w_re)        F_ip = fixed(sigma * w_im)        F_in = fixed(-sigma * w_im)
 *                                                (fixed() = the 24-bit fixed-point number of the float call: rint(w * 8355711))
 *   out_re:  S_d = sum_a digit_d(F_re) * x_re + digit_d(F_in) * x_im        d = 1, 2, 3
 *   out_im:  S_d = sum_a digit_d(F_re) * x_im + digit_d(F_ip) * x_re
 *   tail  :  low = RN32(S2 * 256 + S3);  f = RN32(S1 * 65536 + low);  v = RN32(f * inv)   (or * RN32(s_b * inv))
 *   (inv = RN32(1 / 8355711); digit_d: the balanced base-256 digits in [-128, 127], d1 the highest)
 *
 * Digits of the negated operand.  The digits of F_in are the balanced base-256 digits of the NUMBER -sigma * F(w_im) --
 * rint is odd, so fixed(-w) = -fixed(w) exactly.  They are not the negated digits of F_ip, because a digit can be -128.
 * The split between S1 and low decides a rounding, so the contract names the digits.  Samples are never negated:
 * -(-128) does not fit a byte.
 *
 * Int32 wrap-around.  The int32 sums are exact: |S_d| <= 2 * 256 * 128 * 128 = 2^23.  S2 * 256 + S3 is not safe in int32
 * here: its bound is 2^31 + 2^23 at 256 antennas.  The kernels evaluate low = fmaf((float)S2, 256.0f, (float)S3): both
 * conversions are exact because |S| <= 2^23, so it is the same single rounding of the same exact integer, bit-identical to
 * the integer form wherever the integer form does not wrap (tests/test_beam_complex_model.py proves both).
 *
 * Non-finite coefficients.  Both output planes of a row depend on both coefficient components: a row with a non-finite
 * coefficient in either component is NaN in BOTH planes (all four floats of a sample pair), whatever the samples are.
 *
 * Detected form.  p_t and the balanced pairwise block sum of dcs_beam_power.h are applied to exactly the floats the
 * complex float call returns.
 *
 * Accuracy: against the exact rational sum_a w_a * x_a of the fp32 coefficients,
 * |v - exact| <= 9e-8 * sum_a (|x_re| + |x_im|) + 1.8e-7 * |exact| per component.
 *
 * The int8-quantised output of this product -- 8-bit voltage beams -- is dcs_beam_complex_quant.h.  Out of scope: the fp32
 * fma-chain form (dcs_bf_tuning.math_mode bit 3: refused with DCS_ERR_UNSUPPORTED, nothing enqueued, like the other
 * companions' calls), and the per-sample fused beamformer (dcs_bf_generate_and_beamform).
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, a NULL output, d_beams not
 * 8-byte aligned, d_block_power or non-NULL weights not 4-byte aligned, nt % 16 != 0, a bit of flags other than
 * DCS_BF_COMPLEX_CONJ.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so of
 * another build, and the fp32 fma-chain form.  Everything else as the float call (sizes, the antenna tensor's alignment,
 * more than 256 antennas); buffers smaller than the tensors above are DCS_ERR_INVALID_ARGUMENT.  Capture: under the rule
 * of the float call, as dcs_beam_weights.h states it (a first call on a context allocates, and so does a first weighted
 * one: make one outside the capture).
 */
#ifndef DCS_BEAM_COMPLEX_H
#define DCS_BEAM_COMPLEX_H

#include "dcs_beamformer.h"

#define DCS_BF_COMPLEX_CONJ 1u /* flags bit 0: sum_a conj(w_a) * x_a */

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* the complex product sum_a w_a x_a, float beams out: coefficients of time index t_coeff */
int dcs_bf_beamform_accumulated_complex(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                        size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams,
                                        size_t beams_bytes, void *stream);
/* the same with the coefficients' fDeltaTime given */
int dcs_bf_beamform_accumulated_complex_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                           size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams,
                                           size_t beams_bytes, void *stream);
/* the same two with detected block power out */
int dcs_bf_beamform_accumulated_complex_power(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                              size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_block_power,
                                              size_t power_bytes, void *stream);
int dcs_bf_beamform_accumulated_complex_power_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                                 size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                                 float *d_block_power, size_t power_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_BEAM_COMPLEX_H */
