/*
 * dcs_filterbank.h -- 8-bit search filterbanks from the float spectra of dcs_beam_power.h and dcs_incoherent_beam.h: what
 * a pulsar or transient search reads.  Three calls: running sums per channel and beam over time, the scales {mean, gain}
 * from those sums, and the quantiser, which takes each channel's bandpass out, scales it to a fixed mean and standard
 * deviation, rounds to a byte and transposes from beam-fastest floats to one [time][channel] byte series per beam.
 *
 * Library: dc_sand_amd/csrc/libdcs_filterbank.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 * nr_channels (C) is the context's.  nr_beams (B) is an ARGUMENT of every call, any value >= 1: pass the context's beams
 * for the detected spectra of dcs_bf_integrate_block_power and 1 for the spectra of dcs_bf_integrate_incoherent_power.  No
 * delay table is needed and dcs_bf_tuning.math_mode plays no part.
 *
 * Tensors, all caller-owned device memory.
 * d_spectra: const float [nr_spectra][C][B], beam fastest, 4-byte aligned.
 * d_sums: double [C][B][2] = {s1, s2}, 8-byte aligned.
 * d_scales: float [C][B][2] = {mu, k}, 8-byte aligned.  A caller may fill it itself; the quantiser reads it from device
 *   memory when the work runs, not when it is enqueued.
 * d_filterbank: uint8_t [B][out_spectra][C], channel fastest, 16-byte aligned: per beam a time series, or a ring, that
 *   successive calls fill.
 * d_clip_count: NULL, or unsigned long long [B], 8-byte aligned, zeroed by the caller.
 *
 * dcs_bf_spectra_sums.  Per (c, b) the accumulators start at {0, 0}, with accumulate non-zero at what d_sums holds; then,
 *   for t = 0 .. nr_spectra - 1 in order, with x = d_spectra[t][c][b]:
 *     s1 = RN64(s1 + (double)x),  s2 = RN64(s2 + (double)x * (double)x)
 *   (the product of two floats is exact in a double, so fused and unfused forms give the same bits).  NaN and Inf go
 *   through as this arithmetic takes them.  No atomics; the result does not depend on the launch geometry.  nr_spectra == 0
 *   enqueues nothing and succeeds (d_sums is left as it is).
 *
 * dcs_bf_filterbank_scales.  count is the number of spectra behind the sums, by value, 1 <= count < 2^53.  In fp64, every
 *   operation rounded once, nothing fused, divide and square root the correctly rounded IEEE ones:
 *     N = (double)count;  m = s1 / N;  var = s2 / N - m * m;  sd = var > 0 ? sqrt(var) : 0   (a NaN var gives 0)
 *     mu = RN32(m);  k = sd > 0 ? RN32((double)target_std / sd) : 0
 *   A constant channel has var <= 0 up to rounding and gets k = 0: every one of its bytes is then rint(level).
 *
 * dcs_bf_filterbank_q8 writes rows first_spectrum .. first_spectrum + nr_spectra - 1 of every beam and NO OTHER BYTE of
 *   d_filterbank.  Per element, in fp32 with no fma, x = d_spectra[t][c][b], {mu, k} = d_scales[c][b]:
 *     d = RN(x - mu);  y = RN(RN(d * k) + level);  q = clamp(rint(y), 0, 255), ties to even
 *   A NaN y gives q = 0; +Inf gives 255 and -Inf 0.  d_filterbank[b][first_spectrum + t][c] = q, or, with
 *   DCS_FB_DESCENDING in flags, d_filterbank[b][first_spectrum + t][C - 1 - c] = q (the search formats' frequency order).
 *   An element is clipped where y is NaN, rint(y) < 0 or rint(y) > 255; d_clip_count[b] grows by the clipped elements of
 *   beam b in the call (integer atomics: exact).  NULL gives the same bytes.  nr_spectra == 0 enqueues nothing and succeeds.
 *   d_spectra 16-byte aligned with B % 4 == 0 and C % 16 == 0 takes a form with 16-byte loads and stores; every other case
 *   is served too and gives the same bytes.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, input or output
 * (d_spectra, d_sums, d_scales, d_filterbank as they apply), pointers not aligned as stated above (a non-NULL d_clip_count
 * included), nr_beams == 0, count == 0 or count >= 2^53, flag bits other than DCS_FB_DESCENDING, first_spectrum +
 * nr_spectra > out_spectra.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so
 * of another build.  Then buffers smaller than the tensors above are DCS_ERR_INVALID_ARGUMENT.  Capture: all three calls
 * only launch kernels and allocate nothing, not on a context's first call either, so they can always be captured.
 */
#ifndef DCS_FILTERBANK_H
#define DCS_FILTERBANK_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define DCS_FB_DESCENDING 1u /* flags bit 0: channel c lands in column C - 1 - c */

/* spectra float [nr_spectra][C][B] -> running sums double [C][B][2] = {sum x, sum x^2} over time, in order */
int dcs_bf_spectra_sums(dcs_bf_context *ctx, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                        uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream);
/* sums of count spectra -> scales float [C][B][2] = {mean, target_std / standard deviation} */
int dcs_bf_filterbank_scales(dcs_bf_context *ctx, const double *d_sums, size_t sums_bytes, uint64_t count, uint32_t nr_beams,
                             float target_std, float *d_scales, size_t scales_bytes, void *stream);
/* spectra -> rows first_spectrum .. first_spectrum + nr_spectra - 1 of the filterbanks uint8 [B][out_spectra][C] */
int dcs_bf_filterbank_q8(dcs_bf_context *ctx, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                         const float *d_scales, float level, uint32_t flags, uint8_t *d_filterbank, size_t filterbank_bytes,
                         uint64_t out_spectra, uint64_t first_spectrum, unsigned long long *d_clip_count, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_FILTERBANK_H */
