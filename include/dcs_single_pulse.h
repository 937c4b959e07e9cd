/*
 * dcs_single_pulse.h -- the single-pulse search on the DM-time planes of dcs_dedisperse.h: the matched filter for a pulse of
 * unknown width is a bank of boxcars over each (beam, DM) series.  Three calls: the exact sums {sum x, sum x^2} of every
 * series, the decimated peak plane -- per beam, DM, boxcar width and block of block_len spectra the largest boxcar sum and
 * where it lies -- and the same as signal-to-noise, with the best width per block.  What leaves the GPU is a few hundred
 * times smaller than the planes.  Sums and peaks are exact integers and are stated, and tested, bit for bit; the
 * signal-to-noise is fp64 arithmetic rounded once per operation, and so is it.
 *
 * Library: dc_sand_amd/csrc/libdcs_single_pulse.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 * nr_beams (B) is an ARGUMENT, any value >= 1, as in dcs_dedisperse.h; of the context the calls use its device, nothing
 * else.  A series is one (beam, DM) pair.
 *
 * Tensors, all caller-owned device memory; every call reads them when the work runs, not when it is enqueued.
 * d_dm_time: const uint32_t [B][nr_dm][plane_spectra], time fastest, 4-byte aligned: exactly what dcs_bf_dedisperse_q8
 *   writes.
 * d_widths: const uint32_t [nr_widths], 4-byte aligned: boxcar widths in spectra, in any order; duplicates are allowed.
 * d_sums: uint64_t [B][nr_dm][2] = {s1, s2}, 8-byte aligned.
 * d_peaks: uint32_t [B][nr_dm][nr_widths][peak_blocks][2] = {value, time}, 8-byte aligned.
 * d_snr: float [B][nr_dm][nr_widths][peak_blocks], 4-byte aligned.
 * d_best: NULL, or uint32_t [B][nr_dm][peak_blocks], 4-byte aligned.
 *
 * dcs_bf_dm_time_sums writes per series {sum x, sum x^2 mod 2^64} over the words [first_spectrum, first_spectrum +
 *   nr_spectra) of the series, x widened to 64 bits before it is squared; with accumulate != 0 the two sums are added to
 *   what d_sums holds, mod 2^64.  The sums are exact integers: any order gives the same bits, no atomics are used and the
 *   result does not depend on the launch geometry.  nr_spectra == 0 with accumulate == 0 writes zeros; nr_dm == 0
 *   enqueues nothing and succeeds.
 *
 * dcs_bf_boxcar_peaks.  With t < nr_spectra relative to first_spectrum,
 *     S_w[t] = sum over k < w of d_dm_time[b][m][first_spectrum + t + k]                               (uint32, mod 2^32)
 *   block k covers t in [k * block_len, min((k + 1) * block_len, nr_spectra)), and nr_blocks = ceil(nr_spectra /
 *   block_len).  For the width index i with w = d_widths[i] and every block k < nr_blocks it writes
 *     d_peaks[b][m][i][first_block + k] = {max over the block's t of S_w[t], the smallest t that attains it}
 *                                                                                         if 1 <= w <= max_width,
 *                                         {0, 0xFFFFFFFF}                                 otherwise,
 *   and NO OTHER WORD of d_peaks.  Whatever the width list holds, it reads only the words [first_spectrum, first_spectrum +
 *   nr_spectra + max_width - 1) of a series, and that window is checked by value (as max_delay is in dcs_dedisperse.h).
 *   1 <= max_width <= 4096; block_len is a multiple of 64 in [64, 4096].  No atomics; the result does not depend on the
 *   launch geometry.  nr_spectra == 0, nr_widths == 0 or nr_dm == 0 enqueues nothing and succeeds.
 *
 * dcs_bf_peak_snr writes the entries first_block .. first_block + nr_blocks - 1 of d_snr and, where it is given, d_best,
 *   and no others.  In fp64, every operation rounded once, nothing fused, the divides and the square root the correctly
 *   rounded IEEE ones; {s1, s2} = d_sums[b][m], {value, time} = d_peaks[b][m][i][k], w = d_widths[i]:
 *     N   = (double)count;   mean = RN((double)s1 / N);   var = RN(RN((double)s2 / N) - RN(mean * mean))
 *     num = RN((double)value - RN((double)w * mean));   den = RN(sqrt(RN((double)w * var)))
 *     d_snr[b][m][i][k] = 1 <= w <= max_width ? (var > 0 ? (float) RN(num / den) : 0) : -infinity
 *   (a NaN var gives 0).  d_best[b][m][k] is the lowest width index i with the largest d_snr[b][m][i][k], or 0xFFFFFFFF
 *   where every width dropped or nr_widths == 0.  count is the number of words behind the sums.  nr_blocks == 0 or
 *   nr_dm == 0 enqueues nothing and succeeds.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, d_dm_time, d_widths,
 * d_sums, d_peaks or d_snr as they apply; pointers not aligned as stated above; nr_beams == 0; max_width outside
 * [1, 4096]; block_len no multiple of 64 in [64, 4096]; first_spectrum + nr_spectra > plane_spectra (the sums),
 * first_spectrum + nr_spectra + max_width - 1 > plane_spectra (the peaks); first_block + nr_blocks > peak_blocks;
 * count == 0.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so of another
 * build.  Then buffers smaller than the tensors above are DCS_ERR_INVALID_ARGUMENT.  Capture: all three calls only launch
 * kernels and allocate nothing, not on a context's first call either, so they can always be captured; a replay follows
 * new plane words, widths and sums.
 */
#ifndef DCS_SINGLE_PULSE_H
#define DCS_SINGLE_PULSE_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* planes uint32 [B][nr_dm][plane_spectra] -> {sum x, sum x^2} uint64 [B][nr_dm][2] over nr_spectra words from first_spectrum */
int dcs_bf_dm_time_sums(dcs_bf_context *ctx, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, uint32_t accumulate,
                        uint64_t *d_sums, size_t sums_bytes, void *stream);
/* planes and boxcar widths -> blocks first_block .. of the peak plane uint32 [B][nr_dm][nr_widths][peak_blocks][2] */
int dcs_bf_boxcar_peaks(dcs_bf_context *ctx, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths,
                        uint32_t nr_widths, uint32_t max_width, uint32_t block_len, uint32_t *d_peaks, size_t peaks_bytes,
                        uint64_t peak_blocks, uint64_t first_block, void *stream);
/* peaks, widths and the sums of count words -> signal-to-noise float [B][nr_dm][nr_widths][peak_blocks] and, unless NULL,
   the best width index uint32 [B][nr_dm][peak_blocks], blocks first_block .. first_block + nr_blocks - 1 */
int dcs_bf_peak_snr(dcs_bf_context *ctx, const uint32_t *d_peaks, size_t peaks_bytes, uint64_t peak_blocks, uint64_t first_block,
                    uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths, uint32_t nr_widths,
                    uint32_t max_width, const uint64_t *d_sums, size_t sums_bytes, uint64_t count, float *d_snr, size_t snr_bytes,
                    uint32_t *d_best, size_t best_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_SINGLE_PULSE_H */
