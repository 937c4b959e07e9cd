/*
 * dcs_ddc.h -- the narrowband digital down-converter of an F-engine: the digitiser's real int8 stream mixed with an
 * oscillator, low-pass filtered by a FIR of up to 256 taps and decimated by 16, for one or two bands at once (the reference's
 * feng/ddc/: ddc.py, ddc_kernel.cu).  The mixer is folded into the filter,
 *     sum_j h[j] x[n + j] e^(-i w (n + j)) = e^(-i w n) sum_j (h[j] e^(-i w j)) x[n + j],
 * so the filter is a complex band-pass FIR with fixed INTEGER taps g[j] on the raw samples -- an exact integer contraction,
 * on v_mfma_i32_16x16x64_i8 -- followed by one rotation per output by a 32-bit phase accumulator, as an FPGA F-engine keeps
 * it: no drift, and successive calls continue one series.  dc_sand_amd/ddc.py makes g, the phase step and the gain of a real
 * low-pass h and a mixing frequency.
 *
 * Library: dc_sand_amd/csrc/libdcs_ddc.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns, of which it uses
 * the device and nothing else: every size is an argument.  libdcs_beamformer.so itself keeps its ABI version 3 and its entry
 * points unchanged.  Status codes as dcs_beamformer.h.  dcs_bf_tuning.math_mode plays no part.
 *
 * Fixed: the decimation is 16.  T = nr_taps, T % 64 == 0, 64 <= T <= 256.  nr_bands is 1 or 2.
 *
 * Tensors.
 * d_samples: real int8 [nr_inputs][in_stride], 16-byte aligned, in_stride % 16 == 0.  -128 IS A LEGAL SAMPLE.  Row i is read
 *   from sample 0 to sample 16 (nr_out - 1) + T - 1 and nowhere else: in_stride >= 16 (nr_out - 1) + T, and samples_bytes
 *   >= (nr_inputs - 1) in_stride + 16 (nr_out - 1) + T.  (The reference's 10-bit unpacking is `pass` and has no counterpart.)
 * d_taps: int32 [band][T][{re, im}] in CORRELATION order: tap j multiplies sample 16 m + j of output m.
 * d_digits: the taps as the kernel's operand, DCS_DDC_DIGITS_BYTES(T) = 16 T bytes, 16-byte aligned, opaque, only ever made by
 *   dcs_bf_ddc_tap_digits, for the (T, nr_bands) it is later used with.  Each tap component v is written as
 *   v = d0 + 256 d1 + 65536 d2 with balanced digits in [-128, 127] (d0 = the low byte of v as a signed byte, and so on): exact
 *   for |v| <= 8 355 711 = 127 * 65793.  Outside that range the top digit wraps modulo 256: the tap acts as
 *   g = ((v + 8 421 504) mod 2^24) - 8 421 504.
 * bands: HOST array of nr_bands dcs_ddc_band, read when the call is made.
 * d_out: float [band][input][out_stride][{re, im}], 8-byte aligned, out_stride >= nr_out, out_bytes >= ((nr_bands * nr_inputs
 *   - 1) out_stride + nr_out) * 8: the last row need not be a whole stride, so a call can write into the rows of a longer
 *   series.  Of a row the first nr_out pairs are written, each word exactly once, by a plain store; no atomics.
 *
 * Arithmetic per output m = 0 .. nr_out - 1, input and band (g = the taps as the digits hold them):
 *   1. S_re = sum_j g_re[j] x[16 m + j], S_im likewise, as integers modulo 2^32: the three digit sums, each an exact int32
 *      (|sum| <= 256 * 128 * 128), combined as s0 + (s1 << 8) + (s2 << 16) in wrapping 32-bit arithmetic.
 *   2. Under sum_j |g[j]| <= 2^24 - 1 per component no input can take the sum out of int32 (128 (2^24 - 1) < 2^31): the word
 *      is then the exact integer, independent of launch geometry and of the order of summation.
 *   3. F = RN((float)S), S taken as signed.
 *   4. u = phase0 + 16 (first_output + m) phase_step mod 2^32.
 *   5. (c, s) = dcs_sincos_turn32(u) of dc_sand_amd/csrc/bf_math.h: cos and sin of u / 2^32 turns, each within 2^-22: the
 *      quadrant n = (u + 2^29) >> 30, r = (int32)(u - (n << 30)), x = RN(RN((float)r) k), k = RN(pi/2 2^-30), the
 *      polynomials of the generator's sincos on [-pi/4, pi/4], the quadrant rotation.
 *   6. re = RN(RN(RN(F_re c) + RN(F_im s)) gain),  im = RN(RN(RN(F_im c) - RN(F_re s)) gain): F e^(-i 2 pi u / 2^32) gain, every
 *      operation a single fp32 operation, nothing contracted.
 *   7. With phase_step = 0 and phase0 = 0, c = 1 and s = 0 exactly and the output is gain (float)S.
 * first_output enters the phase only: a call that continues a series passes the count of outputs made so far and a sample
 *   pointer advanced by 16 per output, and gives the bits one call over the whole series gives.
 * An output must not overlap an input.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, d_taps, d_digits, bands or
 * d_out; d_taps not aligned to 4 bytes, d_digits or d_samples not to 16, d_out not to 8; nr_taps % 64 != 0 or outside
 * [64, 256]; nr_bands not 1 or 2; digits_bytes < 16 T; in_stride % 16 != 0; out_stride < nr_out; and, unless nr_out == 0 or
 * nr_inputs == 0, a NULL d_samples, in_stride < 16 (nr_out - 1) + T and buffers smaller than stated above.  Then, with
 * DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so of another build.  nr_out == 0 and
 * nr_inputs == 0 enqueue nothing and succeed.  Capture: both calls only launch kernels (one each) and allocate nothing, not
 * on a context's first call either, so both can always be captured; a replay follows new sample bytes, and keeps the bands
 * and first_output of the captured call.
 */
#ifndef DCS_DDC_H
#define DCS_DDC_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define DCS_DDC_DECIMATION 16u
#define DCS_DDC_DIGITS_BYTES(nr_taps) ((size_t)16u * (size_t)(nr_taps))

/* one band's oscillator and scale: u(m) = phase0 + 16 (first_output + m) phase_step mod 2^32, in units of 2^-32 turns */
typedef struct dcs_ddc_band {
    uint32_t phase_step; /* per INPUT sample */
    uint32_t phase0;
    float gain;
} dcs_ddc_band;

/* int32 [band][T][{re, im}] -> the operand table of 16 T bytes */
int dcs_bf_ddc_tap_digits(dcs_bf_context *ctx, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, void *d_digits,
                          size_t digits_bytes, void *stream);
/* int8 [nr_inputs][in_stride] -> float [band][input][out_stride][{re, im}], nr_out outputs per row */
int dcs_bf_ddc(dcs_bf_context *ctx, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes,
               uint64_t in_stride, const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands,
               const dcs_ddc_band *bands, uint64_t first_output, float *d_out, size_t out_bytes, uint64_t out_stride, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_DDC_H */
