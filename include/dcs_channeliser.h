/*
 * dcs_channeliser.h -- the polyphase channeliser, the second half of an F-engine: the complex series of dcs_bf_ddc (dcs_ddc.h)
 * through a polyphase filterbank -- a FIR over P rows of N samples, then an N-point FFT -- per-channel gains, requantisation
 * to 8 bits and the corner turn into the sample tensor int8 [channel][nt / 16][station][16][{re, im}] that both beamformers,
 * the correlator and the incoherent beam take.  The reference has no counterpart (its feng/ holds the DDC only).
 *
 * Library: dc_sand_amd/csrc/libdcs_channeliser.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns, of which it uses
 * the device and nothing else: every size is an argument.  libdcs_beamformer.so itself keeps its ABI version 3 and its entry
 * points unchanged.  Status codes as dcs_beamformer.h.  dcs_bf_tuning.math_mode plays no part.
 *
 * Fixed: N = nr_channels is a power of two, 64 <= N <= 2048.  P = nr_taps, 1 <= P <= 16.  nr_spectra % 16 == 0.  order is
 * DCS_CHAN_ORDER_FFT (0) or DCS_CHAN_ORDER_ASCENDING (1).
 *
 * Tensors.
 * d_in: float [nr_inputs][in_stride][{re, im}], 8-byte aligned; in_stride in pairs.  One band of dcs_bf_ddc's output is this
 *   tensor as it stands.  Spectrum n of a row reads pairs n N .. n N + P N - 1; a row is read from pair 0 to
 *   (nr_spectra + P - 1) N - 1 and nowhere else: in_stride >= (nr_spectra + P - 1) N, and in_bytes >= ((nr_inputs - 1) in_stride
 *   + (nr_spectra + P - 1) N) * 8.  No state is kept between calls: a caller that continues a series presents the last
 *   (P - 1) N pairs again, as dcs_bf_dedisperse_q8 asks of a ring.
 * d_taps: float [P N], real, 4-byte aligned.  Tap p N + r multiplies pair (n + p) N + r.
 * d_twiddles: float [N / 2][{re, im}], 8-byte aligned.  Any table is served; the arithmetic is stated in its entries.
 *   dc_sand_amd/channeliser.py's twiddles(N) is RN32(cos, -sin of 2 pi j / N).
 * d_out: float [N][out_blocks][out_inputs][16][{re, im}], 16-byte aligned; d_out_q8 the same shape in int8, 16-byte aligned:
 *   the sample tensor's order, so with out_inputs = nr_stations and nt = 16 out_blocks it is the d_antenna of every call that
 *   takes one.  A call writes the runs of 16 pairs at [c][first_block + n / 16][first_input + i][n % 16] for all c, n <
 *   nr_spectra, i < nr_inputs, and no other byte; each word once, by a plain store.  Successive calls therefore fill a long
 *   tensor by blocks and by inputs.  out_bytes >= the whole tensor.  An output must not overlap an input.
 * d_gains: float [nr_inputs][N], 4-byte aligned, indexed by the call's input and the OUTPUT channel c.
 * d_clip_count: unsigned long long [nr_inputs], 8-byte aligned, or NULL.  The caller zeroes it.
 *
 * Arithmetic, per input and spectrum n; re and im each on their own; every RN is one fp32 operation, nothing contracted
 * (h = the taps, z = the row, W = the table):
 *   1. FIR.  For r = 0 .. N - 1: y[r] = RN(h[r] z[n N + r]); then for p = 1 .. P - 1 in order
 *      y[r] = RN(y[r] + RN(h[p N + r] z[(n + p) N + r])).
 *   2. Permutation.  v[i] = y[bitrev(i)], bit reversal over log2 N bits.
 *   3. Stages.  For s = 1 .. log2 N, m = 2^(s - 1), every group base g = 0, 2 m, 4 m, ... and j = 0 .. m - 1, with
 *      a = v[g + j], b = v[g + j + m], q = j N / (2 m):
 *        j == 0:      t = b, no arithmetic;
 *        q == N / 4:  t = (b.im, -b.re), no arithmetic;
 *        otherwise:   t.re = RN(RN(W[q].re b.re) - RN(W[q].im b.im)),  t.im = RN(RN(W[q].re b.im) + RN(W[q].im b.re));
 *      then v[g + j] = RN(a + t), v[g + j + m] = RN(a - t).  Entries 0 and N / 4 of the table are never read.
 *   4. Channel order.  X[k] = v[k]: with twiddles(N) this is sum_r y[r] e^(-2 pi i k r / N), and a tone e^(+2 pi i k0 t / N)
 *      lands in k0.  Output channel c = k for order 0; c = (k + N / 2) mod N for order 1, which ascends in frequency.
 *   5. dcs_bf_channelise writes X.
 *   6. dcs_bf_channelise_q8 writes exactly "quantise what the float call returns", by the quantiser of dcs_beam_quant.h:
 *      y = RN(X gain[i][c]); NaN -> -128, and nothing else gives -128; otherwise clamp(rint(y), -127, 127), ties to even;
 *      clipped: NaN or |rint(y)| > 127, re and im counted separately into d_clip_count[i] (integer atomic adds, exact in any
 *      order).  NULL counters give the same bytes.  Gains and counters are read and written when the work runs.
 * Consequences.  The result does not depend on the launch geometry, nor on how an implementation groups the butterflies:
 * radix 4, 8 or 16 in registers compose the same nodes.  A series cut at any multiple of 16 spectra gives the bits of one
 * call.  Denormals are kept.  NaN and +-Inf propagate as the network says; a NaN's payload is not part of the contract.
 * Error against the exact transform: |X - X_exact| <= (P + 5 log2 N) 2^-24 1.01 sum_{p,r} |h[p N + r]| |z[(n + p) N + r]|
 * for a table within 2^-24 of the roots of unity.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context; unless nr_spectra == 0 or
 * nr_inputs == 0, a NULL d_in, d_taps, d_twiddles, output or d_gains; d_in or d_twiddles not aligned to 8 bytes, d_taps or
 * d_gains not to 4, an output not to 16, counters not to 8; N no power of two in [64, 2048]; P outside [1, 16]; nr_spectra %
 * 16 != 0; order above 1; and, unless the call is empty, in_stride < (nr_spectra + P - 1) N, in_bytes smaller than stated,
 * first_block + nr_spectra / 16 > out_blocks (also where a 64-bit sum would wrap), first_input + nr_inputs > out_inputs, and
 * out_bytes smaller than the whole tensor; products are formed so that they cannot wrap.  Then, with DCS_ERR_UNSUPPORTED and
 * nothing enqueued: a context made by a libdcs_beamformer.so of another build.  nr_spectra == 0 and nr_inputs == 0 enqueue
 * nothing and succeed.  Capture: both calls only launch kernels (one each) and allocate nothing, not on a context's first call
 * either, so both can always be captured; a replay follows new input, taps, twiddles, gains and counters.
 */
#ifndef DCS_CHANNELISER_H
#define DCS_CHANNELISER_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define DCS_CHAN_ORDER_FFT 0u       /* channel c is bin c: 0, +1, ..., N / 2 - 1, -N / 2, ..., -1 */
#define DCS_CHAN_ORDER_ASCENDING 1u /* channel c is bin c - N / 2: ascending in frequency */
#define DCS_CHAN_IN_PAIRS(nr_channels, nr_taps, nr_spectra) \
    (((uint64_t)(nr_spectra) + (uint64_t)(nr_taps) - 1u) * (uint64_t)(nr_channels))

/* float [nr_inputs][in_stride][{re, im}] -> float [nr_channels][out_blocks][out_inputs][16][{re, im}] */
int dcs_bf_channelise(dcs_bf_context *ctx, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                      const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles,
                      uint32_t order, float *d_out, size_t out_bytes, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs,
                      uint32_t first_input, void *stream);
/* the same quantised: int8 [nr_channels][out_blocks][out_inputs][16][{re, im}] */
int dcs_bf_channelise_q8(dcs_bf_context *ctx, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                         const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles,
                         uint32_t order, const float *d_gains, int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks,
                         uint64_t first_block, uint32_t out_inputs, uint32_t first_input, unsigned long long *d_clip_count,
                         void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_CHANNELISER_H */
