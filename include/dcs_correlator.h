/*
 * dcs_correlator.h -- the correlator: the visibilities V[a][b] = sum_t x_a[t] conj(x_b[t]) of every pair of antennas of
 * the sample tensor that the beamformer calls take, integrated in time.  It is the other half of an array back end: the
 * beam weights and delay tables that this library applies are solved from visibilities, on the samples that it beamforms.
 * Every term is an integer, so the stated arithmetic is exact: there is no rounding before the one conversion to float at
 * the end of an integration.
 *
 * Library: dc_sand_amd/csrc/libdcs_correlator.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns, and
 * nr_stations (A) and nr_channels (C) are the context's.  libdcs_beamformer.so itself keeps its ABI version 3 and its entry
 * points unchanged.  Status codes as dcs_beamformer.h.  No delay table is needed: there are no coefficients, hence no
 * coefficient time and no _dt entry points, and dcs_bf_tuning.math_mode plays no part.
 *
 * Tensors.
 * d_antenna: int8 [C][nt / 16][A][16][{re, im}] as dcs_bf_beamform_accumulated takes it, C * nt * A * 2 bytes, 16-byte
 *   aligned, nt % 16 == 0, A <= 256.  -128 IS A LEGAL SAMPLE and arithmetic like any other byte.  A dual-polarisation array
 *   passes its 2 A inputs as stations; the pairs of one antenna's polarisations are then among the baselines.
 * Baselines: NB = A (A + 1) / 2.  The pair (a, b) with b <= a has index a (a + 1) / 2 + b: row a of the lower triangle,
 *   the autocorrelation of a last in its row.  V[b][a] is the conjugate of V[a][b] and is not stored.
 * d_vis: int32_t [C][nr_vis][NB][{re, im}], nr_vis = (nt / 16) / blocks_per_vis, C * nr_vis * NB * 8 bytes, 8-byte aligned,
 *   caller-owned.  With n = blocks_per_vis, (re_a, im_a) and (re_b, im_b) the samples of a and b, and the sums over the
 *   16 n samples of blocks i n .. i n + n - 1 of the channel, visibility i is
 *     re = sum re_a re_b + im_a im_b        (= Re sum x_a conj(x_b))
 *     im = sum im_a re_b - re_a im_b        (= Im sum x_a conj(x_b))
 *   1 <= n <= 4095: under that bound no sum can leave int32 -- the largest magnitude is 4095 * 16 * 2 * 128^2 =
 *   2 146 959 360 < 2^31 -- so every word is the exact integer, any order of summation gives the same bits, the result cannot
 *   depend on the launch geometry, and im of an autocorrelation is exactly 0.  im is formed from the two sums
 *   sum im_a re_b and sum re_a im_b, subtracted as 32-bit integers: no byte is negated, so -128 needs no care.  Every word
 *   of d_vis is written exactly once, by a plain store; there are no atomics.  Longer integrations: the second call.
 * d_out: float [nr_vis / vis_per_integration][C][NB][{re, im}], time-major, 4-byte aligned, caller-owned: successive calls
 *   that write behind each other append to one time series.
 *
 * Integration (dcs_bf_integrate_visibilities), m = vis_per_integration.  For every output i, channel c, baseline and
 *   component, S = sum_j vis[c][i * m + j][..], j = 0 .. m - 1, exactly, in signed 64 bits; the output is RN((float)S): ONE
 *   rounding, to nearest, ties to even.  With accumulate non-zero it is RN(old + RN((float)S)), old being what d_out held.
 *   No float atomics.  nr_vis is the visibility count of d_vis.  The rule is dcs_bf_integrate_stokes' (dcs_stokes.h).
 * An output must not overlap an input: the result of a call whose output overlaps one of its inputs is undefined.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, a NULL output or a NULL
 * d_vis of the integration, d_vis not aligned to 8 bytes or d_out not to 4, nt % 16 != 0, blocks_per_vis == 0 or > 4095,
 * (nt / 16) % blocks_per_vis != 0, vis_per_integration == 0 or nr_vis % vis_per_integration != 0.  Then, with
 * DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so of another build.  Then a NULL
 * d_antenna with nt != 0 (invalid argument), A > 256 (DCS_ERR_UNSUPPORTED), a d_antenna that is not aligned to 16 bytes,
 * and buffers smaller than the tensors above: DCS_ERR_INVALID_ARGUMENT.  nt == 0 and nr_vis == 0 enqueue nothing and
 * succeed.  Capture: both calls only launch kernels and allocate nothing, not on a context's first call either, so both
 * can always be captured; a replay follows new sample bytes.
 */
#ifndef DCS_CORRELATOR_H
#define DCS_CORRELATOR_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* the sample tensor int8 [C][nt / 16][A][16][2] -> exact visibilities int32 [C][(nt / 16) / blocks_per_vis][NB][2] */
int dcs_bf_correlate_block(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                           uint32_t blocks_per_vis, int32_t *d_vis, size_t vis_bytes, void *stream);
/* visibilities [C][nr_vis][NB][2] summed vis_per_integration at a time -> float [nr_vis / m][C][NB][2] */
int dcs_bf_integrate_visibilities(dcs_bf_context *ctx, const int32_t *d_vis, size_t vis_bytes, uint32_t nr_vis,
                                  uint32_t vis_per_integration, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_CORRELATOR_H */
