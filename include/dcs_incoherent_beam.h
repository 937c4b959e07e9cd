/*
 * dcs_incoherent_beam.h -- the incoherent beam beside the tied-array outputs of dcs_beamformer.h: the antennas' own power
 * summed, sum_a |x_a|^2 per channel and time, integrated like the detected beams of dcs_beam_power.h.  A search pipeline
 * runs it next to the coherent beams: it covers the whole primary beam, it normalises the detected beams and it vetoes
 * interference.  Every term is an integer, so the stated arithmetic is exact: there is no rounding before the one
 * conversion to float at the end of an integration.
 *
 * Library: dc_sand_amd/csrc/libdcs_incoherent_beam.so, a companion of libdcs_beamformer.so built with it from the same
 * tree (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns, and
 * nr_stations (A) and nr_channels (C) are the context's.  libdcs_beamformer.so itself keeps its ABI version 3 and its
 * entry points unchanged.  Status codes as dcs_beamformer.h.  No delay table is needed: there are no coefficients, hence
 * no coefficient time and no _dt entry points, and dcs_bf_tuning.math_mode plays no part (bit 3 is not refused).
 *
 * Tensors.
 * d_antenna: as the float call takes it, int8 [C][nt / 16][A][16][{re, im}], C * nt * A * 2 bytes, 16-byte aligned,
 *   nt % 16 == 0, A <= 256.  -128 is a legal sample.
 * d_weights: NULL, or const float [A], 4-byte aligned: ONE row in the sense of dcs_beam_weights.h, so a pointer to row b
 *   of a [B][A] weight table works.  The weights are FLAGS ONLY: antenna a takes part iff d_weights == NULL or
 *   d_weights[a] != 0.  +0 and -0 exclude the antenna; every other value -- 0.5, -3, NaN and the infinities included --
 *   includes it at weight 1.  VALUES OTHER THAN 0 DO NOT SCALE: an antenna is in the sum whole, or it is not in it.  (A
 *   real taper would give up the exact integer contract.)  The weights are read when the work runs, not when it is enqueued.
 * d_block_power: uint32_t [C][nt / 16], C * (nt / 16) * 4 bytes, 4-byte aligned, caller-owned:
 *   P[c][k] = sum over the antennas taking part, over the 16 samples t of block k, of re^2 + im^2, as an exact integer.
 *   Its maximum is 256 * 16 * 2 * 128^2 = 2^27, so it fits 32 bits; any order of summation gives the same bits, so the
 *   result cannot depend on the launch geometry.
 * d_spectra: float [nr_blocks / blocks_per_spectrum][C], time-major, 4-byte aligned, caller-owned: successive calls that
 *   write behind each other append to one time series.
 *
 * Integration (dcs_bf_integrate_incoherent_power), n = blocks_per_spectrum.  For every spectrum i and channel c,
 *   S = sum_j P[c][i * n + j], j = 0 .. n - 1, exactly, in 64 bits; the output is RN((float)S): ONE rounding, to nearest,
 *   ties to even.  With accumulate non-zero it is RN(old + RN((float)S)), old being what d_spectra[i][c] held.  No float
 *   atomics.  nr_blocks is the block count of d_block_power (nt / 16 of the call that wrote it).  d_block_power and
 *   d_spectra must not overlap: the result of an integration whose output overlaps its input is undefined.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, a NULL output (and, for
 * the integration, a NULL input), d_block_power, d_spectra or non-NULL weights not 4-byte aligned, nt % 16 != 0,
 * blocks_per_spectrum == 0 or nr_blocks % blocks_per_spectrum != 0.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued:
 * a context made by a libdcs_beamformer.so of another build.  Everything else as the float call (the antenna tensor's
 * alignment, more than 256 antennas; nt == 0 and nr_blocks == 0 enqueue nothing and succeed); buffers smaller than the
 * tensors above are DCS_ERR_INVALID_ARGUMENT.  Capture: both calls only launch kernels and allocate nothing, not on
 * a context's first call either, so both can always be captured.
 */
#ifndef DCS_INCOHERENT_BEAM_H
#define DCS_INCOHERENT_BEAM_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* int8 samples [C][nt / 16][A][16][2] -> exact block powers uint32 [C][nt / 16] of the antennas that d_weights flags */
int dcs_bf_incoherent_block_power(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                  const float *d_weights, uint32_t *d_block_power, size_t power_bytes, void *stream);
/* block powers [C][nr_blocks] summed blocks_per_spectrum at a time into spectra float [nr_blocks / blocks_per_spectrum][C] */
int dcs_bf_integrate_incoherent_power(dcs_bf_context *ctx, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                      uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                      void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_INCOHERENT_BEAM_H */
