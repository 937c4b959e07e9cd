/*
 * dcs_beam_power.h -- detected beam power, integrated in time, from the matrix-core beamformer of dcs_beamformer.h
 * (dcs_bf_beamform_accumulated*): what a pulsar or transient search consumes is not voltages but |beam|^2 summed over a
 * run of samples, as a filterbank [time][channel][beam].  The detection happens in the beamformer kernel's epilogue, so
 * the call writes 4 bytes per (beam, 16-sample block) -- 0.25 bytes per (beam, sample) instead of 8 -- and the fp32
 * beams never reach memory.  A second, small kernel sums runs of blocks into spectra.
 *
 * Library: dc_sand_amd/csrc/libdcs_beam_power.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 *
 * Tensors: d_antenna and d_weights (NULL: unweighted) as dcs_beam_quant.h describes them.
 * d_block_power: float [nr_channels][nt / 16][nr_beams], C * (nt / 16) * B * 4 bytes, 4-byte aligned, caller-owned.
 * d_spectra: float [nr_blocks / blocks_per_spectrum][nr_channels][nr_beams], 4-byte aligned, caller-owned: time-major, so
 * successive calls that write behind each other append to one time series.  d_block_power and d_spectra must not
 * overlap: the result of an integration whose output overlaps its input is undefined.
 *
 * The numerical contract.  Let v_re(t), v_im(t) be the fp32 values that
 * dcs_bf_beamform_accumulated[_dt] (or, with weights, dcs_bf_beamform_accumulated_weighted[_dt]) writes for a channel,
 * beam and sample, bit for bit -- NaN rows included.  Then
 *   per sample:           p_t = RN(RN(v_re * v_re) + RN(v_im * v_im))     two multiplies and one add, no fma;
 *   per 16-sample block:  P = the balanced pairwise sum of p_0 .. p_15 in sample order: level 1 is p_2m + p_2m+1, level 2
 *                         adds neighbours (0,1) (2,3) ... of level 1, and so on; four levels, every add rounded once.
 * Gradual underflow is kept and nothing is special-cased: a NaN or Inf in v gives what this arithmetic gives.
 * d_weights == NULL and all-ones weights give the same bits.
 *
 * Integration (dcs_bf_integrate_block_power), n = blocks_per_spectrum.  For every spectrum i, channel c and beam b the
 * accumulator starts at d_spectra[i][c][b] if accumulate is non-zero, else at the first block's P; the remaining blocks
 * P[c][i * n + j][b] are added in order of j, one rounded add each.  No float atomics: the result is deterministic and
 * independent of launch geometry.  accumulate lets an integration span calls, so the coefficients can be renewed inside
 * one integration.  nr_channels and nr_beams are the context's; nr_blocks is the block count of d_block_power (nt / 16 of
 * the call that wrote it).
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, a NULL output (and, for
 * the integration, a NULL input), d_block_power, d_spectra or non-NULL weights not 4-byte aligned, nt % 16 != 0,
 * blocks_per_spectrum == 0 or nr_blocks % blocks_per_spectrum != 0.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued:
 * a context made by a libdcs_beamformer.so of another build, and (the beamformer calls) the fp32 fma-chain form
 * (dcs_bf_tuning.math_mode bit 3).  Everything else as the float call (sizes, the antenna tensor's alignment, more than
 * 256 antennas); buffers smaller than the tensors above are DCS_ERR_INVALID_ARGUMENT.  Capture: the beamformer calls
 * under the rule of the float call, as dcs_beam_weights.h states it (a first call on a context allocates, and so does a
 * first weighted one: make one outside the capture); the integration only launches a kernel and can always be captured.
 */
#ifndef DCS_BEAM_POWER_H
#define DCS_BEAM_POWER_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* dcs_bf_beamform_accumulated[_weighted] with detected block power out: coefficients of time index t_coeff */
int dcs_bf_beamform_accumulated_power(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                      size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                      void *stream);
/* the same with the coefficients' fDeltaTime given */
int dcs_bf_beamform_accumulated_power_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                         size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                         void *stream);
/* block powers [C][nr_blocks][B] summed blocks_per_spectrum at a time into spectra [nr_blocks / blocks_per_spectrum][C][B] */
int dcs_bf_integrate_block_power(dcs_bf_context *ctx, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                 uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                 void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_BEAM_POWER_H */
