/*
 * dcs_fold.h -- the pulsar folder: the 8-bit filterbanks of dcs_filterbank.h (or the cleaned ones of dcs_rfi.h) folded at a
 * pulsar's predicted phase into pulse profiles per sub-integration, channel and phase bin, the third product of a tied-array
 * beamformer beside the single-pulse candidates and the visibilities.  Two calls: the fold itself, and the frequency scrunch
 * of its profiles into the sub-integration/phase plane that leaves the GPU for a timing diagnostic.  A profile word is a sum
 * of bytes and the phase is integer arithmetic, so both results are stated, and tested, bit for bit.
 *
 * Library: dc_sand_amd/csrc/libdcs_fold.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 * nr_channels (C) is the context's.  nr_beams (B) is an ARGUMENT, any value >= 1, as in dcs_filterbank.h.  No delay-model
 * table is needed and dcs_bf_tuning.math_mode plays no part.
 *
 * The phase model.  dcs_bf_fold_model {phase0, step, accel} is 24 bytes, 8-byte aligned, in units of 2^-64 turn; every
 * operation on it is modulo 2^64, the same kind of integer phase accumulator as the down-converter's oscillator: no drift
 * and no floating point on the device.  For spectrum k, 0 <= k < subint_len, of a sub-integration and nbin phase bins
 *     phi(k) = phase0 + k * step + (k (k - 1) / 2) * accel     (uint64, wraps; k (k - 1) / 2 is exact since k < 2^32)
 *     bin(k) = ((phi(k) >> 32) * nbin) >> 32                   (0 .. nbin - 1, for any nbin, not only powers of two)
 *   A negative accel is its two's complement.  A model advanced by m spectra is {phi(m), step + m * accel, accel}, exactly
 *   modulo 2^64: phi'(k) = phi(m + k) for every k.  So a sub-integration cut anywhere and folded in two calls, the second
 *   with the advanced model, first_spectrum + m and accumulate = 1, gives the bits of one call.
 *
 * Tensors, all caller-owned device memory, read when the work runs, not when it is enqueued.  P = nr_beams /
 * beams_per_model; beam b uses the model row and the delay row p = b / beams_per_model (4 for the Stokes filterbanks of
 * nr_beams = 4 B, which fold with one model per pointing; 1 otherwise).
 * d_filterbank: const uint8_t [nr_beams][in_spectra][C], channel fastest, 16-byte aligned: exactly what
 *   dcs_bf_filterbank_q8 and dcs_bf_rfi_clean_q8 write.
 * d_models: const dcs_bf_fold_model [P][nr_subints], 8-byte aligned.
 * d_delays: NULL (every delay 0), or const int32_t [P][C], 4-byte aligned, in whole spectra: what dcs_bf_dm_delays makes of
 *   a double [P] list of DMs, one per pointing.
 * d_channel_mask: NULL, or const uint8_t [C]; a zero byte folds the column to zero.
 * d_profiles: uint32_t [nr_beams][out_subints][C][nbin], bin fastest, 4-byte aligned.
 * d_hits: NULL (not wanted), or uint32_t [P][out_subints][nbin], 4-byte aligned.
 * d_scrunched: uint64_t [nr_beams][out_subints][nbin], 8-byte aligned.
 *
 * dcs_bf_fold_q8.  Sub-integration s < nr_subints covers the rows first_spectrum + s * subint_len + k of every beam and is
 *   placed at first_subint + s of the outputs.  With on(p, c) = (mask[c] != 0 and 0 <= d_delays[p][c] <= max_delay) and
 *   bin_{p,s} the bins of d_models[p][s], the call writes (accumulate = 0) or adds modulo 2^32 (accumulate = 1)
 *     d_profiles[b][first_subint + s][c][j]  (=|+=)  on(p, c) ? sum over the k with bin_{p,s}(k) == j of
 *                                d_filterbank[b][first_spectrum + s * subint_len + k + d_delays[p][c]][c]  :  0
 *     d_hits[p][first_subint + s][j]         (=|+=)  #{ k : bin_{p,s}(k) == j }
 *   for every j < nbin and NO OTHER WORD of either output.  The delay moves the read, not the bin: a dedispersed profile is
 *   the plain sum over c, and the hits do not depend on the channel.  subint_len <= 2^24, so no word wraps without
 *   accumulate (255 * 2^24 < 2^32).  A table entry outside [0, max_delay] folds its column to zero; INT32_MAX and every
 *   negative entry are always outside.  So no table can make the call read outside the rows [first_spectrum,
 *   first_spectrum + nr_subints * subint_len + max_delay) of a beam, and that window is checked by value.  The result is an
 *   exact integer and does not depend on the launch geometry: the only atomics are integer adds on words in LDS, whose
 *   order cannot show; every word of global memory is written by exactly one thread.  nr_subints == 0 enqueues nothing and
 *   succeeds.
 *
 * dcs_bf_fold_scrunch writes (accumulate = 0) or adds modulo 2^64 (accumulate = 1), for first_subint <= s < first_subint +
 *   nr_subints and j < nbin,
 *     d_scrunched[b][s][j]  (=|+=)  sum over c < C of d_profiles[b][s][c][j]                          (uint64, exact)
 *   and no other word: the frequency-scrunched sub-integration/phase plane, C times smaller than the profiles.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, d_filterbank, d_models,
 * d_profiles or d_scrunched as they apply; pointers not aligned as stated above; nr_beams == 0; beams_per_model == 0 or no
 * divisor of nr_beams; nbin outside 1 .. 1024; subint_len outside 1 .. 2^24; max_delay > 2^31 - 2; first_spectrum +
 * nr_subints * subint_len + max_delay > in_spectra; first_subint + nr_subints > out_subints; accumulate > 1.  Then, with
 * DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a libdcs_beamformer.so of another build.  Then buffers smaller
 * than the tensors above (filterbank_bytes, models_bytes, delays_bytes where d_delays is given, profiles_bytes, hits_bytes
 * where d_hits is given, scrunched_bytes) are DCS_ERR_INVALID_ARGUMENT.  Capture: both calls only launch kernels (no memset
 * node is needed) and allocate nothing, not on a context's first call either, so they can always be captured.
 */
#ifndef DCS_FOLD_H
#define DCS_FOLD_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* device memory, read when the work runs: one sub-integration's phase polynomial in units of 2^-64 turn */
typedef struct {
    uint64_t phase0, step, accel;
} dcs_bf_fold_model;

/* filterbanks uint8 [nr_beams][in_spectra][C], models [P][nr_subints] and delays int32 [P][C] -> sub-integrations first_subint ..
   first_subint + nr_subints - 1 of the profiles uint32 [nr_beams][out_subints][C][nbin] and of the hits uint32 [P][out_subints][nbin] */
int dcs_bf_fold_q8(dcs_bf_context *ctx, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                   uint64_t first_spectrum, uint32_t subint_len, uint32_t nr_subints, uint32_t nr_beams,
                   uint32_t beams_per_model, const dcs_bf_fold_model *d_models, size_t models_bytes, const int32_t *d_delays,
                   size_t delays_bytes, uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t nbin, uint32_t *d_profiles,
                   size_t profiles_bytes, uint32_t *d_hits, size_t hits_bytes, uint64_t out_subints, uint64_t first_subint,
                   uint32_t accumulate, void *stream);
/* profiles uint32 [nr_beams][out_subints][C][nbin] -> the same sub-integrations of uint64 [nr_beams][out_subints][nbin], summed over C */
int dcs_bf_fold_scrunch(dcs_bf_context *ctx, const uint32_t *d_profiles, size_t profiles_bytes, uint32_t nr_beams,
                        uint64_t out_subints, uint64_t first_subint, uint32_t nr_subints, uint32_t nbin, uint64_t *d_scrunched,
                        size_t scrunched_bytes, uint32_t accumulate, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_FOLD_H */
