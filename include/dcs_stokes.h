/*
 * dcs_stokes.h -- full-Stokes detection of dual-polarisation 8-bit voltage beams: the two int8 beam tensors that
 * dcs_bf_beamform_accumulated_complex_q8 (dcs_beam_complex_quant.h) makes of a telescope's two polarisations, one call
 * per polarisation with the same coefficients, combined into the Stokes parameters I (for searching) or I, Q, U, V (for
 * timing and polarimetry) per channel, 16-sample block and beam, and integrated in time like the incoherent beam of
 * dcs_incoherent_beam.h.  The cross terms Re(x y*) and Im(x y*) cannot be recovered from the two polarisations' detected
 * powers, so no composition of the other calls gives Q, U or V.  Every term is an integer, so the stated arithmetic is
 * exact: there is no rounding before the one conversion to float at the end of an integration.
 *
 * Library: dc_sand_amd/csrc/libdcs_stokes.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns, and
 * nr_channels (C) and nr_beams (B) are the context's.  libdcs_beamformer.so itself keeps its ABI version 3 and its entry
 * points unchanged.  Status codes as dcs_beamformer.h.  No delay table is needed: there are no coefficients, hence no
 * coefficient time and no _dt entry points, and dcs_bf_tuning.math_mode plays no part.
 *
 * Tensors.
 * d_beams_x, d_beams_y: the beams of polarisation x and of polarisation y, each int8 [C][nt / 16][B][16][{re, im}] as
 *   dcs_beam_quant.h lays them out, C * nt * B * 2 bytes, 16-byte aligned, nt % 16 == 0.  d_beams_x == d_beams_y is legal
 *   and gives I = 2 Pxx, Q = 0, U = 2 Pxx, V = 0.  -128 IS ARITHMETIC LIKE ANY OTHER BYTE: the quantiser upstream uses it
 *   to mark a NaN and its clip counters report that; this call does not special-case it.  The two polarisations should
 *   have been quantised with the same per-beam gain, or Q is biased; that is the caller's to see to and is not checked.
 * nr_stokes: DCS_BF_STOKES_I (1) writes I only; DCS_BF_STOKES_IQUV (4) writes I, Q, U, V in that order, innermost.
 * d_block_stokes: int32_t [C][nt / 16][B][nr_stokes], C * (nt / 16) * B * nr_stokes * 4 bytes, aligned to 4 * nr_stokes
 *   bytes, caller-owned.  With x_t = (xr, xi) and y_t = (yr, yi) the 16 samples t of one (channel, block, beam) in the
 *   two tensors, all sums exact integers:
 *     Pxx = sum_t xr^2 + xi^2          Pyy = sum_t yr^2 + yi^2
 *     Cr  = sum_t xr yr + xi yi        (= Re sum_t x conj(y))
 *     Ci  = sum_t xi yr - xr yi        (= Im sum_t x conj(y))
 *     I = Pxx + Pyy    Q = Pxx - Pyy    U = 2 Cr    V = 2 Ci
 *   THE SIGN OF V IS THIS FORMULA'S: x = i, y = 1 in every sample gives V = +2 per sample.  Which handedness of circular
 *   polarisation that is depends on the caller's feeds; there is no flag for it.  |I|, |Q|, |U|, |V| <= 16 * 2 * 2 * 128^2
 *   = 2^20, so 32 bits are ample; any order of summation gives the same bits, so the result cannot depend on the launch
 *   geometry.  Ci is formed from the two sums sum_t xi yr and sum_t xr yi, subtracted as 32-bit integers: no byte of either
 *   operand is negated, so -128 needs no care.
 * d_spectra: float [nr_blocks / blocks_per_spectrum][C][B][nr_stokes], time-major, aligned to 4 * nr_stokes bytes,
 *   caller-owned: successive calls that write behind each other append to one time series.  It is a legal spectra tensor
 *   of dcs_filterbank.h with nr_beams = nr_stokes * B: series nr_stokes * b + s is Stokes s of beam b.
 *
 * Integration (dcs_bf_integrate_stokes), n = blocks_per_spectrum.  For every spectrum i, channel c, beam b and Stokes s,
 *   S = sum_j block[c][i * n + j][b][s], j = 0 .. n - 1, exactly, in signed 64 bits; the output is RN((float)S): ONE
 *   rounding, to nearest, ties to even.  With accumulate non-zero it is RN(old + RN((float)S)), old being what
 *   d_spectra[i][c][b][s] held.  No float atomics.  nr_blocks is the block count of d_block_stokes (nt / 16 of the call that
 *   wrote it) and nr_stokes the one it was written with.
 * An output must not overlap an input: the result of a call whose output overlaps one of its inputs is undefined.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, a NULL input or a NULL
 * output, nr_stokes other than 1 and 4, a pointer that is not aligned as stated above, nt % 16 != 0, blocks_per_spectrum
 * == 0 or nr_blocks % blocks_per_spectrum != 0.  Then, with DCS_ERR_UNSUPPORTED and nothing enqueued: a context made by a
 * libdcs_beamformer.so of another build.  Then buffers smaller than the tensors above: DCS_ERR_INVALID_ARGUMENT.  nt == 0
 * and nr_blocks == 0 enqueue nothing and succeed.  Capture: both calls only launch kernels and allocate nothing, not on a
 * context's first call either, so both can always be captured.
 */
#ifndef DCS_STOKES_H
#define DCS_STOKES_H

#include "dcs_beamformer.h"

#define DCS_BF_STOKES_I 1u
#define DCS_BF_STOKES_IQUV 4u

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* two int8 beam tensors [C][nt / 16][B][16][2] (polarisations x and y) -> exact block Stokes int32 [C][nt / 16][B][nr_stokes] */
int dcs_bf_stokes_block(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                        uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream);
/* block Stokes [C][nr_blocks][B][nr_stokes] summed blocks_per_spectrum at a time -> float [nr_blocks / n][C][B][nr_stokes] */
int dcs_bf_integrate_stokes(dcs_bf_context *ctx, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                            uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                            size_t spectra_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_STOKES_H */
