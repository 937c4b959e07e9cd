/*
 * dcs_candidates.h -- the candidate sifter: the signal-to-noise planes of dcs_single_pulse.h as a list of single-pulse
 * candidates.  A bright pulse lights up dozens of neighbouring DMs, widths and blocks; the sifter collapses the width axis,
 * keeps the cells at or above a threshold that no neighbour within two radii beats, and writes them, compacted and in
 * order, as 32-byte records with a count -- on the device, inside a captured graph, where a host pass over the planes
 * cannot live.  The arithmetic is fp32 compares and integer counts only; it is stated below and tested bit for bit.
 *
 * Library: dc_sand_amd/csrc/libdcs_candidates.so, a companion of libdcs_beamformer.so built with it from the same tree
 * (`python -m dc_sand_amd.build`); it takes the dcs_bf_context handles that library's dcs_bf_create returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 * nr_beams (B) is an ARGUMENT, any value >= 1, as in dcs_single_pulse.h; of the context the call uses its device, nothing
 * else.
 *
 * Tensors, all caller-owned device memory, read and written when the work runs, not when it is enqueued.
 * d_snr: const float [B][nr_dm][nr_widths][peak_blocks], 4-byte aligned: exactly what dcs_bf_peak_snr writes.
 * d_peaks: const uint32_t [B][nr_dm][nr_widths][peak_blocks][2] = {value, time}, 8-byte aligned: exactly what
 *   dcs_bf_boxcar_peaks writes.
 * d_cands: dcs_bf_candidate [max_candidates], 8-byte aligned; NULL is allowed where max_candidates == 0.
 * d_count: uint32_t [2], 4-byte aligned.
 * d_work: dcs_bf_candidates_workspace_bytes(B, nr_dm, nr_blocks) bytes, 8-byte aligned; scratch of the call, of no meaning
 *   afterwards.  The function is pure host code and needs no context; it is monotone in each argument, 0 only for an empty
 *   shape, and SIZE_MAX where the figure does not fit a size_t.
 *
 * dcs_bf_find_candidates, for the blocks k of [first_block, first_block + nr_blocks) -- a cell is one (beam b, DM m,
 * block k); the cells of a beam form the rectangle [0, nr_dm) x [first_block, first_block + nr_blocks), and cells outside
 * it do not exist:
 *
 *  1. Cell.  s = -infinity, i* = 0xFFFFFFFF; for i = 0 .. nr_widths - 1 in order: if d_snr[b][m][i][k] > s then
 *     s = d_snr[b][m][i][k], i* = i.  A NaN never compares greater and is skipped.  Where dcs_bf_peak_snr made d_snr, i* is
 *     its d_best[b][m][k].
 *  2. Order.  Cell Q beats cell P when s_Q > s_P, or s_Q == s_P and (m_Q, k_Q) is lexicographically smaller than
 *     (m_P, k_P).  All compares are fp32 IEEE compares: +0 == -0 holds, and a NaN gives false.
 *  3. Candidate.  P is a candidate when s_P >= threshold and no cell Q of the same beam with |m_Q - m_P| <= dm_radius and
 *     |k_Q - k_P| <= block_radius beats it.  A plateau of equal values yields exactly one candidate, its lexicographically
 *     first cell; radius 0 in both axes yields every cell at or above threshold.  Only existing cells take part: a caller
 *     who cuts a series into calls overlaps consecutive calls by block_radius blocks (and drops the candidates of the
 *     overlap that the neighbouring call decides with its fuller window).
 *  4. Record.  {beam, dm, block} = the cell (block is k itself, not k - first_block); width_index = i*; {value, time} =
 *     the two words of d_peaks[b][m][i*][k], unchanged; snr = the bits of s; members = the number of cells Q of the window
 *     of 3. with s_Q >= threshold, P included: an exact integer.
 *  5. List.  The candidates in ascending (b, m, k).  d_count[0] = the number of candidates found, d_count[1] =
 *     min(found, max_candidates); the first d_count[1] records of d_cands are written and NO OTHER BYTE of it.  With
 *     max_candidates == 0 the call only counts.
 *  6. Determinism.  The result does not depend on the launch geometry: no float atomics, and no atomic decides a position
 *     in the list (there are no atomics at all).
 *
 * 0 <= dm_radius, block_radius <= 8.  nr_widths == 0 makes every cell -infinity, so nothing is found.  nr_blocks == 0 or
 * nr_dm == 0 enqueues only what zeroes d_count, and succeeds.
 *
 * Arguments refused with DCS_ERR_INVALID_ARGUMENT before the context is touched: a NULL context, d_snr, d_peaks, d_count or
 * d_work; a NULL d_cands with max_candidates != 0; pointers not aligned as stated above; nr_beams == 0; a radius above 8; a
 * threshold that is not finite; first_block + nr_blocks > peak_blocks.  Then, with DCS_ERR_UNSUPPORTED and nothing
 * enqueued: a context made by a libdcs_beamformer.so of another build; B * nr_dm * nr_blocks >= 2^32 (the counts are 32-bit
 * words) or first_block + nr_blocks > 2^32 (block is one).  Then buffers smaller than the tensors above, work_bytes and
 * cands_bytes (32 max_candidates) included, are DCS_ERR_INVALID_ARGUMENT.  Capture: the call only launches kernels -- at
 * most three -- and allocates nothing, not on a context's first call either, so it can always be captured; a replay follows
 * new d_snr and d_peaks contents.
 */
#ifndef DCS_CANDIDATES_H
#define DCS_CANDIDATES_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* one candidate: 32 bytes */
typedef struct dcs_bf_candidate {
    uint32_t beam;
    uint32_t dm;          /* DM index m */
    uint32_t width_index; /* i*: the lowest width index with the cell's largest signal-to-noise */
    uint32_t block;       /* k */
    uint32_t time;        /* d_peaks[b][m][i*][k][1] */
    uint32_t value;       /* d_peaks[b][m][i*][k][0] */
    float snr;            /* s */
    uint32_t members;     /* cells of the window at or above threshold, this one included */
} dcs_bf_candidate;

/* bytes of d_work for a call of this shape; host code, no context */
size_t dcs_bf_candidates_workspace_bytes(uint32_t nr_beams, uint32_t nr_dm, uint32_t nr_blocks);
/* signal-to-noise and peaks, blocks first_block .. first_block + nr_blocks - 1 -> the candidates in ascending (b, m, k) and
   d_count = {found, written} */
int dcs_bf_find_candidates(dcs_bf_context *ctx, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                           uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                           uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, dcs_bf_candidate *d_cands,
                           size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_CANDIDATES_H */
