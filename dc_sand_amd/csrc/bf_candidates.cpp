// bf_candidates.cpp -- include/dcs_candidates.h, the companion library libdcs_candidates.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_candidates.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The export makes its entry's device-free checks (bf_arg_checks.h), then forwards; the workspace figure is
// bf_arg_checks.h's, the one the implementation behind the table holds work_bytes to.

#include "../../include/dcs_candidates.h"

#include "bf_ctx_ext.h"

extern "C" {

size_t dcs_bf_candidates_workspace_bytes(uint32_t nr_beams, uint32_t nr_dm, uint32_t nr_blocks)
{
    return candidates_workspace_bytes(nr_beams, nr_dm, nr_blocks);
}

int dcs_bf_find_candidates(dcs_bf_context *ctx, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                           uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                           uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, dcs_bf_candidate *d_cands,
                           size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes, void *stream)
{
    if (int e = find_candidates_args(ctx, d_snr, d_peaks, peak_blocks, first_block, nr_blocks, nr_beams, threshold, dm_radius,
                                     block_radius, d_cands, max_candidates, d_count, d_work))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::find_candidates, d_snr, snr_bytes, d_peaks, peaks_bytes, peak_blocks, first_block, nr_blocks,
                   nr_beams, nr_dm, nr_widths, threshold, dm_radius, block_radius, static_cast<void *>(d_cands), cands_bytes,
                   max_candidates, d_count, d_work, work_bytes, stream);
}

} // extern "C"
