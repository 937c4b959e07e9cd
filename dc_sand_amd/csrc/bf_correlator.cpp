// bf_correlator.cpp -- include/dcs_correlator.h, the companion library libdcs_correlator.so.  Host code only: the kernels
// are libdcs_beamformer.so's (bf_correlator.hip, bf_integrate.hip), reached through the table at the head
// of every context it makes (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_correlator.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_correlate_block(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, uint32_t blocks_per_vis,
                           int32_t *d_vis, size_t vis_bytes, void *stream)
{
    if (int e = correlate_block_args(ctx, nt, blocks_per_vis, d_vis)) return e;
    return forward(ctx, &bf_ctx_ext_ops::correlate_block, nt, d_antenna, antenna_bytes, blocks_per_vis, d_vis, vis_bytes, stream);
}

int dcs_bf_integrate_visibilities(dcs_bf_context *ctx, const int32_t *d_vis, size_t vis_bytes, uint32_t nr_vis,
                                  uint32_t vis_per_integration, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream)
{
    if (int e = integrate_visibilities_args(ctx, d_vis, nr_vis, vis_per_integration, d_out)) return e;
    return forward(ctx, &bf_ctx_ext_ops::integrate_visibilities, d_vis, vis_bytes, nr_vis, vis_per_integration, accumulate, d_out,
                   out_bytes, stream);
}

} // extern "C"
