// bf_beam_quant.cpp -- include/dcs_beam_quant.h, the companion library libdcs_beam_quant.so.  Host code only: the
// quantised beamformer is libdcs_beamformer.so's, reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_beam_quant.h"

#include "bf_ctx_ext.h"

namespace {

bool args_ok(dcs_bf_context *c, uint32_t nt, const float *d_weights, const float *d_quant_gains,
             const unsigned long long *d_clip_count)
{
    return c && d_quant_gains && !(reinterpret_cast<uintptr_t>(d_quant_gains) & 3u) &&
           !(reinterpret_cast<uintptr_t>(d_weights) & 3u) && !(reinterpret_cast<uintptr_t>(d_clip_count) & 7u) && nt % 16u == 0u;
}

} // namespace

extern "C" {

int dcs_bf_beamform_accumulated_q8(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                   size_t antenna_bytes, const float *d_weights, const float *d_quant_gains,
                                   int8_t *d_beams_q8, size_t beams_bytes, unsigned long long *d_clip_count, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, d_quant_gains, d_clip_count)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_q8(ctx, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, d_quant_gains,
                                              d_beams_q8, beams_bytes, d_clip_count, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_q8_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                      size_t antenna_bytes, const float *d_weights, const float *d_quant_gains,
                                      int8_t *d_beams_q8, size_t beams_bytes, unsigned long long *d_clip_count, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, d_quant_gains, d_clip_count)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_q8(ctx, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, d_quant_gains,
                                              d_beams_q8, beams_bytes, d_clip_count, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
