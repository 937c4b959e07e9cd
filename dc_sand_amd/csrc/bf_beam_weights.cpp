// bf_beam_weights.cpp -- include/dcs_beam_weights.h, the companion library libdcs_beam_weights.so.  Host code only: the
// weighted pre-pass and beamformers are libdcs_beamformer.so's, reached through the table at the head of every context it
// makes (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_beam_weights.h"

#include "bf_ctx_ext.h"

namespace {

bool args_ok(dcs_bf_context *c, uint32_t nt, const float *d_weights)
{
    return c && d_weights && !(reinterpret_cast<uintptr_t>(d_weights) & 3u) && nt % 16u == 0u;
}

} // namespace

extern "C" {

int dcs_bf_generate_and_beamform_weighted(dcs_bf_context *ctx, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                          size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                          void *stream)
{
    if (!args_ok(ctx, nt, d_weights) || t0 % 16u) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->generate_and_beamform_weighted(ctx, nullptr, t0, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                                                     beams_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_generate_and_beamform_weighted_dt(dcs_bf_context *ctx, const float *dt, uint32_t nt, const int8_t *d_antenna,
                                             size_t antenna_bytes, const float *d_weights, float *d_beams,
                                             size_t beams_bytes, void *stream)
{
    if (!args_ok(ctx, nt, d_weights) || (!dt && nt)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->generate_and_beamform_weighted(ctx, dt, 0, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                                                     beams_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_weighted(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                         size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                         void *stream)
{
    if (!args_ok(ctx, nt, d_weights)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_weighted(ctx, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                                                    beams_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_weighted_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                            size_t antenna_bytes, const float *d_weights, float *d_beams,
                                            size_t beams_bytes, void *stream)
{
    if (!args_ok(ctx, nt, d_weights)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_weighted(ctx, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                                                    beams_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
