// bf_beam_complex.cpp -- include/dcs_beam_complex.h, the companion library libdcs_beam_complex.so.  Host code only: the
// complex-product beamformer is libdcs_beamformer.so's, reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_beam_complex.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned4(const void *p) { return !(reinterpret_cast<uintptr_t>(p) & 3u); }

// d_out: the float beams (8-byte aligned) or the block powers (4-byte aligned)
bool args_ok(dcs_bf_context *c, uint32_t nt, const float *d_weights, uint32_t flags, const float *d_out, uintptr_t out_mask)
{
    return c && d_out && !(reinterpret_cast<uintptr_t>(d_out) & out_mask) && aligned4(d_weights) && nt % 16u == 0u &&
           !(flags & ~(uint32_t)DCS_BF_COMPLEX_CONJ);
}

} // namespace

extern "C" {

int dcs_bf_beamform_accumulated_complex(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                        size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams,
                                        size_t beams_bytes, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, flags, d_beams, 7u)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_complex(ctx, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, flags, d_beams,
                                                   beams_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_complex_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                           size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams,
                                           size_t beams_bytes, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, flags, d_beams, 7u)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_complex(ctx, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, flags, d_beams,
                                                   beams_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_complex_power(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                              size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_block_power,
                                              size_t power_bytes, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, flags, d_block_power, 3u)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_complex_power(ctx, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, flags,
                                                         d_block_power, power_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_complex_power_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                                 size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                                 float *d_block_power, size_t power_bytes, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, flags, d_block_power, 3u)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_complex_power(ctx, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, flags,
                                                         d_block_power, power_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
