// bf_beam_complex_quant.cpp -- include/dcs_beam_complex_quant.h, the companion library libdcs_beam_complex_quant.so.  Host
// code only: the quantised complex-product beamformer is libdcs_beamformer.so's, reached through the table at the head of
// every context it makes (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_beam_complex_quant.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned(const void *p, uintptr_t mask) { return !(reinterpret_cast<uintptr_t>(p) & mask); }

bool args_ok(dcs_bf_context *c, uint32_t nt, const float *d_weights, uint32_t flags, const float *d_quant_gains,
             const int8_t *d_beams_q8, const unsigned long long *d_clip_count)
{
    return c && d_quant_gains && d_beams_q8 && aligned(d_quant_gains, 3u) && aligned(d_weights, 3u) && aligned(d_clip_count, 7u) &&
           aligned(d_beams_q8, 7u) && nt % 16u == 0u && !(flags & ~(uint32_t)DCS_BF_COMPLEX_CONJ);
}

} // namespace

extern "C" {

int dcs_bf_beamform_accumulated_complex_q8(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                           size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                           const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                           unsigned long long *d_clip_count, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, flags, d_quant_gains, d_beams_q8, d_clip_count)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_complex_q8(ctx, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, flags,
                                                      d_quant_gains, d_beams_q8, beams_bytes, d_clip_count, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_complex_q8_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                              size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                              const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                              unsigned long long *d_clip_count, void *stream)
{
    if (!args_ok(ctx, nt, d_weights, flags, d_quant_gains, d_beams_q8, d_clip_count)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_complex_q8(ctx, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, flags,
                                                      d_quant_gains, d_beams_q8, beams_bytes, d_clip_count, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
