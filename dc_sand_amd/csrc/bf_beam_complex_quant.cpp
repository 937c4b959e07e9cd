// bf_beam_complex_quant.cpp -- include/dcs_beam_complex_quant.h, the companion library libdcs_beam_complex_quant.so.  Host
// code only: the quantised complex-product beamformer is libdcs_beamformer.so's, reached through the table at the head of
// every context it makes (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_beam_complex_quant.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_beamform_accumulated_complex_q8(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                           size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                           const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                           unsigned long long *d_clip_count, void *stream)
{
    if (int e = beamform_accumulated_complex_q8_args(ctx, nt, d_weights, flags, d_quant_gains, d_beams_q8, d_clip_count)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_complex_q8, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights,
                   flags, d_quant_gains, d_beams_q8, beams_bytes, d_clip_count, stream);
}

int dcs_bf_beamform_accumulated_complex_q8_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                              size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                              const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                              unsigned long long *d_clip_count, void *stream)
{
    if (int e = beamform_accumulated_complex_q8_args(ctx, nt, d_weights, flags, d_quant_gains, d_beams_q8, d_clip_count)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_complex_q8, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, flags,
                   d_quant_gains, d_beams_q8, beams_bytes, d_clip_count, stream);
}

} // extern "C"
