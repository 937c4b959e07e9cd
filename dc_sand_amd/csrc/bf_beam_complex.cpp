// bf_beam_complex.cpp -- include/dcs_beam_complex.h, the companion library libdcs_beam_complex.so.  Host code only: the
// complex-product beamformer is libdcs_beamformer.so's, reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_beam_complex.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_beamform_accumulated_complex(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                        size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams,
                                        size_t beams_bytes, void *stream)
{
    if (int e = beamform_accumulated_complex_args(ctx, nt, d_weights, flags, d_beams)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_complex, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, flags,
                   d_beams, beams_bytes, stream);
}

int dcs_bf_beamform_accumulated_complex_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                           size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams,
                                           size_t beams_bytes, void *stream)
{
    if (int e = beamform_accumulated_complex_args(ctx, nt, d_weights, flags, d_beams)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_complex, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, flags,
                   d_beams, beams_bytes, stream);
}

int dcs_bf_beamform_accumulated_complex_power(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                              size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_block_power,
                                              size_t power_bytes, void *stream)
{
    if (int e = beamform_accumulated_complex_power_args(ctx, nt, d_weights, flags, d_block_power)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_complex_power, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights,
                   flags, d_block_power, power_bytes, stream);
}

int dcs_bf_beamform_accumulated_complex_power_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                                 size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                                 float *d_block_power, size_t power_bytes, void *stream)
{
    if (int e = beamform_accumulated_complex_power_args(ctx, nt, d_weights, flags, d_block_power)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_complex_power, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights,
                   flags, d_block_power, power_bytes, stream);
}

} // extern "C"
