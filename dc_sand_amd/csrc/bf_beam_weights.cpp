// bf_beam_weights.cpp -- include/dcs_beam_weights.h, the companion library libdcs_beam_weights.so.  Host code only: the
// weighted pre-pass and beamformers are libdcs_beamformer.so's, reached through the table at the head of every context it
// makes (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_beam_weights.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_generate_and_beamform_weighted(dcs_bf_context *ctx, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                          size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                          void *stream)
{
    if (int e = generate_and_beamform_weighted_args(ctx, nullptr, t0, nt, d_weights)) return e;
    return forward(ctx, &bf_ctx_ext_ops::generate_and_beamform_weighted, nullptr, t0, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                   beams_bytes, stream);
}

// behind the table a null dt means "the time index", so the one check that an export alone can make is made here
int dcs_bf_generate_and_beamform_weighted_dt(dcs_bf_context *ctx, const float *dt, uint32_t nt, const int8_t *d_antenna,
                                             size_t antenna_bytes, const float *d_weights, float *d_beams,
                                             size_t beams_bytes, void *stream)
{
    if (!dt && nt) return DCS_ERR_INVALID_ARGUMENT;
    if (int e = generate_and_beamform_weighted_args(ctx, dt, 0, nt, d_weights)) return e;
    return forward(ctx, &bf_ctx_ext_ops::generate_and_beamform_weighted, dt, 0, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                   beams_bytes, stream);
}

int dcs_bf_beamform_accumulated_weighted(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                         size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                         void *stream)
{
    if (int e = beamform_accumulated_weighted_args(ctx, nt, d_weights)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_weighted, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights,
                   d_beams, beams_bytes, stream);
}

int dcs_bf_beamform_accumulated_weighted_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                            size_t antenna_bytes, const float *d_weights, float *d_beams,
                                            size_t beams_bytes, void *stream)
{
    if (int e = beamform_accumulated_weighted_args(ctx, nt, d_weights)) return e;
    return forward(ctx, &bf_ctx_ext_ops::beamform_accumulated_weighted, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, d_beams,
                   beams_bytes, stream);
}

} // extern "C"
