// bf_beam_power.cpp -- include/dcs_beam_power.h, the companion library libdcs_beam_power.so.  Host code only: the
// detecting beamformer and the integrator are libdcs_beamformer.so's, reached through the table at the head of every
// context it makes (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_beam_power.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned4(const void *p) { return !(reinterpret_cast<uintptr_t>(p) & 3u); }

bool args_ok(dcs_bf_context *c, uint32_t nt, const float *d_weights, const float *d_block_power)
{
    return c && d_block_power && aligned4(d_block_power) && aligned4(d_weights) && nt % 16u == 0u;
}

} // namespace

extern "C" {

int dcs_bf_beamform_accumulated_power(dcs_bf_context *ctx, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                      size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                      void *stream)
{
    if (!args_ok(ctx, nt, d_weights, d_block_power)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_power(ctx, nullptr, t_coeff, nt, d_antenna, antenna_bytes, d_weights, d_block_power,
                                                 power_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_beamform_accumulated_power_dt(dcs_bf_context *ctx, float dt_coeff, uint32_t nt, const int8_t *d_antenna,
                                         size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                         void *stream)
{
    if (!args_ok(ctx, nt, d_weights, d_block_power)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->beamform_accumulated_power(ctx, &dt_coeff, 0, nt, d_antenna, antenna_bytes, d_weights, d_block_power,
                                                 power_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_integrate_block_power(dcs_bf_context *ctx, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                 uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                 void *stream)
{
    if (!ctx || !d_block_power || !d_spectra || !aligned4(d_block_power) || !aligned4(d_spectra)) return DCS_ERR_INVALID_ARGUMENT;
    if (blocks_per_spectrum == 0u || nr_blocks % blocks_per_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->integrate_block_power(ctx, d_block_power, power_bytes, nr_blocks, blocks_per_spectrum, accumulate, d_spectra,
                                            spectra_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
