// bf_incoherent_beam.cpp -- include/dcs_incoherent_beam.h, the companion library libdcs_incoherent_beam.so.  Host code
// only: the kernels are libdcs_beamformer.so's (bf_incoherent.hip, bf_integrate.hip), reached through the table at the head of every
// context it makes (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_incoherent_beam.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_incoherent_block_power(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                  const float *d_weights, uint32_t *d_block_power, size_t power_bytes, void *stream)
{
    if (int e = incoherent_block_power_args(ctx, nt, d_weights, d_block_power)) return e;
    return forward(ctx, &bf_ctx_ext_ops::incoherent_block_power, nt, d_antenna, antenna_bytes, d_weights, d_block_power, power_bytes,
                   stream);
}

int dcs_bf_integrate_incoherent_power(dcs_bf_context *ctx, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                      uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                      void *stream)
{
    if (int e = integrate_incoherent_power_args(ctx, d_block_power, nr_blocks, blocks_per_spectrum, d_spectra)) return e;
    return forward(ctx, &bf_ctx_ext_ops::integrate_incoherent_power, d_block_power, power_bytes, nr_blocks, blocks_per_spectrum,
                   accumulate, d_spectra, spectra_bytes, stream);
}

} // extern "C"
