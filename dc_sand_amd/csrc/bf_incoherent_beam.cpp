// bf_incoherent_beam.cpp -- include/dcs_incoherent_beam.h, the companion library libdcs_incoherent_beam.so.  Host code
// only: the kernels are libdcs_beamformer.so's (bf_incoherent.hip), reached through the table at the head of every
// context it makes (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_incoherent_beam.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned4(const void *p) { return !(reinterpret_cast<uintptr_t>(p) & 3u); }

} // namespace

extern "C" {

int dcs_bf_incoherent_block_power(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                  const float *d_weights, uint32_t *d_block_power, size_t power_bytes, void *stream)
{
    if (!ctx || !d_block_power || !aligned4(d_block_power) || !aligned4(d_weights) || nt % 16u) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->incoherent_block_power(ctx, nt, d_antenna, antenna_bytes, d_weights, d_block_power, power_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_integrate_incoherent_power(dcs_bf_context *ctx, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                      uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                      void *stream)
{
    if (!ctx || !d_block_power || !d_spectra || !aligned4(d_block_power) || !aligned4(d_spectra)) return DCS_ERR_INVALID_ARGUMENT;
    if (blocks_per_spectrum == 0u || nr_blocks % blocks_per_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->integrate_incoherent_power(ctx, d_block_power, power_bytes, nr_blocks, blocks_per_spectrum, accumulate,
                                                 d_spectra, spectra_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
