// bf_channeliser.cpp -- include/dcs_channeliser.h, the companion library libdcs_channeliser.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_channeliser.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_channeliser.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_channelise(dcs_bf_context *ctx, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                      const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles,
                      uint32_t order, float *d_out, size_t out_bytes, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs,
                      uint32_t first_input, void *stream)
{
    if (int e = channelise_args(ctx, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles, order,
                                d_out, 4u, out_bytes, out_blocks, first_block, out_inputs, first_input))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::channelise, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps,
                   d_twiddles, order, d_out, out_bytes, out_blocks, first_block, out_inputs, first_input, stream);
}

int dcs_bf_channelise_q8(dcs_bf_context *ctx, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                         const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles,
                         uint32_t order, const float *d_gains, int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks,
                         uint64_t first_block, uint32_t out_inputs, uint32_t first_input, unsigned long long *d_clip_count,
                         void *stream)
{
    if (int e = channelise_q8_args(ctx, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles,
                                   order, d_gains, d_out_q8, out_bytes, out_blocks, first_block, out_inputs, first_input, d_clip_count))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::channelise_q8, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps,
                   d_twiddles, order, d_gains, d_out_q8, out_bytes, out_blocks, first_block, out_inputs, first_input, d_clip_count,
                   stream);
}

} // extern "C"
