// bf_ddc.cpp -- include/dcs_ddc.h, the companion library libdcs_ddc.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_ddc.hip), reached through the table at the head of every context it makes (bf_ctx_ext.h).
// Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_ddc.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_ddc_tap_digits(dcs_bf_context *ctx, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, void *d_digits,
                          size_t digits_bytes, void *stream)
{
    if (int e = ddc_tap_digits_args(ctx, d_taps, nr_taps, nr_bands, d_digits, digits_bytes)) return e;
    return forward(ctx, &bf_ctx_ext_ops::ddc_tap_digits, d_taps, nr_taps, nr_bands, d_digits, digits_bytes, stream);
}

int dcs_bf_ddc(dcs_bf_context *ctx, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes,
               uint64_t in_stride, const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands,
               const dcs_ddc_band *bands, uint64_t first_output, float *d_out, size_t out_bytes, uint64_t out_stride, void *stream)
{
    if (int e = ddc_args(ctx, nr_inputs, nr_out, d_samples, samples_bytes, in_stride, d_digits, digits_bytes, nr_taps, nr_bands, bands,
                         d_out, out_bytes, out_stride))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::ddc, nr_inputs, nr_out, d_samples, samples_bytes, in_stride, d_digits, digits_bytes, nr_taps,
                   nr_bands, bands, first_output, d_out, out_bytes, out_stride, stream);
}

} // extern "C"
