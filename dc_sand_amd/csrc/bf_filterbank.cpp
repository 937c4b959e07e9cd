// bf_filterbank.cpp -- include/dcs_filterbank.h, the companion library libdcs_filterbank.so.  Host code only: the kernels
// are libdcs_beamformer.so's (bf_filterbank.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_filterbank.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_spectra_sums(dcs_bf_context *ctx, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                        uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream)
{
    if (int e = spectra_sums_args(ctx, d_spectra, nr_beams, d_sums)) return e;
    return forward(ctx, &bf_ctx_ext_ops::spectra_sums, d_spectra, spectra_bytes, nr_spectra, nr_beams, accumulate, d_sums, sums_bytes,
                   stream);
}

int dcs_bf_filterbank_scales(dcs_bf_context *ctx, const double *d_sums, size_t sums_bytes, uint64_t count, uint32_t nr_beams,
                             float target_std, float *d_scales, size_t scales_bytes, void *stream)
{
    if (int e = filterbank_scales_args(ctx, d_sums, count, nr_beams, d_scales)) return e;
    return forward(ctx, &bf_ctx_ext_ops::filterbank_scales, d_sums, sums_bytes, count, nr_beams, target_std, d_scales, scales_bytes,
                   stream);
}

int dcs_bf_filterbank_q8(dcs_bf_context *ctx, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                         const float *d_scales, float level, uint32_t flags, uint8_t *d_filterbank, size_t filterbank_bytes,
                         uint64_t out_spectra, uint64_t first_spectrum, unsigned long long *d_clip_count, void *stream)
{
    if (int e = filterbank_q8_args(ctx, d_spectra, nr_spectra, nr_beams, d_scales, flags, d_filterbank, out_spectra, first_spectrum,
                                   d_clip_count))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::filterbank_q8, d_spectra, spectra_bytes, nr_spectra, nr_beams, d_scales, level, flags,
                   d_filterbank, filterbank_bytes, out_spectra, first_spectrum, d_clip_count, stream);
}

} // extern "C"
