// bf_filterbank.cpp -- include/dcs_filterbank.h, the companion library libdcs_filterbank.so.  Host code only: the kernels
// are libdcs_beamformer.so's (bf_filterbank.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_filterbank.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned(const void *p, uintptr_t n) { return !(reinterpret_cast<uintptr_t>(p) & (n - 1u)); }

} // namespace

extern "C" {

int dcs_bf_spectra_sums(dcs_bf_context *ctx, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                        uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream)
{
    if (!ctx || !d_spectra || !d_sums || !aligned(d_spectra, 4u) || !aligned(d_sums, 8u) || nr_beams == 0u)
        return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->spectra_sums(ctx, d_spectra, spectra_bytes, nr_spectra, nr_beams, accumulate, d_sums, sums_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_filterbank_scales(dcs_bf_context *ctx, const double *d_sums, size_t sums_bytes, uint64_t count, uint32_t nr_beams,
                             float target_std, float *d_scales, size_t scales_bytes, void *stream)
{
    if (!ctx || !d_sums || !d_scales || !aligned(d_sums, 8u) || !aligned(d_scales, 8u) || nr_beams == 0u) return DCS_ERR_INVALID_ARGUMENT;
    if (count == 0u || count >= (1ull << 53)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->filterbank_scales(ctx, d_sums, sums_bytes, count, nr_beams, target_std, d_scales, scales_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_filterbank_q8(dcs_bf_context *ctx, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                         const float *d_scales, float level, uint32_t flags, uint8_t *d_filterbank, size_t filterbank_bytes,
                         uint64_t out_spectra, uint64_t first_spectrum, unsigned long long *d_clip_count, void *stream)
{
    if (!ctx || !d_spectra || !d_scales || !d_filterbank) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_spectra, 4u) || !aligned(d_scales, 8u) || !aligned(d_filterbank, 16u) || !aligned(d_clip_count, 8u))
        return DCS_ERR_INVALID_ARGUMENT;
    if (nr_beams == 0u || (flags & ~(uint32_t)DCS_FB_DESCENDING)) return DCS_ERR_INVALID_ARGUMENT;
    if (first_spectrum > out_spectra || nr_spectra > out_spectra - first_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->filterbank_q8(ctx, d_spectra, spectra_bytes, nr_spectra, nr_beams, d_scales, level, flags, d_filterbank,
                                    filterbank_bytes, out_spectra, first_spectrum, d_clip_count, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
