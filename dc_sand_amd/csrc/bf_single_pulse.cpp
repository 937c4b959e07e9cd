// bf_single_pulse.cpp -- include/dcs_single_pulse.h, the companion library libdcs_single_pulse.so.  Host code only: the
// kernels are libdcs_beamformer.so's (bf_single_pulse.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_single_pulse.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned(const void *p, uintptr_t n) { return !(reinterpret_cast<uintptr_t>(p) & (n - 1u)); }

// first + n <= total, without a sum that could wrap
bool fits(uint64_t first, uint64_t n, uint64_t total) { return first <= total && n <= total - first; }

} // namespace

extern "C" {

int dcs_bf_dm_time_sums(dcs_bf_context *ctx, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, uint32_t accumulate,
                        uint64_t *d_sums, size_t sums_bytes, void *stream)
{
    if (!ctx || !d_dm_time || !d_sums || !aligned(d_dm_time, 4u) || !aligned(d_sums, 8u)) return DCS_ERR_INVALID_ARGUMENT;
    if (nr_beams == 0u || !fits(first_spectrum, nr_spectra, plane_spectra)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->dm_time_sums(ctx, d_dm_time, dm_time_bytes, plane_spectra, first_spectrum, nr_spectra, nr_beams, nr_dm,
                                   accumulate, d_sums, sums_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_boxcar_peaks(dcs_bf_context *ctx, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths,
                        uint32_t nr_widths, uint32_t max_width, uint32_t block_len, uint32_t *d_peaks, size_t peaks_bytes,
                        uint64_t peak_blocks, uint64_t first_block, void *stream)
{
    if (!ctx || !d_dm_time || !d_widths || !d_peaks) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_dm_time, 4u) || !aligned(d_widths, 4u) || !aligned(d_peaks, 8u)) return DCS_ERR_INVALID_ARGUMENT;
    if (nr_beams == 0u || max_width < 1u || max_width > 4096u) return DCS_ERR_INVALID_ARGUMENT;
    if (block_len < 64u || block_len > 4096u || block_len % 64u) return DCS_ERR_INVALID_ARGUMENT;
    const uint64_t window = (uint64_t)nr_spectra + (max_width - 1u); // < 2^33
    if (!fits(first_spectrum, window, plane_spectra)) return DCS_ERR_INVALID_ARGUMENT;
    const uint64_t nr_blocks = ((uint64_t)nr_spectra + block_len - 1u) / block_len;
    if (!fits(first_block, nr_blocks, peak_blocks)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->boxcar_peaks(ctx, d_dm_time, dm_time_bytes, plane_spectra, first_spectrum, nr_spectra, nr_beams, nr_dm, d_widths,
                                   nr_widths, max_width, block_len, d_peaks, peaks_bytes, peak_blocks, first_block, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_peak_snr(dcs_bf_context *ctx, const uint32_t *d_peaks, size_t peaks_bytes, uint64_t peak_blocks, uint64_t first_block,
                    uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths, uint32_t nr_widths,
                    uint32_t max_width, const uint64_t *d_sums, size_t sums_bytes, uint64_t count, float *d_snr, size_t snr_bytes,
                    uint32_t *d_best, size_t best_bytes, void *stream)
{
    if (!ctx || !d_peaks || !d_widths || !d_sums || !d_snr) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_peaks, 8u) || !aligned(d_widths, 4u) || !aligned(d_sums, 8u) || !aligned(d_snr, 4u) || !aligned(d_best, 4u))
        return DCS_ERR_INVALID_ARGUMENT;
    if (nr_beams == 0u || max_width < 1u || max_width > 4096u) return DCS_ERR_INVALID_ARGUMENT;
    if (!fits(first_block, nr_blocks, peak_blocks) || count == 0u) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->peak_snr(ctx, d_peaks, peaks_bytes, peak_blocks, first_block, nr_blocks, nr_beams, nr_dm, d_widths, nr_widths,
                               max_width, d_sums, sums_bytes, count, d_snr, snr_bytes, d_best, best_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
