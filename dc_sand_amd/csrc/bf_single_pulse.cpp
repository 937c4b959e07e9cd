// bf_single_pulse.cpp -- include/dcs_single_pulse.h, the companion library libdcs_single_pulse.so.  Host code only: the
// kernels are libdcs_beamformer.so's (bf_single_pulse.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_single_pulse.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_dm_time_sums(dcs_bf_context *ctx, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, uint32_t accumulate,
                        uint64_t *d_sums, size_t sums_bytes, void *stream)
{
    if (int e = dm_time_sums_args(ctx, d_dm_time, plane_spectra, first_spectrum, nr_spectra, nr_beams, d_sums)) return e;
    return forward(ctx, &bf_ctx_ext_ops::dm_time_sums, d_dm_time, dm_time_bytes, plane_spectra, first_spectrum, nr_spectra, nr_beams,
                   nr_dm, accumulate, d_sums, sums_bytes, stream);
}

int dcs_bf_boxcar_peaks(dcs_bf_context *ctx, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths,
                        uint32_t nr_widths, uint32_t max_width, uint32_t block_len, uint32_t *d_peaks, size_t peaks_bytes,
                        uint64_t peak_blocks, uint64_t first_block, void *stream)
{
    if (int e = boxcar_peaks_args(ctx, d_dm_time, plane_spectra, first_spectrum, nr_spectra, nr_beams, d_widths, max_width, block_len,
                                  d_peaks, peak_blocks, first_block))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::boxcar_peaks, d_dm_time, dm_time_bytes, plane_spectra, first_spectrum, nr_spectra, nr_beams,
                   nr_dm, d_widths, nr_widths, max_width, block_len, d_peaks, peaks_bytes, peak_blocks, first_block, stream);
}

int dcs_bf_peak_snr(dcs_bf_context *ctx, const uint32_t *d_peaks, size_t peaks_bytes, uint64_t peak_blocks, uint64_t first_block,
                    uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths, uint32_t nr_widths,
                    uint32_t max_width, const uint64_t *d_sums, size_t sums_bytes, uint64_t count, float *d_snr, size_t snr_bytes,
                    uint32_t *d_best, size_t best_bytes, void *stream)
{
    if (int e = peak_snr_args(ctx, d_peaks, peak_blocks, first_block, nr_blocks, nr_beams, d_widths, max_width, d_sums, count, d_snr,
                              d_best))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::peak_snr, d_peaks, peaks_bytes, peak_blocks, first_block, nr_blocks, nr_beams, nr_dm, d_widths,
                   nr_widths, max_width, d_sums, sums_bytes, count, d_snr, snr_bytes, d_best, best_bytes, stream);
}

} // extern "C"
