// bf_dedisperse.cpp -- include/dcs_dedisperse.h, the companion library libdcs_dedisperse.so.  Host code only: the kernels
// are libdcs_beamformer.so's (bf_dedisperse.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_dedisperse.h"

#include <cmath>

#include "bf_ctx_ext.h"

namespace {

bool aligned(const void *p, uintptr_t n) { return !(reinterpret_cast<uintptr_t>(p) & (n - 1u)); }

} // namespace

extern "C" {

int dcs_bf_dm_delays(dcs_bf_context *ctx, const dcs_bf_band *band, const double *d_dms, uint32_t nr_dm, int32_t *d_delays,
                     size_t delays_bytes, void *stream)
{
    if (!ctx || !band || !d_dms || !d_delays || !aligned(d_dms, 8u) || !aligned(d_delays, 4u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(band->freq_first_mhz) || !std::isfinite(band->freq_step_mhz) || !std::isfinite(band->sample_time_s))
        return DCS_ERR_INVALID_ARGUMENT;
    if (!(band->sample_time_s > 0.0) || !(band->freq_first_mhz > 0.0)) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->dm_delays(ctx, band, d_dms, nr_dm, d_delays, delays_bytes, stream) : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_dedisperse_q8(dcs_bf_context *ctx, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                         uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays,
                         uint32_t nr_dm, uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t *d_dm_time,
                         size_t dm_time_bytes, uint64_t out_spectra, uint64_t first_out, void *stream)
{
    if (!ctx || !d_filterbank || !d_delays || !d_dm_time) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_filterbank, 16u) || !aligned(d_delays, 4u) || !aligned(d_dm_time, 4u)) return DCS_ERR_INVALID_ARGUMENT;
    if (nr_beams == 0u || max_delay > 0x7ffffffeu) return DCS_ERR_INVALID_ARGUMENT;
    const uint64_t window = (uint64_t)nr_spectra + max_delay; // < 2^33
    if (first_spectrum > in_spectra || window > in_spectra - first_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    if (first_out > out_spectra || nr_spectra > out_spectra - first_out) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->dedisperse_q8(ctx, d_filterbank, filterbank_bytes, in_spectra, first_spectrum, nr_spectra, nr_beams, d_delays,
                                    nr_dm, max_delay, d_channel_mask, d_dm_time, dm_time_bytes, out_spectra, first_out, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
