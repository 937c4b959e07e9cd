// bf_dedisperse.cpp -- include/dcs_dedisperse.h, the companion library libdcs_dedisperse.so.  Host code only: the kernels
// are libdcs_beamformer.so's (bf_dedisperse.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_dedisperse.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_dm_delays(dcs_bf_context *ctx, const dcs_bf_band *band, const double *d_dms, uint32_t nr_dm, int32_t *d_delays,
                     size_t delays_bytes, void *stream)
{
    if (int e = dm_delays_args(ctx, band, d_dms, d_delays)) return e;
    return forward(ctx, &bf_ctx_ext_ops::dm_delays, band, d_dms, nr_dm, d_delays, delays_bytes, stream);
}

int dcs_bf_dedisperse_q8(dcs_bf_context *ctx, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                         uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays,
                         uint32_t nr_dm, uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t *d_dm_time,
                         size_t dm_time_bytes, uint64_t out_spectra, uint64_t first_out, void *stream)
{
    if (int e = dedisperse_q8_args(ctx, d_filterbank, in_spectra, first_spectrum, nr_spectra, nr_beams, d_delays, max_delay, d_dm_time,
                                   out_spectra, first_out))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::dedisperse_q8, d_filterbank, filterbank_bytes, in_spectra, first_spectrum, nr_spectra, nr_beams,
                   d_delays, nr_dm, max_delay, d_channel_mask, d_dm_time, dm_time_bytes, out_spectra, first_out, stream);
}

} // extern "C"
