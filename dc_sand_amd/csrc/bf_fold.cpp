// bf_fold.cpp -- include/dcs_fold.h, the companion library libdcs_fold.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_fold.hip), reached through the table at the head of every context it makes (bf_ctx_ext.h).  Each
// export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_fold.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_fold_q8(dcs_bf_context *ctx, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                   uint64_t first_spectrum, uint32_t subint_len, uint32_t nr_subints, uint32_t nr_beams,
                   uint32_t beams_per_model, const dcs_bf_fold_model *d_models, size_t models_bytes, const int32_t *d_delays,
                   size_t delays_bytes, uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t nbin, uint32_t *d_profiles,
                   size_t profiles_bytes, uint32_t *d_hits, size_t hits_bytes, uint64_t out_subints, uint64_t first_subint,
                   uint32_t accumulate, void *stream)
{
    if (int e = fold_q8_args(ctx, d_filterbank, in_spectra, first_spectrum, subint_len, nr_subints, nr_beams, beams_per_model, d_models,
                             d_delays, max_delay, nbin, d_profiles, d_hits, out_subints, first_subint, accumulate))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::fold_q8, d_filterbank, filterbank_bytes, in_spectra, first_spectrum, subint_len, nr_subints,
                   nr_beams, beams_per_model, d_models, models_bytes, d_delays, delays_bytes, max_delay, d_channel_mask, nbin, d_profiles,
                   profiles_bytes, d_hits, hits_bytes, out_subints, first_subint, accumulate, stream);
}

int dcs_bf_fold_scrunch(dcs_bf_context *ctx, const uint32_t *d_profiles, size_t profiles_bytes, uint32_t nr_beams,
                        uint64_t out_subints, uint64_t first_subint, uint32_t nr_subints, uint32_t nbin, uint64_t *d_scrunched,
                        size_t scrunched_bytes, uint32_t accumulate, void *stream)
{
    if (int e = fold_scrunch_args(ctx, d_profiles, nr_beams, out_subints, first_subint, nr_subints, nbin, d_scrunched, accumulate)) return e;
    return forward(ctx, &bf_ctx_ext_ops::fold_scrunch, d_profiles, profiles_bytes, nr_beams, out_subints, first_subint, nr_subints, nbin,
                   d_scrunched, scrunched_bytes, accumulate, stream);
}

} // extern "C"
