// bf_rfi.cpp -- include/dcs_rfi.h, the companion library libdcs_rfi.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_rfi.hip), reached through the table at the head of every context it makes (bf_ctx_ext.h).
// Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_rfi.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_rfi_moments(dcs_bf_context *ctx, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                       uint64_t first_spectrum, uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams,
                       uint32_t *d_cell_sums, size_t cell_sums_bytes, uint32_t *d_zero_dm, size_t zero_dm_bytes, void *stream)
{
    if (int e = rfi_moments_args(ctx, d_filterbank, in_spectra, first_spectrum, nr_blocks, block_len, nr_beams, d_cell_sums, d_zero_dm,
                                 zero_dm_bytes))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::rfi_moments, d_filterbank, filterbank_bytes, in_spectra, first_spectrum, nr_blocks, block_len,
                   nr_beams, d_cell_sums, cell_sums_bytes, d_zero_dm, zero_dm_bytes, stream);
}

int dcs_bf_rfi_flags(dcs_bf_context *ctx, const uint32_t *d_cell_sums, size_t cell_sums_bytes, const uint32_t *d_zero_dm,
                     size_t zero_dm_bytes, uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams,
                     const dcs_bf_rfi_thresholds *thr, uint8_t *d_cell_flags, size_t cell_flags_bytes, uint8_t *d_channel_mask,
                     size_t channel_mask_bytes, uint8_t *d_spectrum_flags, size_t spectrum_flags_bytes, uint32_t *d_counts,
                     size_t counts_bytes, void *stream)
{
    if (int e = rfi_flags_args(ctx, d_cell_sums, d_zero_dm, zero_dm_bytes, nr_blocks, block_len, nr_beams, thr, d_cell_flags,
                               d_channel_mask, d_spectrum_flags, spectrum_flags_bytes, d_counts, counts_bytes))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::rfi_flags, d_cell_sums, cell_sums_bytes, d_zero_dm, zero_dm_bytes, nr_blocks, block_len,
                   nr_beams, thr, d_cell_flags, cell_flags_bytes, d_channel_mask, channel_mask_bytes, d_spectrum_flags,
                   spectrum_flags_bytes, d_counts, counts_bytes, stream);
}

int dcs_bf_rfi_clean_q8(dcs_bf_context *ctx, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                        uint64_t first_spectrum, uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams,
                        const uint8_t *d_cell_flags, const uint8_t *d_channel_mask, const uint8_t *d_spectrum_flags, uint8_t fill,
                        uint8_t *d_out, size_t out_bytes, uint64_t out_spectra, uint64_t first_out, unsigned long long *d_replaced,
                        void *stream)
{
    if (int e = rfi_clean_q8_args(ctx, d_filterbank, in_spectra, first_spectrum, nr_blocks, block_len, nr_beams, d_out, out_spectra,
                                  first_out, d_replaced))
        return e;
    return forward(ctx, &bf_ctx_ext_ops::rfi_clean_q8, d_filterbank, filterbank_bytes, in_spectra, first_spectrum, nr_blocks, block_len,
                   nr_beams, d_cell_flags, d_channel_mask, d_spectrum_flags, fill, d_out, out_bytes, out_spectra, first_out, d_replaced,
                   stream);
}

} // extern "C"
