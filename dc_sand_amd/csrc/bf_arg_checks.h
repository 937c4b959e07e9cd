// bf_arg_checks.h -- the checks a call behind bf_ctx_ext_ops can make without a device, each stated once: one function per
// table entry, named after it, called by the companion's export before it reads the table and again as the first statement
// of the *_impl behind the table.  What a function refuses is what a handle that is no context of this build gets
// DCS_ERR_INVALID_ARGUMENT for instead of DCS_ERR_UNSUPPORTED (tests/test_host_abi_*.py); a check that needs the context's
// sizes or its device is the _impl's own.  Host code, header-only, no HIP.  Not a public interface.
#ifndef BF_ARG_CHECKS_H
#define BF_ARG_CHECKS_H

#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "../../include/dcs_beam_complex.h" // DCS_BF_COMPLEX_CONJ
#include "../../include/dcs_beamformer.h"
#include "../../include/dcs_ddc.h"        // dcs_ddc_band
#include "../../include/dcs_dedisperse.h" // dcs_bf_band
#include "../../include/dcs_filterbank.h" // DCS_FB_DESCENDING
#include "../../include/dcs_fold.h"       // dcs_bf_fold_model
#include "../../include/dcs_rfi.h"        // dcs_bf_rfi_thresholds
#include "../../include/dcs_stokes.h"     // DCS_BF_STOKES_I, DCS_BF_STOKES_IQUV

// p is a multiple of bytes, a power of two; a null pointer passes (an optional tensor's alignment is checked the same way)
inline bool aligned(const void *p, uintptr_t bytes) { return !(reinterpret_cast<uintptr_t>(p) & (bytes - 1u)); }

// first + n <= total, without a sum that could wrap
inline bool fits(uint64_t first, uint64_t n, uint64_t total) { return first <= total && n <= total - first; }

// have >= x * y * z * w, the product taken without overflow
inline bool holds(size_t have, uint64_t x, uint64_t y, uint64_t z, uint64_t w)
{
    const unsigned __int128 xy = (unsigned __int128)x * y, zw = (unsigned __int128)z * w;
    if ((xy >> 64) || (zw >> 64)) return xy == 0 || zw == 0;
    const unsigned __int128 need = xy * zw;
    return !(need >> 64) && (uint64_t)need <= (uint64_t)have;
}

inline int arg_status(bool ok) { return ok ? DCS_OK : DCS_ERR_INVALID_ARGUMENT; }
inline bool stokes_ok(uint32_t nr_stokes) { return nr_stokes == DCS_BF_STOKES_I || nr_stokes == DCS_BF_STOKES_IQUV; }
inline bool complex_flags_ok(uint32_t flags) { return !(flags & ~(uint32_t)DCS_BF_COMPLEX_CONJ); }
inline bool width_ok(uint32_t max_width) { return max_width >= 1u && max_width <= 4096u; }

// what the three integrations share: both tensors, aligned to their elements of bytes, and whole spectra of blocks
inline int integration_args(dcs_bf_context *c, const void *d_blocks, const void *d_spectra, uintptr_t bytes, uint32_t nr_blocks,
                            uint32_t blocks_per_spectrum)
{
    return arg_status(c && d_blocks && d_spectra && aligned(d_blocks, bytes) && aligned(d_spectra, bytes) && blocks_per_spectrum != 0u &&
                      nr_blocks % blocks_per_spectrum == 0u);
}

// include/dcs_beam_weights.h.  dt: nullptr for the times of the samples from t0 on, which begins a 16-sample block
inline int beamform_accumulated_weighted_args(dcs_bf_context *c, uint32_t nt, const float *d_weights)
{
    return arg_status(c && d_weights && aligned(d_weights, 4u) && nt % 16u == 0u);
}
inline int generate_and_beamform_weighted_args(dcs_bf_context *c, const float *dt, uint64_t t0, uint32_t nt, const float *d_weights)
{
    return arg_status(!beamform_accumulated_weighted_args(c, nt, d_weights) && (dt || t0 % 16u == 0u));
}

// include/dcs_beam_quant.h
inline int beamform_accumulated_q8_args(dcs_bf_context *c, uint32_t nt, const float *d_weights, const float *d_quant_gains,
                                        const unsigned long long *d_clip_count)
{
    return arg_status(c && d_quant_gains && aligned(d_quant_gains, 4u) && aligned(d_weights, 4u) && aligned(d_clip_count, 8u) &&
                      nt % 16u == 0u);
}

// include/dcs_beam_power.h and include/dcs_incoherent_beam.h: block powers out, one dword each
inline int beamform_accumulated_power_args(dcs_bf_context *c, uint32_t nt, const float *d_weights, const void *d_block_power)
{
    return arg_status(c && d_block_power && aligned(d_block_power, 4u) && aligned(d_weights, 4u) && nt % 16u == 0u);
}
inline int integrate_block_power_args(dcs_bf_context *c, const float *d_block_power, uint32_t nr_blocks, uint32_t blocks_per_spectrum,
                                      const float *d_spectra)
{
    return integration_args(c, d_block_power, d_spectra, 4u, nr_blocks, blocks_per_spectrum);
}
inline int incoherent_block_power_args(dcs_bf_context *c, uint32_t nt, const float *d_weights, const uint32_t *d_block_power)
{
    return beamform_accumulated_power_args(c, nt, d_weights, d_block_power);
}
inline int integrate_incoherent_power_args(dcs_bf_context *c, const uint32_t *d_block_power, uint32_t nr_blocks,
                                           uint32_t blocks_per_spectrum, const float *d_spectra)
{
    return integration_args(c, d_block_power, d_spectra, 4u, nr_blocks, blocks_per_spectrum);
}

// include/dcs_filterbank.h
inline int spectra_sums_args(dcs_bf_context *c, const float *d_spectra, uint32_t nr_beams, const double *d_sums)
{
    return arg_status(c && d_spectra && d_sums && aligned(d_spectra, 4u) && aligned(d_sums, 8u) && nr_beams != 0u);
}
inline int filterbank_scales_args(dcs_bf_context *c, const double *d_sums, uint64_t count, uint32_t nr_beams, const float *d_scales)
{
    return arg_status(c && d_sums && d_scales && aligned(d_sums, 8u) && aligned(d_scales, 8u) && nr_beams != 0u && count != 0u &&
                      count < (1ull << 53));
}
inline int filterbank_q8_args(dcs_bf_context *c, const float *d_spectra, uint32_t nr_spectra, uint32_t nr_beams, const float *d_scales,
                              uint32_t flags, const uint8_t *d_filterbank, uint64_t out_spectra, uint64_t first_spectrum,
                              const unsigned long long *d_clip_count)
{
    return arg_status(c && d_spectra && d_scales && d_filterbank && aligned(d_spectra, 4u) && aligned(d_scales, 8u) &&
                      aligned(d_filterbank, 16u) && aligned(d_clip_count, 8u) && nr_beams != 0u &&
                      !(flags & ~(uint32_t)DCS_FB_DESCENDING) && fits(first_spectrum, nr_spectra, out_spectra));
}

// include/dcs_beam_complex.h (d_beams: (re, im) fp32 pairs; d_block_power: single floats) and include/dcs_beam_complex_quant.h
inline int beamform_accumulated_complex_args(dcs_bf_context *c, uint32_t nt, const float *d_weights, uint32_t flags, const float *d_beams)
{
    return arg_status(c && d_beams && aligned(d_beams, 8u) && aligned(d_weights, 4u) && nt % 16u == 0u && complex_flags_ok(flags));
}
inline int beamform_accumulated_complex_power_args(dcs_bf_context *c, uint32_t nt, const float *d_weights, uint32_t flags,
                                                   const float *d_block_power)
{
    return arg_status(!beamform_accumulated_power_args(c, nt, d_weights, d_block_power) && complex_flags_ok(flags));
}
inline int beamform_accumulated_complex_q8_args(dcs_bf_context *c, uint32_t nt, const float *d_weights, uint32_t flags,
                                                const float *d_quant_gains, const int8_t *d_beams_q8,
                                                const unsigned long long *d_clip_count)
{
    return arg_status(!beamform_accumulated_q8_args(c, nt, d_weights, d_quant_gains, d_clip_count) && d_beams_q8 &&
                      aligned(d_beams_q8, 8u) && complex_flags_ok(flags));
}

// include/dcs_stokes.h: a block's nr_stokes values are stored as one word or one quad
inline int stokes_block_args(dcs_bf_context *c, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, uint32_t nr_stokes,
                             const int32_t *d_block_stokes)
{
    return arg_status(c && d_beams_x && d_beams_y && d_block_stokes && stokes_ok(nr_stokes) && aligned(d_beams_x, 16u) &&
                      aligned(d_beams_y, 16u) && aligned(d_block_stokes, 4u * nr_stokes) && nt % 16u == 0u);
}
inline int integrate_stokes_args(dcs_bf_context *c, const int32_t *d_block_stokes, uint32_t nr_blocks, uint32_t blocks_per_spectrum,
                                 uint32_t nr_stokes, const float *d_spectra)
{
    return arg_status(stokes_ok(nr_stokes) &&
                      !integration_args(c, d_block_stokes, d_spectra, 4u * nr_stokes, nr_blocks, blocks_per_spectrum));
}

// include/dcs_dedisperse.h.  The band's last frequency needs the context's channel count: dm_delays_impl checks it
inline int dm_delays_args(dcs_bf_context *c, const dcs_bf_band *band, const double *d_dms, const int32_t *d_delays)
{
    return arg_status(c && band && d_dms && d_delays && aligned(d_dms, 8u) && aligned(d_delays, 4u) &&
                      std::isfinite(band->freq_first_mhz) && std::isfinite(band->freq_step_mhz) && std::isfinite(band->sample_time_s) &&
                      band->sample_time_s > 0.0 && band->freq_first_mhz > 0.0);
}
inline int dedisperse_q8_args(dcs_bf_context *c, const uint8_t *d_filterbank, uint64_t in_spectra, uint64_t first_spectrum,
                              uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays, uint32_t max_delay,
                              const uint32_t *d_dm_time, uint64_t out_spectra, uint64_t first_out)
{
    return arg_status(c && d_filterbank && d_delays && d_dm_time && aligned(d_filterbank, 16u) && aligned(d_delays, 4u) &&
                      aligned(d_dm_time, 4u) && nr_beams != 0u && max_delay <= 0x7ffffffeu &&
                      fits(first_spectrum, (uint64_t)nr_spectra + max_delay, in_spectra) && fits(first_out, nr_spectra, out_spectra));
}

// include/dcs_single_pulse.h.  A boxcar of max_width spectra reads max_width - 1 past the last one it starts at; a peak block
// is block_len starts
inline int dm_time_sums_args(dcs_bf_context *c, const uint32_t *d_dm_time, uint64_t plane_spectra, uint64_t first_spectrum,
                             uint32_t nr_spectra, uint32_t nr_beams, const uint64_t *d_sums)
{
    return arg_status(c && d_dm_time && d_sums && aligned(d_dm_time, 4u) && aligned(d_sums, 8u) && nr_beams != 0u &&
                      fits(first_spectrum, nr_spectra, plane_spectra));
}
inline int boxcar_peaks_args(dcs_bf_context *c, const uint32_t *d_dm_time, uint64_t plane_spectra, uint64_t first_spectrum,
                             uint32_t nr_spectra, uint32_t nr_beams, const uint32_t *d_widths, uint32_t max_width, uint32_t block_len,
                             const uint32_t *d_peaks, uint64_t peak_blocks, uint64_t first_block)
{
    if (!c || !d_dm_time || !d_widths || !d_peaks || !aligned(d_dm_time, 4u) || !aligned(d_widths, 4u) || !aligned(d_peaks, 8u) ||
        nr_beams == 0u || !width_ok(max_width) || block_len < 64u || block_len > 4096u || block_len % 64u)
        return DCS_ERR_INVALID_ARGUMENT;
    const uint64_t nr_blocks = ((uint64_t)nr_spectra + block_len - 1u) / block_len;
    return arg_status(fits(first_spectrum, (uint64_t)nr_spectra + (max_width - 1u), plane_spectra) &&
                      fits(first_block, nr_blocks, peak_blocks));
}
inline int peak_snr_args(dcs_bf_context *c, const uint32_t *d_peaks, uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks,
                         uint32_t nr_beams, const uint32_t *d_widths, uint32_t max_width, const uint64_t *d_sums, uint64_t count,
                         const float *d_snr, const uint32_t *d_best)
{
    return arg_status(c && d_peaks && d_widths && d_sums && d_snr && aligned(d_peaks, 8u) && aligned(d_widths, 4u) &&
                      aligned(d_sums, 8u) && aligned(d_snr, 4u) && aligned(d_best, 4u) && nr_beams != 0u && width_ok(max_width) &&
                      fits(first_block, nr_blocks, peak_blocks) && count != 0u);
}

// include/dcs_correlator.h: a visibility is blocks_per_vis whole blocks, few enough that no sum leaves int32; a baseline's
// (re, im) is stored as one pair of words
inline int correlate_block_args(dcs_bf_context *c, uint32_t nt, uint32_t blocks_per_vis, const int32_t *d_vis)
{
    return arg_status(c && d_vis && aligned(d_vis, 8u) && nt % 16u == 0u && blocks_per_vis != 0u && blocks_per_vis <= 4095u &&
                      (nt / 16u) % blocks_per_vis == 0u);
}
inline int integrate_visibilities_args(dcs_bf_context *c, const int32_t *d_vis, uint32_t nr_vis, uint32_t vis_per_integration,
                                       const float *d_out)
{
    return arg_status(c && d_vis && d_out && aligned(d_vis, 8u) && aligned(d_out, 4u) && vis_per_integration != 0u &&
                      nr_vis % vis_per_integration == 0u);
}

// include/dcs_ddc.h: T taps in whole K steps of 64, one or two bands, the operand table of 16 T bytes
inline bool ddc_shape_ok(uint32_t nr_taps, uint32_t nr_bands)
{
    return nr_taps % 64u == 0u && nr_taps >= 64u && nr_taps <= 256u && (nr_bands == 1u || nr_bands == 2u);
}
inline int ddc_tap_digits_args(dcs_bf_context *c, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, const void *d_digits,
                               size_t digits_bytes)
{
    return arg_status(c && d_taps && d_digits && aligned(d_taps, 4u) && aligned(d_digits, 16u) && ddc_shape_ok(nr_taps, nr_bands) &&
                      holds(digits_bytes, 16u, nr_taps, 1u, 1u));
}
// a row is read from its sample 0 to 16 (nr_out - 1) + T - 1 and written from its pair 0 to nr_out - 1: the last row of either
// tensor need not be a whole stride
inline int ddc_args(dcs_bf_context *c, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes,
                    uint64_t in_stride, const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands,
                    const dcs_ddc_band *bands, const float *d_out, size_t out_bytes, uint64_t out_stride)
{
    if (!(c && d_digits && bands && d_out && aligned(d_samples, 16u) && aligned(d_digits, 16u) && aligned(d_out, 8u) &&
          ddc_shape_ok(nr_taps, nr_bands) && holds(digits_bytes, 16u, nr_taps, 1u, 1u) && in_stride % 16u == 0u && out_stride >= nr_out))
        return DCS_ERR_INVALID_ARGUMENT;
    if (nr_out == 0u || nr_inputs == 0u) return DCS_OK;
    const uint64_t row = 16u * ((uint64_t)nr_out - 1u) + nr_taps;
    const unsigned __int128 need = (unsigned __int128)(nr_inputs - 1u) * in_stride + row;
    const unsigned __int128 pairs = (unsigned __int128)((uint64_t)nr_bands * nr_inputs - 1u) * out_stride + nr_out; // < 2^98
    return arg_status(d_samples && in_stride >= row && !(need >> 64) && (uint64_t)need <= (uint64_t)samples_bytes &&
                      !(pairs >> 61) && (uint64_t)pairs * (2u * sizeof(float)) <= (uint64_t)out_bytes);
}

// include/dcs_candidates.h.  The sifter's tiles are kCandTileDms DMs by kCandTileBlocks blocks (bf_candidates.hip); a segment
// is one row of a tile, the 64 cells whose marks are one ballot.  The workspace holds per segment one 64-bit word of marks,
// then one 32-bit count that the scan turns into the segment's place in the list, both in the order (beam, DM, tile of blocks)
constexpr uint32_t kCandTileDms = 16u, kCandTileBlocks = 64u, kCandMaxRadius = 8u;
inline unsigned __int128 candidates_segments(uint32_t nr_beams, uint32_t nr_dm, uint32_t nr_blocks)
{
    return (unsigned __int128)nr_beams * nr_dm * (((uint64_t)nr_blocks + kCandTileBlocks - 1u) / kCandTileBlocks);
}
inline size_t candidates_workspace_bytes(uint32_t nr_beams, uint32_t nr_dm, uint32_t nr_blocks)
{
    const unsigned __int128 segments = candidates_segments(nr_beams, nr_dm, nr_blocks); // < 2^90
    const unsigned __int128 bytes = segments * 8u + (segments * 4u + 7u) / 8u * 8u;
    return bytes > (unsigned __int128)SIZE_MAX ? SIZE_MAX : (size_t)bytes;
}
inline int find_candidates_args(dcs_bf_context *c, const float *d_snr, const uint32_t *d_peaks, uint64_t peak_blocks, uint64_t first_block,
                                uint32_t nr_blocks, uint32_t nr_beams, float threshold, uint32_t dm_radius, uint32_t block_radius,
                                const void *d_cands, uint32_t max_candidates, const uint32_t *d_count, const void *d_work)
{
    return arg_status(c && d_snr && d_peaks && d_count && d_work && (d_cands || max_candidates == 0u) && aligned(d_snr, 4u) &&
                      aligned(d_peaks, 8u) && aligned(d_cands, 8u) && aligned(d_count, 4u) && aligned(d_work, 8u) && nr_beams != 0u &&
                      dm_radius <= kCandMaxRadius && block_radius <= kCandMaxRadius && std::isfinite(threshold) &&
                      fits(first_block, nr_blocks, peak_blocks));
}

// include/dcs_channeliser.h: N a power of two in [64, 2048], 1 .. 16 taps per branch, whole blocks of 16 spectra.  A row is read
// from its pair 0 to (nr_spectra + P - 1) N - 1; the output is the whole tensor [N][out_blocks][out_inputs][16][2] of words of
// elem bytes (4: float, 1: int8), of which the call writes blocks first_block .. and inputs first_input ..
inline int channelise_args(dcs_bf_context *c, uint32_t N, uint32_t P, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                           size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order,
                           const void *d_out, uint32_t elem, size_t out_bytes, uint64_t out_blocks, uint64_t first_block,
                           uint32_t out_inputs, uint32_t first_input)
{
    const bool empty = nr_spectra == 0u || nr_inputs == 0u;
    if (!c || (!empty && !(d_in && d_taps && d_twiddles && d_out))) return DCS_ERR_INVALID_ARGUMENT;
    if (!(aligned(d_in, 8u) && aligned(d_taps, 4u) && aligned(d_twiddles, 8u) && aligned(d_out, 16u))) return DCS_ERR_INVALID_ARGUMENT;
    if (N < 64u || N > 2048u || (N & (N - 1u)) || P < 1u || P > 16u || nr_spectra % 16u != 0u || order > 1u)
        return DCS_ERR_INVALID_ARGUMENT;
    if (empty) return DCS_OK;
    const uint64_t row = ((uint64_t)nr_spectra + P - 1u) * N;                                   // < 2^44
    const unsigned __int128 need = (unsigned __int128)(nr_inputs - 1u) * in_stride + row;      // < 2^97
    return arg_status(in_stride >= row && !(need >> 61) && (uint64_t)need * (2u * sizeof(float)) <= (uint64_t)in_bytes &&
                      fits(first_block, nr_spectra / 16u, out_blocks) && fits(first_input, nr_inputs, out_inputs) &&
                      holds(out_bytes, N, out_blocks, out_inputs, 32u * elem));
}
inline int channelise_q8_args(dcs_bf_context *c, uint32_t N, uint32_t P, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                              size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order,
                              const float *d_gains, const int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks, uint64_t first_block,
                              uint32_t out_inputs, uint32_t first_input, const unsigned long long *d_clip_count)
{
    const bool empty = nr_spectra == 0u || nr_inputs == 0u;
    if (!c || (!empty && !d_gains) || !aligned(d_gains, 4u) || !aligned(d_clip_count, 8u)) return DCS_ERR_INVALID_ARGUMENT;
    return channelise_args(c, N, P, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles, order, d_out_q8, 1u, out_bytes,
                           out_blocks, first_block, out_inputs, first_input);
}

// include/dcs_rfi.h: a window of nr_blocks blocks of 1 .. 65536 spectra, at most 2^32 - 1 spectra in all.  The buffers whose
// sizes need no C are checked here (a product past 64 bits holds in no buffer); those that need it are the _impl's
inline bool rfi_window_ok(uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams)
{
    return nr_beams != 0u && block_len >= 1u && block_len <= 65536u && (uint64_t)nr_blocks * block_len <= 0xffffffffull;
}
inline bool rfi_threshold_ok(double v) { return std::isfinite(v) && v >= 0.0; }
inline int rfi_moments_args(dcs_bf_context *c, const uint8_t *d_filterbank, uint64_t in_spectra, uint64_t first_spectrum,
                            uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const uint32_t *d_cell_sums,
                            const uint32_t *d_zero_dm, size_t zero_dm_bytes)
{
    return arg_status(c && d_filterbank && d_cell_sums && aligned(d_filterbank, 16u) && aligned(d_cell_sums, 8u) &&
                      aligned(d_zero_dm, 4u) && rfi_window_ok(nr_blocks, block_len, nr_beams) &&
                      fits(first_spectrum, (uint64_t)nr_blocks * block_len, in_spectra) &&
                      (!d_zero_dm || holds(zero_dm_bytes, nr_beams, (uint64_t)nr_blocks * block_len, sizeof(uint32_t), 1u)));
}
inline int rfi_flags_args(dcs_bf_context *c, const uint32_t *d_cell_sums, const uint32_t *d_zero_dm, size_t zero_dm_bytes,
                          uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const dcs_bf_rfi_thresholds *thr,
                          const uint8_t *d_cell_flags, const uint8_t *d_channel_mask, const uint8_t *d_spectrum_flags,
                          size_t spectrum_flags_bytes, const uint32_t *d_counts, size_t counts_bytes)
{
    if (!(c && d_cell_sums && thr && d_cell_flags && d_channel_mask && d_counts && aligned(d_cell_sums, 8u) && aligned(d_zero_dm, 4u) &&
          aligned(d_counts, 4u) && rfi_window_ok(nr_blocks, block_len, nr_beams)))
        return DCS_ERR_INVALID_ARGUMENT;
    if (!(rfi_threshold_ok(thr->mean_thr) && rfi_threshold_ok(thr->mean_floor) && rfi_threshold_ok(thr->var_thr) &&
          rfi_threshold_ok(thr->var_floor) && rfi_threshold_ok(thr->zero_dm_thr) && rfi_threshold_ok(thr->zero_dm_floor)))
        return DCS_ERR_INVALID_ARGUMENT;
    const uint64_t window = (uint64_t)nr_blocks * block_len;
    return arg_status(!d_zero_dm == !d_spectrum_flags && holds(counts_bytes, nr_beams, 3u, sizeof(uint32_t), 1u) &&
                      (!d_zero_dm || (holds(zero_dm_bytes, nr_beams, window, sizeof(uint32_t), 1u) &&
                                      holds(spectrum_flags_bytes, nr_beams, window, 1u, 1u))));
}
inline int rfi_clean_q8_args(dcs_bf_context *c, const uint8_t *d_filterbank, uint64_t in_spectra, uint64_t first_spectrum,
                             uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const uint8_t *d_out, uint64_t out_spectra,
                             uint64_t first_out, const unsigned long long *d_replaced)
{
    return arg_status(c && d_filterbank && d_out && aligned(d_filterbank, 16u) && aligned(d_out, 16u) && aligned(d_replaced, 8u) &&
                      rfi_window_ok(nr_blocks, block_len, nr_beams) &&
                      fits(first_spectrum, (uint64_t)nr_blocks * block_len, in_spectra) &&
                      fits(first_out, (uint64_t)nr_blocks * block_len, out_spectra));
}

// include/dcs_fold.h: nr_subints sub-integrations of 1 .. 2^24 spectra (no profile word wraps), 1 .. 1024 phase bins, one model
// row per beams_per_model beams.  The window nr_subints * subint_len + max_delay is below 2^57: no sum wraps before fits().  The
// buffer sizes are the _impl's, with those that need the context's C
inline int fold_q8_args(dcs_bf_context *c, const uint8_t *d_filterbank, uint64_t in_spectra, uint64_t first_spectrum, uint32_t subint_len,
                        uint32_t nr_subints, uint32_t nr_beams, uint32_t beams_per_model, const dcs_bf_fold_model *d_models,
                        const int32_t *d_delays, uint32_t max_delay, uint32_t nbin, const uint32_t *d_profiles, const uint32_t *d_hits,
                        uint64_t out_subints, uint64_t first_subint, uint32_t accumulate)
{
    return arg_status(c && d_filterbank && d_models && d_profiles && aligned(d_filterbank, 16u) && aligned(d_models, 8u) &&
                      aligned(d_delays, 4u) && aligned(d_profiles, 4u) && aligned(d_hits, 4u) && nr_beams != 0u &&
                      beams_per_model != 0u && nr_beams % beams_per_model == 0u && nbin >= 1u && nbin <= 1024u && subint_len >= 1u &&
                      subint_len <= (1u << 24) && max_delay <= 0x7ffffffeu &&
                      fits(first_spectrum, (uint64_t)nr_subints * subint_len + max_delay, in_spectra) &&
                      fits(first_subint, nr_subints, out_subints) && accumulate <= 1u);
}
inline int fold_scrunch_args(dcs_bf_context *c, const uint32_t *d_profiles, uint32_t nr_beams, uint64_t out_subints, uint64_t first_subint,
                             uint32_t nr_subints, uint32_t nbin, const uint64_t *d_scrunched, uint32_t accumulate)
{
    return arg_status(c && d_profiles && d_scrunched && aligned(d_profiles, 4u) && aligned(d_scrunched, 8u) && nr_beams != 0u &&
                      nbin >= 1u && nbin <= 1024u && fits(first_subint, nr_subints, out_subints) && accumulate <= 1u);
}

#endif // BF_ARG_CHECKS_H
