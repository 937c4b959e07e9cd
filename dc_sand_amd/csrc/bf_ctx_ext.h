// bf_ctx_ext.h -- the internal contract between libdcs_beamformer.so and its companions libdcs_beam_weights.so
// (include/dcs_beam_weights.h), libdcs_beam_quant.so (include/dcs_beam_quant.h), libdcs_beam_power.so
// (include/dcs_beam_power.h), libdcs_incoherent_beam.so (include/dcs_incoherent_beam.h), libdcs_filterbank.so
// (include/dcs_filterbank.h), libdcs_beam_complex.so (include/dcs_beam_complex.h), libdcs_beam_complex_quant.so
// (include/dcs_beam_complex_quant.h), libdcs_stokes.so (include/dcs_stokes.h), libdcs_dedisperse.so
// (include/dcs_dedisperse.h), libdcs_single_pulse.so (include/dcs_single_pulse.h), libdcs_correlator.so
// (include/dcs_correlator.h), libdcs_ddc.so (include/dcs_ddc.h), libdcs_candidates.so (include/dcs_candidates.h),
// libdcs_channeliser.so (include/dcs_channeliser.h) and libdcs_rfi.so (include/dcs_rfi.h).  All are built from this tree together.
// Every dcs_bf_context begins with a bf_ctx_ext_head whose table points at the product library's
// implementation of the weighted, the quantised, the detecting and the complex-product beamformer calls, of the incoherent
// beam, of the filterbank calls, of the Stokes detection, of the dedispersion, of the single-pulse search, of the correlator, of the down-converter, of the candidate sifter, of the channeliser and of the RFI flagger; a companion's
// export is two statements: the entry's device-free checks (bf_arg_checks.h, where the implementation behind the table
// takes them from too), then forward(), which checks the table's version and calls the entry.  Not a public interface.
#ifndef BF_CTX_EXT_H
#define BF_CTX_EXT_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/dcs_beamformer.h"
#include "../../include/dcs_dedisperse.h" // dcs_bf_band
#include "bf_arg_checks.h"

// 2: beamform_accumulated_q8 appended; 3: beamform_accumulated_power, integrate_block_power appended; 5: incoherent_block_power,
// integrate_incoherent_power appended.  4 is skipped for good: tests/test_host_abi_beam_power.py hands the power companion a
// zeroed table whose version word is 4 and expects DCS_ERR_UNSUPPORTED -- at version 4 it would call a null pointer.
// 6: spectra_sums, filterbank_scales, filterbank_q8 appended (the tests hand foreign versions 1 to 5 only).
// 7: beamform_accumulated_complex, beamform_accumulated_complex_power appended (tests/test_host_abi_beam_complex.py hands its
// companion the foreign versions 1, 3, 5 and 6).
// 8: beamform_accumulated_complex_q8 appended (tests/test_host_abi_beam_complex_quant.py hands its companion 1, 6 and 7).
// 9: stokes_block, integrate_stokes appended (tests/test_host_abi_stokes.py hands its companion 1, 7 and 8; the older tests
// hand foreign versions 1 to 7 only).
// 10: dm_delays, dedisperse_q8 appended (tests/test_host_abi_dedisperse.py hands its companion 1, 8 and 9; no older test
// hands a foreign version above 8).
// 11: dm_time_sums, boxcar_peaks, peak_snr appended (tests/test_host_abi_single_pulse.py hands its companion 1, 9 and 10; no
// older test hands a foreign version above 9).
// 12: correlate_block, integrate_visibilities appended (tests/test_host_abi_correlator.py hands its companion 1, 10 and 11; no
// older test hands a foreign version above 10).
// 13: ddc_tap_digits, ddc appended (tests/test_host_abi_ddc.py hands its companion 1, 11 and 12; no older test hands a
// foreign version above 11).
// 14: find_candidates appended (tests/test_host_abi_candidates.py hands its companion 1, 12 and 13; no older test hands a
// foreign version above 12).
// 15: channelise, channelise_q8 appended (tests/test_host_abi_channeliser.py hands its companion 1, 13 and 14; no older test
// hands a foreign version above 13).
// 16: rfi_moments, rfi_flags, rfi_clean_q8 appended (tests/test_host_abi_rfi.py hands its companion 1, 14 and 15; no older test
// hands a foreign version above 14).
#define BF_CTX_EXT_VERSION 16u

struct bf_ctx_ext_ops {
    uint32_t version; // BF_CTX_EXT_VERSION
    // dt: nt fDeltaTime values, or nullptr for the times of samples t0 .. t0 + nt - 1
    int (*generate_and_beamform_weighted)(dcs_bf_context *c, const float *dt, uint64_t t0, uint32_t nt,
                                          const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                          float *d_beams, size_t beams_bytes, void *stream);
    // dt_coeff: the coefficients' fDeltaTime, or nullptr for that of sample t_coeff
    int (*beamform_accumulated_weighted)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                         const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                         float *d_beams, size_t beams_bytes, void *stream);
    // the same with int8 output (include/dcs_beam_quant.h); d_weights: nullptr = unweighted; d_clip_count: nullptr = no counting
    int (*beamform_accumulated_q8)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                   const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                   const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                   unsigned long long *d_clip_count, void *stream);
    // the same with detected block power out (include/dcs_beam_power.h): float [C][nt / 16][B]; d_weights: nullptr = unweighted
    int (*beamform_accumulated_power)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                      const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                      float *d_block_power, size_t power_bytes, void *stream);
    // block powers [C][nr_blocks][B] -> spectra [nr_blocks / blocks_per_spectrum][C][B]
    int (*integrate_block_power)(dcs_bf_context *c, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                 uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                 void *stream);
    // the incoherent beam (include/dcs_incoherent_beam.h): exact block powers uint32 [C][nt / 16] of the antennas that
    // d_weights ([A], nullptr = all) flags with a value != 0
    int (*incoherent_block_power)(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                  const float *d_weights, uint32_t *d_block_power, size_t power_bytes, void *stream);
    // block powers [C][nr_blocks] -> spectra [nr_blocks / blocks_per_spectrum][C]
    int (*integrate_incoherent_power)(dcs_bf_context *c, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                      uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                      void *stream);
    // 8-bit search filterbanks (include/dcs_filterbank.h): spectra float [nr_spectra][C][nr_beams] -> running sums double
    // [C][nr_beams][2]; sums -> scales float [C][nr_beams][2]; spectra and scales -> uint8 [nr_beams][out_spectra][C]
    int (*spectra_sums)(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                        uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream);
    int (*filterbank_scales)(dcs_bf_context *c, const double *d_sums, size_t sums_bytes, uint64_t count, uint32_t nr_beams,
                             float target_std, float *d_scales, size_t scales_bytes, void *stream);
    int (*filterbank_q8)(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                         const float *d_scales, float level, uint32_t flags, uint8_t *d_filterbank, size_t filterbank_bytes,
                         uint64_t out_spectra, uint64_t first_spectrum, unsigned long long *d_clip_count, void *stream);
    // the true complex product sum_a w_a x_a (include/dcs_beam_complex.h): float beams, and detected block power; d_weights:
    // nullptr = unweighted; flags: bit 0 = DCS_BF_COMPLEX_CONJ
    int (*beamform_accumulated_complex)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                        const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                        float *d_beams, size_t beams_bytes, void *stream);
    int (*beamform_accumulated_complex_power)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                              const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                              float *d_block_power, size_t power_bytes, void *stream);
    // the complex product with int8 output (include/dcs_beam_complex_quant.h): beamform_accumulated_q8's arguments and flags
    int (*beamform_accumulated_complex_q8)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                           const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                           const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                           unsigned long long *d_clip_count, void *stream);
    // full-Stokes detection (include/dcs_stokes.h): two int8 beam tensors [C][nt / 16][B][16][2] -> exact block Stokes int32
    // [C][nt / 16][B][nr_stokes]; block Stokes [C][nr_blocks][B][nr_stokes] -> spectra [nr_blocks / blocks_per_spectrum][C][B][nr_stokes]
    int (*stokes_block)(dcs_bf_context *c, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                        uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream);
    int (*integrate_stokes)(dcs_bf_context *c, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                            uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                            size_t spectra_bytes, void *stream);
    // incoherent dedispersion (include/dcs_dedisperse.h): a band (host memory) and DMs double [nr_dm] -> delays int32
    // [nr_dm][C]; filterbanks uint8 [nr_beams][in_spectra][C] and delays -> DM-time planes uint32 [nr_beams][nr_dm][out_spectra]
    int (*dm_delays)(dcs_bf_context *c, const dcs_bf_band *band, const double *d_dms, uint32_t nr_dm, int32_t *d_delays,
                     size_t delays_bytes, void *stream);
    int (*dedisperse_q8)(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                         uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays, uint32_t nr_dm,
                         uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t *d_dm_time, size_t dm_time_bytes,
                         uint64_t out_spectra, uint64_t first_out, void *stream);
    // the single-pulse search (include/dcs_single_pulse.h) on those planes: the exact sums uint64 [nr_beams][nr_dm][2] of every
    // series; boxcar peaks uint32 [nr_beams][nr_dm][nr_widths][peak_blocks][2]; peaks and sums -> signal-to-noise float
    // [nr_beams][nr_dm][nr_widths][peak_blocks] and the best width uint32 [nr_beams][nr_dm][peak_blocks] (nullptr = not wanted)
    int (*dm_time_sums)(dcs_bf_context *c, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, uint32_t accumulate,
                        uint64_t *d_sums, size_t sums_bytes, void *stream);
    int (*boxcar_peaks)(dcs_bf_context *c, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                        uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths,
                        uint32_t nr_widths, uint32_t max_width, uint32_t block_len, uint32_t *d_peaks, size_t peaks_bytes,
                        uint64_t peak_blocks, uint64_t first_block, void *stream);
    int (*peak_snr)(dcs_bf_context *c, const uint32_t *d_peaks, size_t peaks_bytes, uint64_t peak_blocks, uint64_t first_block,
                    uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths, uint32_t nr_widths,
                    uint32_t max_width, const uint64_t *d_sums, size_t sums_bytes, uint64_t count, float *d_snr, size_t snr_bytes,
                    uint32_t *d_best, size_t best_bytes, void *stream);
    // the correlator (include/dcs_correlator.h): the sample tensor -> exact visibilities int32 [C][nr_vis][NB][{re, im}] of
    // the pairs b <= a, nr_vis = (nt / 16) / blocks_per_vis; visibilities -> float [nr_vis / vis_per_integration][C][NB][{re, im}]
    int (*correlate_block)(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, uint32_t blocks_per_vis,
                           int32_t *d_vis, size_t vis_bytes, void *stream);
    int (*integrate_visibilities)(dcs_bf_context *c, const int32_t *d_vis, size_t vis_bytes, uint32_t nr_vis,
                                  uint32_t vis_per_integration, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream);
    // the digital down-converter (include/dcs_ddc.h): integer taps -> the operand table; real int8 [nr_inputs][in_stride] ->
    // float [band][input][out_stride][{re, im}], mixed, filtered and decimated by 16
    int (*ddc_tap_digits)(dcs_bf_context *c, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, void *d_digits,
                          size_t digits_bytes, void *stream);
    int (*ddc)(dcs_bf_context *c, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes,
               uint64_t in_stride, const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands,
               const dcs_ddc_band *bands, uint64_t first_output, float *d_out, size_t out_bytes, uint64_t out_stride, void *stream);
    // the candidate sifter (include/dcs_candidates.h): signal-to-noise float [nr_beams][nr_dm][nr_widths][peak_blocks] and the
    // peaks behind it -> dcs_bf_candidate [max_candidates] in ascending (beam, DM, block) and d_count = {found, written}
    int (*find_candidates)(dcs_bf_context *c, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                           uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                           uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, void *d_cands,
                           size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes,
                           void *stream);
    // the polyphase channeliser (include/dcs_channeliser.h): float [nr_inputs][in_stride][{re, im}] -> the spectra of a FIR of
    // nr_taps rows of nr_channels pairs and an nr_channels-point butterfly network, [nr_channels][out_blocks][out_inputs][16][{re, im}]
    // as floats, or quantised with gains float [nr_inputs][nr_channels]; d_clip_count: nullptr = no counting
    int (*channelise)(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                      const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles,
                      uint32_t order, float *d_out, size_t out_bytes, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs,
                      uint32_t first_input, void *stream);
    int (*channelise_q8)(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                         const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles,
                         uint32_t order, const float *d_gains, int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks,
                         uint64_t first_block, uint32_t out_inputs, uint32_t first_input, unsigned long long *d_clip_count,
                         void *stream);
    // the RFI flagger (include/dcs_rfi.h): filterbanks uint8 [nr_beams][in_spectra][C] -> {sum x, sum x^2} uint32
    // [nr_beams][nr_blocks][C][2] and the zero-DM series uint32 [nr_beams][nr_blocks * block_len] (nullptr = not wanted); those ->
    // cell flags uint8 [nr_beams][nr_blocks][C], channel masks uint8 [nr_beams][C], spectrum flags uint8 [nr_beams][nr_blocks *
    // block_len] and counts uint32 [nr_beams][3]; filterbanks and any of the flags (nullptr = none) -> the cleaned filterbanks
    int (*rfi_moments)(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                       uint64_t first_spectrum, uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, uint32_t *d_cell_sums,
                       size_t cell_sums_bytes, uint32_t *d_zero_dm, size_t zero_dm_bytes, void *stream);
    int (*rfi_flags)(dcs_bf_context *c, const uint32_t *d_cell_sums, size_t cell_sums_bytes, const uint32_t *d_zero_dm,
                     size_t zero_dm_bytes, uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const dcs_bf_rfi_thresholds *thr,
                     uint8_t *d_cell_flags, size_t cell_flags_bytes, uint8_t *d_channel_mask, size_t channel_mask_bytes,
                     uint8_t *d_spectrum_flags, size_t spectrum_flags_bytes, uint32_t *d_counts, size_t counts_bytes, void *stream);
    int (*rfi_clean_q8)(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                        uint64_t first_spectrum, uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const uint8_t *d_cell_flags,
                        const uint8_t *d_channel_mask, const uint8_t *d_spectrum_flags, uint8_t fill, uint8_t *d_out, size_t out_bytes,
                        uint64_t out_spectra, uint64_t first_out, unsigned long long *d_replaced, void *stream);
};

// the first member of struct dcs_bf_context
struct bf_ctx_ext_head {
    const bf_ctx_ext_ops *ops;
};

// a companion's way to the table, once the entry's checks have found c non-null: nullptr where the versions differ
static inline const bf_ctx_ext_ops *ops_of(dcs_bf_context *c)
{
    const bf_ctx_ext_ops *ops = reinterpret_cast<const bf_ctx_ext_head *>(c)->ops;
    return ops && ops->version == BF_CTX_EXT_VERSION ? ops : nullptr;
}

// a companion's call of one entry with the arguments a: DCS_ERR_UNSUPPORTED where the versions differ
template <class F, class... A>
int forward(dcs_bf_context *c, F bf_ctx_ext_ops::*entry, A... a)
{
    const bf_ctx_ext_ops *ops = ops_of(c);
    return ops ? (ops->*entry)(c, a...) : DCS_ERR_UNSUPPORTED;
}

#endif // BF_CTX_EXT_H
