// bf_ctx_ext.h -- the internal contract between libdcs_beamformer.so and its companion libraries: dc_sand_amd/companions.py
// is their list, each with its public header.  All are built from this tree together.  Every dcs_bf_context begins with a
// bf_ctx_ext_head whose table points at the product library's implementation of the companions' calls; a companion's
// export is two statements: the entry's device-free checks (bf_arg_checks.h, where the implementation behind the table
// takes them from too), then forward(), which checks the table's version and calls the entry.  Not a public interface.
//
// An entry whose signature is its export's takes its type from the public declaration, decltype(dcs_bf_NAME) *, so the
// parameter list is stated once, in the public header; bf_host.h declares the function behind the entry the same way.
#ifndef BF_CTX_EXT_H
#define BF_CTX_EXT_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/dcs_beam_power.h"
#include "../../include/dcs_beamformer.h"
#include "../../include/dcs_channeliser.h"
#include "../../include/dcs_correlator.h"
#include "../../include/dcs_incoherent_beam.h"
#include "../../include/dcs_single_pulse.h"
#include "bf_arg_checks.h" // and through it the public headers of the other entries

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
// 17: fold_q8, fold_scrunch appended (tests/test_host_abi_fold.py hands its companion 1, 15 and 16; no older test hands a
// foreign version above 15).
#define BF_CTX_EXT_VERSION 17u

struct bf_ctx_ext_ops {
    uint32_t version; // BF_CTX_EXT_VERSION
    // The seven beamformer entries are written out: they are no export's signature, each merges the time-index and the _dt
    // export of its call into one entry.
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
    decltype(dcs_bf_integrate_block_power) *integrate_block_power;
    // the incoherent beam (include/dcs_incoherent_beam.h): exact block powers uint32 [C][nt / 16] of the antennas that
    // d_weights ([A], nullptr = all) flags with a value != 0
    decltype(dcs_bf_incoherent_block_power) *incoherent_block_power;
    // block powers [C][nr_blocks] -> spectra [nr_blocks / blocks_per_spectrum][C]
    decltype(dcs_bf_integrate_incoherent_power) *integrate_incoherent_power;
    // 8-bit search filterbanks (include/dcs_filterbank.h): spectra float [nr_spectra][C][nr_beams] -> running sums double
    // [C][nr_beams][2]; sums -> scales float [C][nr_beams][2]; spectra and scales -> uint8 [nr_beams][out_spectra][C]
    decltype(dcs_bf_spectra_sums) *spectra_sums;
    decltype(dcs_bf_filterbank_scales) *filterbank_scales;
    decltype(dcs_bf_filterbank_q8) *filterbank_q8;
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
    decltype(dcs_bf_stokes_block) *stokes_block;
    decltype(dcs_bf_integrate_stokes) *integrate_stokes;
    // incoherent dedispersion (include/dcs_dedisperse.h): a band (host memory) and DMs double [nr_dm] -> delays int32
    // [nr_dm][C]; filterbanks uint8 [nr_beams][in_spectra][C] and delays -> DM-time planes uint32 [nr_beams][nr_dm][out_spectra]
    decltype(dcs_bf_dm_delays) *dm_delays;
    decltype(dcs_bf_dedisperse_q8) *dedisperse_q8;
    // the single-pulse search (include/dcs_single_pulse.h) on those planes: the exact sums uint64 [nr_beams][nr_dm][2] of every
    // series; boxcar peaks uint32 [nr_beams][nr_dm][nr_widths][peak_blocks][2]; peaks and sums -> signal-to-noise float
    // [nr_beams][nr_dm][nr_widths][peak_blocks] and the best width uint32 [nr_beams][nr_dm][peak_blocks] (nullptr = not wanted)
    decltype(dcs_bf_dm_time_sums) *dm_time_sums;
    decltype(dcs_bf_boxcar_peaks) *boxcar_peaks;
    decltype(dcs_bf_peak_snr) *peak_snr;
    // the correlator (include/dcs_correlator.h): the sample tensor -> exact visibilities int32 [C][nr_vis][NB][{re, im}] of
    // the pairs b <= a, nr_vis = (nt / 16) / blocks_per_vis; visibilities -> float [nr_vis / vis_per_integration][C][NB][{re, im}]
    decltype(dcs_bf_correlate_block) *correlate_block;
    decltype(dcs_bf_integrate_visibilities) *integrate_visibilities;
    // the digital down-converter (include/dcs_ddc.h): integer taps -> the operand table; real int8 [nr_inputs][in_stride] ->
    // float [band][input][out_stride][{re, im}], mixed, filtered and decimated by 16
    decltype(dcs_bf_ddc_tap_digits) *ddc_tap_digits;
    decltype(dcs_bf_ddc) *ddc;
    // the candidate sifter (include/dcs_candidates.h): signal-to-noise float [nr_beams][nr_dm][nr_widths][peak_blocks] and the
    // peaks behind it -> dcs_bf_candidate [max_candidates] in ascending (beam, DM, block) and d_count = {found, written}
    // written out too: the export's d_cands is a dcs_bf_candidate *, the entry's a void *
    int (*find_candidates)(dcs_bf_context *c, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                           uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                           uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, void *d_cands,
                           size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes,
                           void *stream);
    // the polyphase channeliser (include/dcs_channeliser.h): float [nr_inputs][in_stride][{re, im}] -> the spectra of a FIR of
    // nr_taps rows of nr_channels pairs and an nr_channels-point butterfly network, [nr_channels][out_blocks][out_inputs][16][{re, im}]
    // as floats, or quantised with gains float [nr_inputs][nr_channels]; d_clip_count: nullptr = no counting
    decltype(dcs_bf_channelise) *channelise;
    decltype(dcs_bf_channelise_q8) *channelise_q8;
    // the RFI flagger (include/dcs_rfi.h): filterbanks uint8 [nr_beams][in_spectra][C] -> {sum x, sum x^2} uint32
    // [nr_beams][nr_blocks][C][2] and the zero-DM series uint32 [nr_beams][nr_blocks * block_len] (nullptr = not wanted); those ->
    // cell flags uint8 [nr_beams][nr_blocks][C], channel masks uint8 [nr_beams][C], spectrum flags uint8 [nr_beams][nr_blocks *
    // block_len] and counts uint32 [nr_beams][3]; filterbanks and any of the flags (nullptr = none) -> the cleaned filterbanks
    decltype(dcs_bf_rfi_moments) *rfi_moments;
    decltype(dcs_bf_rfi_flags) *rfi_flags;
    decltype(dcs_bf_rfi_clean_q8) *rfi_clean_q8;
    // the pulsar folder (include/dcs_fold.h): filterbanks uint8 [nr_beams][in_spectra][C], phase models [P][nr_subints] and delays
    // int32 [P][C] (nullptr = none) -> profiles uint32 [nr_beams][out_subints][C][nbin] and hits uint32 [P][out_subints][nbin]
    // (nullptr = not wanted); profiles -> their sums over C, uint64 [nr_beams][out_subints][nbin]
    decltype(dcs_bf_fold_q8) *fold_q8;
    decltype(dcs_bf_fold_scrunch) *fold_scrunch;
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
