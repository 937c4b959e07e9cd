// bf_capi_detect.hip -- what comes after detection: the integration of block powers (include/dcs_beam_power.h), the
// incoherent beam (include/dcs_incoherent_beam.h), the search filterbanks (include/dcs_filterbank.h), the Stokes
// detection of 8-bit beams (include/dcs_stokes.h), the dedispersion of the filterbanks (include/dcs_dedisperse.h), the
// single-pulse search on its planes (include/dcs_single_pulse.h), the correlator (include/dcs_correlator.h), the digital
// down-converter (include/dcs_ddc.h), the candidate sifter (include/dcs_candidates.h), the polyphase channeliser
// (include/dcs_channeliser.h) and the RFI flagger (include/dcs_rfi.h), each reached through the table at the head of every context (bf_ctx_ext.h).  Of the context these calls use its parameters and its device, nothing
// else.  Each begins with the device-free checks of its table entry (bf_arg_checks.h), the ones its companion has made
// already; what follows needs the device or the context's sizes, or is a condition that only this side makes.  Host code
// only; the kernels are in bf_integrate.hip, bf_incoherent.hip, bf_filterbank.hip, bf_stokes.hip, bf_dedisperse.hip,
// bf_single_pulse.hip, bf_correlator.hip, bf_ddc.hip, bf_candidates.hip, bf_channeliser.hip and bf_rfi.hip.

#include <cmath>
#include <cstring>

#include "bf_host.h"

using namespace bf_host;

namespace bf_host {

// The one integration behind integrate_block_power, integrate_incoherent_power, integrate_stokes and integrate_visibilities
// (bf_integrate.hip): blocks [C][nr_blocks][bs] of 4-byte words of the named type, n at a time, into out [nr_blocks / n][C][bs].
// The caller has made its own device-free checks: n >= 1 divides nr_blocks.
static int integrate_blocks(dcs_bf_context *c, bf_integrate_type type, const void *d_blocks, size_t blocks_bytes, uint64_t bs,
                            uint32_t nr_blocks, uint32_t n, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream)
{
    DCS_CHECK_DEVICE(c);
    const uint64_t C = (uint32_t)c->p.nr_channels, n_out = nr_blocks / n;
    if (bs > 0xffffffffull) return DCS_ERR_UNSUPPORTED;
    if (!holds(blocks_bytes, C, nr_blocks, bs, 4u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(out_bytes, n_out, C, bs, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    bf_integrate_args a;
    std::memset(&a, 0, sizeof(a));
    a.blocks = d_blocks;
    a.out = d_out;
    a.total = n_out * C * bs;
    a.bs = (uint32_t)bs;
    a.C = (uint32_t)C;
    a.nr_blocks = nr_blocks;
    a.n = n;
    a.accumulate = accumulate ? 1u : 0u;
    return (int)bf_launch_integrate(type, a, as_stream(stream));
}

int integrate_block_power_impl(dcs_bf_context *c, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                               uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes, void *stream)
{
    if (int e = integrate_block_power_args(c, d_block_power, nr_blocks, blocks_per_spectrum, d_spectra)) return e;
    return integrate_blocks(c, BF_INTEGRATE_F32, d_block_power, power_bytes, (uint32_t)c->p.nr_beams, nr_blocks, blocks_per_spectrum,
                            accumulate, d_spectra, spectra_bytes, stream);
}

// include/dcs_incoherent_beam.h, reached the same way.  No coefficients: no delay table, no terms, nothing allocated, and
// math_mode plays no part.
int incoherent_block_power_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                uint32_t *d_block_power, size_t power_bytes, void *stream)
{
    if (int e = incoherent_block_power_args(c, nt, d_weights, d_block_power)) return e;
    if (nt && !d_antenna) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    const uint32_t A = (uint32_t)c->p.nr_stations, C = (uint32_t)c->p.nr_channels;
    if (A > 256u) return DCS_ERR_UNSUPPORTED; // as the float call
    if (antenna_bytes < (size_t)A * C * nt * 2u) return DCS_ERR_INVALID_ARGUMENT;
    if (power_bytes < (size_t)C * (nt / 16u) * sizeof(uint32_t)) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_antenna, 16u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_incoh_args a;
    std::memset(&a, 0, sizeof(a));
    a.ant = d_antenna;
    a.weights = d_weights;
    a.block_power = d_block_power;
    a.rows = (uint64_t)C * (nt / 16u);
    a.A = A;
    return (int)bf_launch_incoherent_power(a, as_stream(stream));
}

int integrate_incoherent_power_impl(dcs_bf_context *c, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                    uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                    void *stream)
{
    if (int e = integrate_incoherent_power_args(c, d_block_power, nr_blocks, blocks_per_spectrum, d_spectra)) return e;
    return integrate_blocks(c, BF_INTEGRATE_U32, d_block_power, power_bytes, 1u, nr_blocks, blocks_per_spectrum, accumulate, d_spectra,
                            spectra_bytes, stream);
}

// include/dcs_filterbank.h, reached the same way.  No coefficients and nothing allocated; nr_beams is the caller's, so the
// one set of calls serves detected (the context's beams) and incoherent (1) spectra.
int spectra_sums_impl(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                      uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream)
{
    if (int e = spectra_sums_args(c, d_spectra, nr_beams, d_sums)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(spectra_bytes, nr_spectra, C, nr_beams, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(sums_bytes, C, nr_beams, 2u, sizeof(double))) return DCS_ERR_INVALID_ARGUMENT;
    bf_fbsums_args a;
    std::memset(&a, 0, sizeof(a));
    a.spectra = d_spectra;
    a.sums = d_sums;
    a.cb = (uint64_t)C * nr_beams;
    a.T = nr_spectra;
    a.accumulate = accumulate ? 1u : 0u;
    return (int)bf_launch_spectra_sums(a, as_stream(stream));
}

int filterbank_scales_impl(dcs_bf_context *c, const double *d_sums, size_t sums_bytes, uint64_t count, uint32_t nr_beams,
                           float target_std, float *d_scales, size_t scales_bytes, void *stream)
{
    if (int e = filterbank_scales_args(c, d_sums, count, nr_beams, d_scales)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(sums_bytes, C, nr_beams, 2u, sizeof(double))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(scales_bytes, C, nr_beams, 2u, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    bf_fbscales_args a;
    std::memset(&a, 0, sizeof(a));
    a.sums = d_sums;
    a.scales = d_scales;
    a.cb = (uint64_t)C * nr_beams;
    a.count = count;
    a.target_std = target_std;
    return (int)bf_launch_filterbank_scales(a, as_stream(stream));
}

int filterbank_q8_impl(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                       const float *d_scales, float level, uint32_t flags, uint8_t *d_filterbank, size_t filterbank_bytes,
                       uint64_t out_spectra, uint64_t first_spectrum, unsigned long long *d_clip_count, void *stream)
{
    if (int e = filterbank_q8_args(c, d_spectra, nr_spectra, nr_beams, d_scales, flags, d_filterbank, out_spectra, first_spectrum,
                                   d_clip_count))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(spectra_bytes, nr_spectra, C, nr_beams, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(filterbank_bytes, nr_beams, out_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_fbq8_args a;
    std::memset(&a, 0, sizeof(a));
    a.spectra = d_spectra;
    a.scales = d_scales;
    a.out = d_filterbank;
    a.clip_count = d_clip_count;
    a.out_spectra = out_spectra;
    a.first = first_spectrum;
    a.C = C;
    a.B = nr_beams;
    a.T = nr_spectra;
    a.descending = flags & DCS_FB_DESCENDING;
    a.level = level;
    return (int)bf_launch_filterbank_q8(a, as_stream(stream));
}

// include/dcs_stokes.h, reached the same way.  No coefficients, nothing allocated, and math_mode plays no part.
int stokes_block_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                      uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream)
{
    if (int e = stokes_block_args(c, nt, d_beams_x, d_beams_y, nr_stokes, d_block_stokes)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t B = (uint32_t)c->p.nr_beams, C = (uint32_t)c->p.nr_channels;
    if (!holds(beams_bytes, C, nt, B, 2u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(stokes_bytes, C, nt / 16u, B, (uint64_t)nr_stokes * sizeof(int32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_stokes_args a;
    std::memset(&a, 0, sizeof(a));
    a.beams_x = d_beams_x;
    a.beams_y = d_beams_y;
    a.block_stokes = d_block_stokes;
    a.rows = (uint64_t)C * (nt / 16u) * B;
    a.nr_stokes = nr_stokes;
    return (int)bf_launch_stokes_block(a, as_stream(stream));
}

int integrate_stokes_impl(dcs_bf_context *c, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                          uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                          size_t spectra_bytes, void *stream)
{
    if (int e = integrate_stokes_args(c, d_block_stokes, nr_blocks, blocks_per_spectrum, nr_stokes, d_spectra)) return e;
    return integrate_blocks(c, BF_INTEGRATE_I32, d_block_stokes, stokes_bytes, (uint64_t)(uint32_t)c->p.nr_beams * nr_stokes, nr_blocks,
                            blocks_per_spectrum, accumulate, d_spectra, spectra_bytes, stream);
}

// include/dcs_dedisperse.h, reached the same way.  No coefficients, nothing allocated, and math_mode plays no part; the band
// is host memory and travels by value in the kernel's arguments.
int dm_delays_impl(dcs_bf_context *c, const dcs_bf_band *band, const double *d_dms, uint32_t nr_dm, int32_t *d_delays,
                   size_t delays_bytes, void *stream)
{
    if (int e = dm_delays_args(c, band, d_dms, d_delays)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    const double f_last = band->freq_first_mhz + (double)(C - 1u) * band->freq_step_mhz; // the kernel's own f_(C-1)
    if (!(f_last > 0.0) || !std::isfinite(f_last)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(delays_bytes, nr_dm, C, sizeof(int32_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_dmdelay_args a;
    std::memset(&a, 0, sizeof(a));
    a.dms = d_dms;
    a.delays = d_delays;
    a.total = (uint64_t)nr_dm * C;
    a.C = C;
    a.freq_first = band->freq_first_mhz;
    a.freq_step = band->freq_step_mhz;
    a.sample_time = band->sample_time_s;
    return (int)bf_launch_dm_delays(a, as_stream(stream));
}

int dedisperse_q8_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                       uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays, uint32_t nr_dm,
                       uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t *d_dm_time, size_t dm_time_bytes,
                       uint64_t out_spectra, uint64_t first_out, void *stream)
{
    if (int e = dedisperse_q8_args(c, d_filterbank, in_spectra, first_spectrum, nr_spectra, nr_beams, d_delays, max_delay, d_dm_time,
                                   out_spectra, first_out))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(filterbank_bytes, nr_beams, in_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(dm_time_bytes, nr_beams, nr_dm, out_spectra, sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_dedisp_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_filterbank;
    a.delays = d_delays;
    a.mask = d_channel_mask;
    a.out = d_dm_time;
    a.in_spectra = in_spectra;
    a.first = first_spectrum;
    a.out_spectra = out_spectra;
    a.first_out = first_out;
    a.C = C;
    a.B = nr_beams;
    a.T = nr_spectra;
    a.nr_dm = nr_dm;
    a.max_delay = max_delay;
    return (int)bf_launch_dedisperse(a, as_stream(stream));
}

// include/dcs_single_pulse.h, reached the same way.  Nothing allocated; of the context only its device is used.  A series is
// one (beam, DM) pair; nr_beams * nr_dm of them fit 64 bits.
int dm_time_sums_impl(dcs_bf_context *c, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                      uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, uint32_t accumulate,
                      uint64_t *d_sums, size_t sums_bytes, void *stream)
{
    if (int e = dm_time_sums_args(c, d_dm_time, plane_spectra, first_spectrum, nr_spectra, nr_beams, d_sums)) return e;
    DCS_CHECK_DEVICE(c);
    const uint64_t series = (uint64_t)nr_beams * nr_dm;
    if (!holds(dm_time_bytes, series, plane_spectra, sizeof(uint32_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(sums_bytes, series, 2u, sizeof(uint64_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_dtsums_args a;
    std::memset(&a, 0, sizeof(a));
    a.plane = d_dm_time;
    a.sums = d_sums;
    a.plane_spectra = plane_spectra;
    a.first = first_spectrum;
    a.T = nr_spectra;
    a.accumulate = accumulate ? 1u : 0u;
    return (int)bf_launch_dm_time_sums(a, series, as_stream(stream));
}

int boxcar_peaks_impl(dcs_bf_context *c, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                      uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths,
                      uint32_t nr_widths, uint32_t max_width, uint32_t block_len, uint32_t *d_peaks, size_t peaks_bytes,
                      uint64_t peak_blocks, uint64_t first_block, void *stream)
{
    if (int e = boxcar_peaks_args(c, d_dm_time, plane_spectra, first_spectrum, nr_spectra, nr_beams, d_widths, max_width, block_len,
                                  d_peaks, peak_blocks, first_block))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint64_t series = (uint64_t)nr_beams * nr_dm;
    if (!holds(dm_time_bytes, series, plane_spectra, sizeof(uint32_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(peaks_bytes, series, nr_widths, peak_blocks, 2u * sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_boxcar_args a;
    std::memset(&a, 0, sizeof(a));
    a.plane = d_dm_time;
    a.widths = d_widths;
    a.peaks = d_peaks;
    a.plane_spectra = plane_spectra;
    a.first = first_spectrum;
    a.peak_blocks = peak_blocks;
    a.first_block = first_block;
    a.T = nr_spectra;
    a.nr_widths = nr_widths;
    a.max_width = max_width;
    a.block_len = block_len;
    return (int)bf_launch_boxcar_peaks(a, series, as_stream(stream));
}

int peak_snr_impl(dcs_bf_context *c, const uint32_t *d_peaks, size_t peaks_bytes, uint64_t peak_blocks, uint64_t first_block,
                  uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths, uint32_t nr_widths,
                  uint32_t max_width, const uint64_t *d_sums, size_t sums_bytes, uint64_t count, float *d_snr, size_t snr_bytes,
                  uint32_t *d_best, size_t best_bytes, void *stream)
{
    if (int e = peak_snr_args(c, d_peaks, peak_blocks, first_block, nr_blocks, nr_beams, d_widths, max_width, d_sums, count, d_snr,
                              d_best))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint64_t series = (uint64_t)nr_beams * nr_dm;
    if (!holds(peaks_bytes, series, nr_widths, peak_blocks, 2u * sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(sums_bytes, series, 2u, sizeof(uint64_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(snr_bytes, series, nr_widths, peak_blocks, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    if (d_best && !holds(best_bytes, series, peak_blocks, sizeof(uint32_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    const unsigned __int128 total = (unsigned __int128)series * nr_blocks;
    if (total >> 64) return DCS_ERR_INVALID_ARGUMENT;
    bf_peaksnr_args a;
    std::memset(&a, 0, sizeof(a));
    a.peaks = d_peaks;
    a.widths = d_widths;
    a.sums = d_sums;
    a.snr = d_snr;
    a.best = d_best;
    a.peak_blocks = peak_blocks;
    a.first_block = first_block;
    a.count = count;
    a.total = (uint64_t)total;
    a.nr_blocks = nr_blocks;
    a.nr_widths = nr_widths;
    a.max_width = max_width;
    return (int)bf_launch_peak_snr(a, as_stream(stream));
}

// include/dcs_correlator.h, reached the same way.  No coefficients, nothing allocated, and math_mode plays no part.
int correlate_block_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, uint32_t blocks_per_vis,
                         int32_t *d_vis, size_t vis_bytes, void *stream)
{
    if (int e = correlate_block_args(c, nt, blocks_per_vis, d_vis)) return e;
    if (nt && !d_antenna) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    const uint32_t A = (uint32_t)c->p.nr_stations, C = (uint32_t)c->p.nr_channels;
    const uint32_t nr_vis = nt / 16u / blocks_per_vis;
    if (A > 256u) return DCS_ERR_UNSUPPORTED; // as the float call
    if (!aligned(d_antenna, 16u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(antenna_bytes, C, nt, A, 2u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(vis_bytes, C, nr_vis, (uint64_t)A * (A + 1u) / 2u, 2u * sizeof(int32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_corr_args a;
    std::memset(&a, 0, sizeof(a));
    a.ant = d_antenna;
    a.vis = d_vis;
    a.A = A;
    a.C = C;
    a.nT16 = nt / 16u;
    a.n = blocks_per_vis;
    a.nr_vis = nr_vis;
    return (int)bf_launch_correlate(a, as_stream(stream));
}

// a (channel, visibility) row is 2 NB = A (A + 1) words
int integrate_visibilities_impl(dcs_bf_context *c, const int32_t *d_vis, size_t vis_bytes, uint32_t nr_vis, uint32_t vis_per_integration,
                                uint32_t accumulate, float *d_out, size_t out_bytes, void *stream)
{
    if (int e = integrate_visibilities_args(c, d_vis, nr_vis, vis_per_integration, d_out)) return e;
    const uint64_t A = (uint32_t)c->p.nr_stations;
    return integrate_blocks(c, BF_INTEGRATE_I32, d_vis, vis_bytes, A * (A + 1u), nr_vis, vis_per_integration, accumulate, d_out, out_bytes,
                            stream);
}

// include/dcs_ddc.h, reached the same way.  Of the context these use the device alone: every size is an argument, and the
// device-free checks are all the checks there are.
int ddc_tap_digits_impl(dcs_bf_context *c, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, void *d_digits,
                        size_t digits_bytes, void *stream)
{
    if (int e = ddc_tap_digits_args(c, d_taps, nr_taps, nr_bands, d_digits, digits_bytes)) return e;
    DCS_CHECK_DEVICE(c);
    bf_ddc_digits_args a;
    std::memset(&a, 0, sizeof(a));
    a.taps = d_taps;
    a.digits = static_cast<int8_t *>(d_digits);
    a.T = nr_taps;
    a.nr_bands = nr_bands;
    return (int)bf_launch_ddc_tap_digits(a, as_stream(stream));
}

// the oscillator of output m of the call is phase0 + 16 (first_output + m) phase_step mod 2^32: the part that does not depend on
// m is made here, in wrapping 32-bit arithmetic
int ddc_impl(dcs_bf_context *c, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes, uint64_t in_stride,
             const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands, const dcs_ddc_band *bands,
             uint64_t first_output, float *d_out, size_t out_bytes, uint64_t out_stride, void *stream)
{
    if (int e = ddc_args(c, nr_inputs, nr_out, d_samples, samples_bytes, in_stride, d_digits, digits_bytes, nr_taps, nr_bands, bands,
                         d_out, out_bytes, out_stride))
        return e;
    DCS_CHECK_DEVICE(c);
    if (nr_out == 0u || nr_inputs == 0u) return DCS_OK;
    bf_ddc_args a;
    std::memset(&a, 0, sizeof(a));
    a.x = d_samples;
    a.digits = static_cast<const int8_t *>(d_digits);
    a.out = d_out;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.nr_inputs = nr_inputs;
    a.nr_out = nr_out;
    a.T = nr_taps;
    a.nr_bands = nr_bands;
    for (uint32_t b = 0; b < nr_bands; b++) {
        a.step16[b] = 16u * bands[b].phase_step;
        a.u0[b] = bands[b].phase0 + (uint32_t)first_output * a.step16[b];
        a.gain[b] = bands[b].gain;
    }
    return (int)bf_launch_ddc(a, as_stream(stream));
}

// include/dcs_candidates.h, reached the same way.  Nothing allocated; of the context only its device is used.  The counts
// and a record's block are 32-bit words: a call with 2^32 cells or more, or with a block past 2^32, is not supported.
int find_candidates_impl(dcs_bf_context *c, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                         uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                         uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, void *d_cands,
                         size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes, void *stream)
{
    if (int e = find_candidates_args(c, d_snr, d_peaks, peak_blocks, first_block, nr_blocks, nr_beams, threshold, dm_radius,
                                     block_radius, d_cands, max_candidates, d_count, d_work))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint64_t series = (uint64_t)nr_beams * nr_dm;
    if (((unsigned __int128)series * nr_blocks >> 32) || first_block + nr_blocks > (1ull << 32)) return DCS_ERR_UNSUPPORTED;
    if (!holds(snr_bytes, series, nr_widths, peak_blocks, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(peaks_bytes, series, nr_widths, peak_blocks, 2u * sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(cands_bytes, max_candidates, 32u, 1u, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (work_bytes < candidates_workspace_bytes(nr_beams, nr_dm, nr_blocks)) return DCS_ERR_INVALID_ARGUMENT;
    const uint64_t segments = (uint64_t)candidates_segments(nr_beams, nr_dm, nr_blocks); // no more than the cells
    bf_cand_args a;
    std::memset(&a, 0, sizeof(a));
    a.snr = d_snr;
    a.peaks = d_peaks;
    a.cands = static_cast<uint32_t *>(d_cands);
    a.count = d_count;
    a.marks = static_cast<uint64_t *>(d_work);
    a.places = reinterpret_cast<uint32_t *>(a.marks + segments);
    a.peak_blocks = peak_blocks;
    a.first_block = first_block;
    a.B = nr_beams;
    a.nr_dm = nr_dm;
    a.nr_blocks = nr_blocks;
    a.nr_widths = nr_widths;
    a.dm_radius = dm_radius;
    a.block_radius = block_radius;
    a.max_candidates = max_candidates;
    a.threshold = threshold;
    return (int)bf_launch_find_candidates(a, as_stream(stream));
}

// include/dcs_channeliser.h, reached the same way.  Of the context these use the device alone: every size is an argument, and
// the device-free checks are all the checks there are.  Nothing allocated: one launch each.
static int channelise_launch(dcs_bf_context *c, uint32_t N, uint32_t P, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                             uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order, const float *d_gains,
                             float *d_out, int8_t *d_out_q8, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs,
                             uint32_t first_input, unsigned long long *d_clip_count, void *stream)
{
    DCS_CHECK_DEVICE(c);
    if (nr_spectra == 0u || nr_inputs == 0u) return DCS_OK;
    bf_chan_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_in;
    a.taps = d_taps;
    a.twiddles = d_twiddles;
    a.gains = d_gains;
    a.out = d_out;
    a.out_q8 = d_out_q8;
    a.clip_count = d_clip_count;
    a.in_stride = in_stride;
    a.out_blocks = out_blocks;
    a.first_block = first_block;
    a.N = N;
    a.P = P;
    a.nr_inputs = nr_inputs;
    a.nr_spectra = nr_spectra;
    a.order = order;
    a.out_inputs = out_inputs;
    a.first_input = first_input;
    return (int)bf_launch_channelise(a, as_stream(stream));
}

int channelise_impl(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                    size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order, float *d_out,
                    size_t out_bytes, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs, uint32_t first_input, void *stream)
{
    if (int e = channelise_args(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles, order,
                                d_out, 4u, out_bytes, out_blocks, first_block, out_inputs, first_input))
        return e;
    return channelise_launch(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_stride, d_taps, d_twiddles, order, nullptr, d_out,
                             nullptr, out_blocks, first_block, out_inputs, first_input, nullptr, stream);
}

int channelise_q8_impl(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                       const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order,
                       const float *d_gains, int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks, uint64_t first_block,
                       uint32_t out_inputs, uint32_t first_input, unsigned long long *d_clip_count, void *stream)
{
    if (int e = channelise_q8_args(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles, order,
                                   d_gains, d_out_q8, out_bytes, out_blocks, first_block, out_inputs, first_input, d_clip_count))
        return e;
    return channelise_launch(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_stride, d_taps, d_twiddles, order, d_gains, nullptr,
                             d_out_q8, out_blocks, first_block, out_inputs, first_input, d_clip_count, stream);
}

// include/dcs_rfi.h, reached the same way.  Nothing allocated; of the context the channel count and the device are used.  The
// sizes that need C are checked here; the thresholds are host memory and travel by value in the kernels' arguments.
int rfi_moments_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra, uint64_t first_spectrum,
                     uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, uint32_t *d_cell_sums, size_t cell_sums_bytes,
                     uint32_t *d_zero_dm, size_t zero_dm_bytes, void *stream)
{
    if (int e = rfi_moments_args(c, d_filterbank, in_spectra, first_spectrum, nr_blocks, block_len, nr_beams, d_cell_sums, d_zero_dm,
                                 zero_dm_bytes))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(filterbank_bytes, nr_beams, in_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(cell_sums_bytes, nr_beams, nr_blocks, C, 2u * sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_rfi_moments_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_filterbank;
    a.cell_sums = d_cell_sums;
    a.zero_dm = d_zero_dm;
    a.in_spectra = in_spectra;
    a.first = first_spectrum;
    a.C = C;
    a.B = nr_beams;
    a.nr_blocks = nr_blocks;
    a.block_len = block_len;
    return (int)bf_launch_rfi_moments(a, as_stream(stream));
}

int rfi_flags_impl(dcs_bf_context *c, const uint32_t *d_cell_sums, size_t cell_sums_bytes, const uint32_t *d_zero_dm, size_t zero_dm_bytes,
                   uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const dcs_bf_rfi_thresholds *thr, uint8_t *d_cell_flags,
                   size_t cell_flags_bytes, uint8_t *d_channel_mask, size_t channel_mask_bytes, uint8_t *d_spectrum_flags,
                   size_t spectrum_flags_bytes, uint32_t *d_counts, size_t counts_bytes, void *stream)
{
    if (int e = rfi_flags_args(c, d_cell_sums, d_zero_dm, zero_dm_bytes, nr_blocks, block_len, nr_beams, thr, d_cell_flags, d_channel_mask,
                               d_spectrum_flags, spectrum_flags_bytes, d_counts, counts_bytes))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(cell_sums_bytes, nr_beams, nr_blocks, C, 2u * sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(cell_flags_bytes, nr_beams, nr_blocks, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(channel_mask_bytes, nr_beams, C, 1u, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_rfi_flags_args a;
    std::memset(&a, 0, sizeof(a));
    a.cell_sums = d_cell_sums;
    a.zero_dm = d_zero_dm;
    a.cell_flags = d_cell_flags;
    a.channel_mask = d_channel_mask;
    a.spectrum_flags = d_spectrum_flags;
    a.counts = d_counts;
    a.mean_thr = thr->mean_thr;
    a.mean_floor = thr->mean_floor;
    a.var_thr = thr->var_thr;
    a.var_floor = thr->var_floor;
    a.zero_dm_thr = thr->zero_dm_thr;
    a.zero_dm_floor = thr->zero_dm_floor;
    a.C = C;
    a.B = nr_beams;
    a.nr_blocks = nr_blocks;
    a.block_len = block_len;
    a.max_bad_blocks = thr->max_bad_blocks;
    return (int)bf_launch_rfi_flags(a, as_stream(stream));
}

int rfi_clean_q8_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra, uint64_t first_spectrum,
                      uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const uint8_t *d_cell_flags, const uint8_t *d_channel_mask,
                      const uint8_t *d_spectrum_flags, uint8_t fill, uint8_t *d_out, size_t out_bytes, uint64_t out_spectra,
                      uint64_t first_out, unsigned long long *d_replaced, void *stream)
{
    if (int e = rfi_clean_q8_args(c, d_filterbank, in_spectra, first_spectrum, nr_blocks, block_len, nr_beams, d_out, out_spectra, first_out,
                                  d_replaced))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(filterbank_bytes, nr_beams, in_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(out_bytes, nr_beams, out_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_rfi_clean_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_filterbank;
    a.out = d_out;
    a.cell_flags = d_cell_flags;
    a.channel_mask = d_channel_mask;
    a.spectrum_flags = d_spectrum_flags;
    a.replaced = d_replaced;
    a.in_spectra = in_spectra;
    a.first = first_spectrum;
    a.out_spectra = out_spectra;
    a.first_out = first_out;
    a.C = C;
    a.B = nr_beams;
    a.nr_blocks = nr_blocks;
    a.block_len = block_len;
    a.fill = fill;
    return (int)bf_launch_rfi_clean(a, as_stream(stream));
}

} // namespace bf_host
