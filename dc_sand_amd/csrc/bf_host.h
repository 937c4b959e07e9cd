// bf_host.h -- what the host units of the C-ABI share (bf_capi*.hip): the context, the status macros, and the few
// functions that cross from one unit to another.  Internal, like bf_ctx_ext.h: never installed, never included by a
// companion.  What a unit does not find here belongs to another unit alone.
#ifndef BF_HOST_H
#define BF_HOST_H

#include "../../include/dcs_beamformer.h"
#ifdef DCS_PROBES
#include "../../include/dcs_probes.h" // the probes build: struct dcs_probe_knobs, dcs_probe_set_knobs
#endif

#include <hip/hip_runtime.h>

#include <cstring>

#include "bf_kernels.h"
#include "bf_ctx_ext.h"

#define DCS_TRY(expr)                          \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) return (int)_e;  \
    } while (0)

constexpr uint32_t kDtSlotFloats = 4096; // time steps per tiled launch
constexpr int kDtSlots = 8;

// A context's buffers and launches belong to the device that was current at dcs_bf_create.
#define DCS_CHECK_DEVICE(c)                                                \
    do {                                                                   \
        int _cur = -1;                                                     \
        if (hipGetDevice(&_cur) != hipSuccess || _cur != (c)->device) return DCS_ERR_WRONG_DEVICE; \
    } while (0)

constexpr int kSideStreams = 4;
struct dcs_bf_context {
    bf_ctx_ext_head ext; // FIRST: the weighted beamformer calls of the companion library reach this library's through it
    dcs_bf_params p;
    dcs_bf_consts k;
    uint32_t n_pairs;
    int device;
    uint32_t div3_verified; // what verify_div3 found for this context's divisor
    bool tuning_now;        // inside dcs_bf_autotune: launch the tuner-tagged kernel symbols
    dcs_delay_vals *d_table[2]; // double-buffered compact table
    int cur;                    // buffer generate reads
    bool table_set;
    float *d_dt;                // kDtSlots * kDtSlotFloats
    float *h_dt;                // pinned mirror
    hipEvent_t dt_ev[kDtSlots];
    // per-time-step launch loops (NAIVE, MULTIPLE_CHANNELS): independent launches, spread over side streams between a
    // fork and a join on the caller's stream
    hipStream_t side[kSideStreams];
    hipEvent_t fork_ev, join_ev[kSideStreams];
    bool dt_used[kDtSlots];
    int dt_next;
    // row-streaming form: per-(time step, pair) terms table + slow-path flags
    uint32_t pairs_pad;     // n_pairs rounded up to 256
    uint32_t terms_steps;   // time steps the table holds
    float *d_terms;         // [terms_steps][pairs_pad][2]; allocated on first use (ensure_terms)
    uint32_t *d_flags;      // [terms_steps][pairs_pad/64]
    uint32_t flag_epoch;    // the beamformers' class words are tagged with the call's number instead of being zeroed per call ...
    bool flags_cleared;     // ... until a beamformer call of this context is captured: from then on every call zeroes its words (clear_class_words)
    // per-input beam weights (include/dcs_beam_weights.h): what the weighted terms pre-pass makes from the caller's weights
    // for the beamformers; allocated on the first weighted call (ensure_weights)
    float *d_wnorm;         // [A][B]: ghat = g / s_b
    float *d_wscale;        // [B]: s_b
    // the terms-table variant of the tiled form (large launches of <= kTermsInline time steps): its own small
    // table, allocated with the context so that those launches stay capturable
    float *d_tt_terms;      // [kTermsInline][pairs_pad][2]
    uint32_t *d_tt_flags;   // [kTermsInline][pairs_pad/64]
    dcs_bf_tuning tune;     // the caller's explicit knobs (dcs_bf_set_tuning); 0 / -1 = not set
    // what dcs_bf_autotune measured for this context's shape, per KERNEL: [0] = fp32, [1] = fp16 from the fp32-grade
    // arithmetic, [2] = fp16 from the b16 arithmetic form (math_mode bit 2), each x {terms computed by every workgroup,
    // terms from the pre-pass table} -- different kernels with different optima (round 2 kept one result per output width and
    // ran a 1.2 GB streaming slab, which takes the first variant, at the geometry tuned for the 16 GiB launch, which takes
    // the second: 6.2 instead of 6.9 TB/s); used for large launches wherever the caller has not set a knob explicitly
    struct tuned_geom {
        bool valid;
        int32_t tpb, cpb, wpc; // wpc: -1 = unlimited
    } tuned[3][2];
#ifdef DCS_PROBES
    dcs_probe_knobs probe;  // measurement knobs (include/dcs_probes.h); the product build has no such member
#endif
};
// a measurement knob of the probes build; a constant 0 in the product
#ifdef DCS_PROBES
#define DCS_PROBE_KNOB(c, f) ((c)->probe.f)
#else
#define DCS_PROBE_KNOB(c, f) 0
#endif

namespace bf_host {

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Launch geometry of the tiled form, as pick_geometry decides it (bf_capi_generate.hip)
struct bf_geom {
    int tpb;
    uint32_t cpb;
    int wpc; // 0 = unlimited
    bool ntstore;
};

// Where a call's fDeltaTime values come from: the verifier's recipe for time indices
// [t0, t0 + nt) (dcs_bf_delta_times), or the caller's own values (dcs_bf_generate_dt / _at).
struct dt_source {
    const float *values; // nullptr: derive from the time index
    uint64_t t0;
};
// the calls behind bf_ctx_ext_ops take both: the caller's values where there are any, else the time index
inline dt_source dt_or_index(const float *dt, uint64_t t) { return dt_source{dt, dt ? 0 : t}; }

// bf_capi.hip
int refuse_if_capturing(hipStream_t stream);

// bf_capi_generate.hip: the tiled form's geometry and launch description (the context's warm-up and the streams' graph
// nodes are made from them), and a call's fDeltaTime values (the beamformers take theirs the same way)
bool want_terms_table(const dcs_bf_context *c, bool out16, const bf_geom &g, uint32_t nc, uint32_t nt);
bf_geom pick_geometry(const dcs_bf_context *c, bool out16, uint32_t nc, uint32_t nt);
int prepare_tiled(dcs_bf_context *c, bool out16, const float *dt_dev, float dt0, uint32_t nt, uint32_t c0, uint32_t nc, void *d_out,
                  bf_kernel_launch *l, const float *dt_host = nullptr, bool terms_table = false);
void fill_terms_table_args(const dcs_bf_context *c, bool out16, float dt0, uint32_t nt, uint32_t c0, uint32_t nc, void *d_out,
                           const float *dt_host, bf_terms_args *ta);
int fill_dt(const dcs_bf_context *c, const dt_source &src, uint32_t off, uint32_t n, float *dst);
int check_dt_range(const dcs_bf_context *c, const dt_source &src, uint32_t nt);
int stage_dt(dcs_bf_context *c, const dt_source &src, uint32_t off, uint32_t n, hipStream_t stream, const float **dt_dev);

// bf_capi_beamform.hip: the terms table and class words (the generator's rows form writes the same table)
int ensure_terms(dcs_bf_context *c, hipStream_t stream);

// the calls behind bf_ctx_ext_ops, in the table's order: four in bf_capi_beamform.hip, six in bf_capi_detect.hip, the
// complex product's three in bf_capi_beamform.hip again, and the Stokes detection's two, the dedispersion's two, the
// single-pulse search's three, the correlator's two and the down-converter's two in bf_capi_detect.hip
int generate_and_beamform_weighted_impl(dcs_bf_context *c, const float *dt, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                        size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                        void *stream);
int beamform_accumulated_weighted_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                       const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, float *d_beams,
                                       size_t beams_bytes, void *stream);
int beamform_accumulated_q8_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                 size_t antenna_bytes, const float *d_weights, const float *d_quant_gains, int8_t *d_beams_q8,
                                 size_t beams_bytes, unsigned long long *d_clip_count, void *stream);
int beamform_accumulated_power_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                    size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                    void *stream);
int integrate_block_power_impl(dcs_bf_context *c, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                               uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes, void *stream);
int incoherent_block_power_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                uint32_t *d_block_power, size_t power_bytes, void *stream);
int integrate_incoherent_power_impl(dcs_bf_context *c, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                    uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                    void *stream);
int spectra_sums_impl(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                      uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream);
int filterbank_scales_impl(dcs_bf_context *c, const double *d_sums, size_t sums_bytes, uint64_t count, uint32_t nr_beams,
                           float target_std, float *d_scales, size_t scales_bytes, void *stream);
int filterbank_q8_impl(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                       const float *d_scales, float level, uint32_t flags, uint8_t *d_filterbank, size_t filterbank_bytes,
                       uint64_t out_spectra, uint64_t first_spectrum, unsigned long long *d_clip_count, void *stream);
int beamform_accumulated_complex_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                      size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams, size_t beams_bytes,
                                      void *stream);
int beamform_accumulated_complex_power_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                            const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                            float *d_block_power, size_t power_bytes, void *stream);
int beamform_accumulated_complex_q8_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                         const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                         const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                         unsigned long long *d_clip_count, void *stream);
int stokes_block_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                      uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream);
int integrate_stokes_impl(dcs_bf_context *c, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                          uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                          size_t spectra_bytes, void *stream);
int dm_delays_impl(dcs_bf_context *c, const dcs_bf_band *band, const double *d_dms, uint32_t nr_dm, int32_t *d_delays,
                   size_t delays_bytes, void *stream);
int dedisperse_q8_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                       uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays, uint32_t nr_dm,
                       uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t *d_dm_time, size_t dm_time_bytes,
                       uint64_t out_spectra, uint64_t first_out, void *stream);
int dm_time_sums_impl(dcs_bf_context *c, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                      uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, uint32_t accumulate,
                      uint64_t *d_sums, size_t sums_bytes, void *stream);
int boxcar_peaks_impl(dcs_bf_context *c, const uint32_t *d_dm_time, size_t dm_time_bytes, uint64_t plane_spectra,
                      uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths,
                      uint32_t nr_widths, uint32_t max_width, uint32_t block_len, uint32_t *d_peaks, size_t peaks_bytes,
                      uint64_t peak_blocks, uint64_t first_block, void *stream);
int peak_snr_impl(dcs_bf_context *c, const uint32_t *d_peaks, size_t peaks_bytes, uint64_t peak_blocks, uint64_t first_block,
                  uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm, const uint32_t *d_widths, uint32_t nr_widths,
                  uint32_t max_width, const uint64_t *d_sums, size_t sums_bytes, uint64_t count, float *d_snr, size_t snr_bytes,
                  uint32_t *d_best, size_t best_bytes, void *stream);
int correlate_block_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, uint32_t blocks_per_vis,
                         int32_t *d_vis, size_t vis_bytes, void *stream);
int integrate_visibilities_impl(dcs_bf_context *c, const int32_t *d_vis, size_t vis_bytes, uint32_t nr_vis,
                                uint32_t vis_per_integration, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream);
int ddc_tap_digits_impl(dcs_bf_context *c, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, void *d_digits,
                        size_t digits_bytes, void *stream);
int ddc_impl(dcs_bf_context *c, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes, uint64_t in_stride,
             const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands, const dcs_ddc_band *bands,
             uint64_t first_output, float *d_out, size_t out_bytes, uint64_t out_stride, void *stream);
int find_candidates_impl(dcs_bf_context *c, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                         uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                         uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, void *d_cands,
                         size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes, void *stream);
int channelise_impl(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                    size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order, float *d_out,
                    size_t out_bytes, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs, uint32_t first_input, void *stream);
int channelise_q8_impl(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                       const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order,
                       const float *d_gains, int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks, uint64_t first_block,
                       uint32_t out_inputs, uint32_t first_input, unsigned long long *d_clip_count, void *stream);
int rfi_moments_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra, uint64_t first_spectrum,
                     uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, uint32_t *d_cell_sums, size_t cell_sums_bytes,
                     uint32_t *d_zero_dm, size_t zero_dm_bytes, void *stream);
int rfi_flags_impl(dcs_bf_context *c, const uint32_t *d_cell_sums, size_t cell_sums_bytes, const uint32_t *d_zero_dm, size_t zero_dm_bytes,
                   uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const dcs_bf_rfi_thresholds *thr, uint8_t *d_cell_flags,
                   size_t cell_flags_bytes, uint8_t *d_channel_mask, size_t channel_mask_bytes, uint8_t *d_spectrum_flags,
                   size_t spectrum_flags_bytes, uint32_t *d_counts, size_t counts_bytes, void *stream);
int rfi_clean_q8_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra, uint64_t first_spectrum,
                      uint32_t nr_blocks, uint32_t block_len, uint32_t nr_beams, const uint8_t *d_cell_flags, const uint8_t *d_channel_mask,
                      const uint8_t *d_spectrum_flags, uint8_t fill, uint8_t *d_out, size_t out_bytes, uint64_t out_spectra,
                      uint64_t first_out, unsigned long long *d_replaced, void *stream);

} // namespace bf_host

#endif // BF_HOST_H
