// bf_host.h -- what the units with host code of the C-ABI share (bf_capi*.hip, and the stage units that carry their own host
// side behind the table of bf_ctx_ext.h): the context, the status macros, and the few functions that cross from one unit to
// another.  Internal, like bf_ctx_ext.h: never installed, never included by a companion.  What a unit does not find here
// belongs to another unit alone.
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

// the words that integrate_blocks sums (bf_integrate.hip, whose launcher takes the same type)
enum bf_integrate_type { BF_INTEGRATE_F32, BF_INTEGRATE_U32 /* built for bs == 1 */, BF_INTEGRATE_I32 };

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

// bf_integrate.hip: the one integration behind the four integrate_* entries, which live with their stages
int integrate_blocks(dcs_bf_context *c, bf_integrate_type type, const void *d_blocks, size_t blocks_bytes, uint64_t bs,
                     uint32_t nr_blocks, uint32_t n, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream);

// the calls behind bf_ctx_ext_ops, in the table's order.  The seven beamformer calls are in bf_capi_beamform.hip, written out
// as the table writes them; every other one is at the end of its stage's kernel unit and takes its type from the public
// declaration, as its table entry does: one line per stage, the unit's name behind it
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
decltype(dcs_bf_integrate_block_power) integrate_block_power_impl;           // bf_integrate.hip
decltype(dcs_bf_incoherent_block_power) incoherent_block_power_impl;         // bf_incoherent.hip
decltype(dcs_bf_integrate_incoherent_power) integrate_incoherent_power_impl;
decltype(dcs_bf_spectra_sums) spectra_sums_impl;                             // bf_filterbank.hip
decltype(dcs_bf_filterbank_scales) filterbank_scales_impl;
decltype(dcs_bf_filterbank_q8) filterbank_q8_impl;
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
decltype(dcs_bf_stokes_block) stokes_block_impl;                             // bf_stokes.hip
decltype(dcs_bf_integrate_stokes) integrate_stokes_impl;
decltype(dcs_bf_dm_delays) dm_delays_impl;                                   // bf_dedisperse.hip
decltype(dcs_bf_dedisperse_q8) dedisperse_q8_impl;
decltype(dcs_bf_dm_time_sums) dm_time_sums_impl;                             // bf_single_pulse.hip
decltype(dcs_bf_boxcar_peaks) boxcar_peaks_impl;
decltype(dcs_bf_peak_snr) peak_snr_impl;
decltype(dcs_bf_correlate_block) correlate_block_impl;                       // bf_correlator.hip
decltype(dcs_bf_integrate_visibilities) integrate_visibilities_impl;
decltype(dcs_bf_ddc_tap_digits) ddc_tap_digits_impl;                         // bf_ddc.hip
decltype(dcs_bf_ddc) ddc_impl;
int find_candidates_impl(dcs_bf_context *c, const float *d_snr, size_t snr_bytes, const uint32_t *d_peaks, size_t peaks_bytes,
                         uint64_t peak_blocks, uint64_t first_block, uint32_t nr_blocks, uint32_t nr_beams, uint32_t nr_dm,
                         uint32_t nr_widths, float threshold, uint32_t dm_radius, uint32_t block_radius, void *d_cands,
                         size_t cands_bytes, uint32_t max_candidates, uint32_t *d_count, void *d_work, size_t work_bytes,
                         void *stream); // bf_candidates.hip; written out, as the table's entry is
decltype(dcs_bf_channelise) channelise_impl;                                 // bf_channeliser.hip
decltype(dcs_bf_channelise_q8) channelise_q8_impl;
decltype(dcs_bf_rfi_moments) rfi_moments_impl;                               // bf_rfi.hip
decltype(dcs_bf_rfi_flags) rfi_flags_impl;
decltype(dcs_bf_rfi_clean_q8) rfi_clean_q8_impl;
decltype(dcs_bf_fold_q8) fold_q8_impl;                                       // bf_fold.hip
decltype(dcs_bf_fold_scrunch) fold_scrunch_impl;

} // namespace bf_host

#endif // BF_HOST_H
