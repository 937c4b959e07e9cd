// bf_capi.hip -- implementation of include/dcs_beamformer.h (the C-ABI).
// Host code only; the kernels are in bf_kernels.hip.  Nothing here exits,
// throws across the boundary, prints, or starts threads.

#include "../../include/dcs_beamformer.h"
#ifdef DCS_PROBES
#include "../../include/dcs_probes.h" // the probes build: struct dcs_probe_knobs, dcs_probe_set_knobs
#endif

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/dcs_stream_staging.h" // DCS_BF_STAGE_CALLER_PINNED
#include "bf_kernels.h"
#include "bf_ctx_ext.h"
#include "bf_stream_ext.h"

static_assert(sizeof(dcs_delay_vals) == 16, "delay_vals must be 4 x fp32 (BeamformerParameters.h:61-66)");

#define DCS_TRY(expr)                          \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) return (int)_e;  \
    } while (0)

namespace {

constexpr uint32_t kDtSlotFloats = 4096; // time steps per tiled launch
constexpr int kDtSlots = 8;

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// A context's buffers and launches belong to the device that was current at dcs_bf_create.
#define DCS_CHECK_DEVICE(c)                                                \
    do {                                                                   \
        int _cur = -1;                                                     \
        if (hipGetDevice(&_cur) != hipSuccess || _cur != (c)->device) return DCS_ERR_WRONG_DEVICE; \
    } while (0)

bool params_ok(const dcs_bf_params *p)
{
    if (!p) return false;
    if (p->nr_channels < 1 || p->nr_channels > (1 << 24)) return false; // (float)c must be exact
    if (p->nr_stations < 1 || p->nr_beams < 1) return false;
    if ((uint64_t)p->nr_stations * (uint64_t)p->nr_beams > 0x7fffffffull) return false;
    if (!(p->sampling_period > 0.0f) || !std::isfinite(p->sampling_period)) return false;
    if (p->fft_size < 1) return false;
    // dcs_bf_gpu_utilisation divides by both (BeamformerCoefficientTest.cu:426-429)
    if (p->nr_samples_per_channel < 1 || p->accumulations_before_new_coeffs < 1) return false;
    if (!(p->adc_sample_rate > 0.0) || !std::isfinite(p->adc_sample_rate)) return false;
    const float D = p->sampling_period * (float)p->nr_channels;
    if (!(D >= 0x1p-40f && D <= 0x1p40f)) return false; // dcs_div_const's proven range
    return true;
}

dcs_bf_consts make_consts(const dcs_bf_params *p)
{
    dcs_bf_consts k;
    // BeamformerCoefficientTest.cu:322  (SAMPLING_PERIOD*NR_CHANNELS): fp32 * int->fp32
    volatile float D = p->sampling_period * (float)p->nr_channels;
    volatile float y = 1.0f / D; // one IEEE fp32 divide
    k.fDenominator = D;
    k.fRcpDenominator = y;
    // |fDelayN| <= |rate| * (C-1) * pi / D * (1 + 3*2^-24); keep a 1e-4 margin.
    const double scale = (double)(p->nr_channels - 1) * 3.14159274101257324219 / (double)D;
    k.fRotBoundScale = (float)(scale * 1.0001) ;
    if (!(k.fRotBoundScale >= 0.0f)) k.fRotBoundScale = INFINITY;
    k.uDiv3Exact = 0u; // set by verify_div3() once a device is at hand
    k.fLowDegLimit = 500.0f;
    k.uHalfMath = 0u;
    k.dHalfChannels = p->nr_channels / 2.0; // BeamformerCoefficientTest.cu:323
    k.dDenominator = (double)D;
    return k;
}

// Is the 3-op divide exact for this launch constant?  All 2^23 significands of one
// binade on the device against the IEEE divide (bf_math.h: scale invariance).
int verify_div3(dcs_bf_consts *k)
{
    uint32_t *d_cnt = nullptr;
    uint32_t h_cnt = 1;
    hipError_t e = hipMalloc((void **)&d_cnt, sizeof(uint32_t));
    if (e != hipSuccess) return (int)e;
    e = hipMemset(d_cnt, 0, sizeof(uint32_t));
    if (e == hipSuccess) e = bf_launch_verify_div3(k->fDenominator, k->fRcpDenominator, d_cnt, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&h_cnt, d_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_cnt);
    if (e != hipSuccess) return (int)e;
    k->uDiv3Exact = (h_cnt == 0u) ? 1u : 0u;
    return DCS_OK;
}

} // namespace

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

constexpr int kTableRing = 4;
struct dcs_bf_stream {
    bf_stream_ext_head ext; // FIRST: the staging calls of the companion library reach this library's through it
    dcs_bf_context *ctx;
    hipStream_t stream;
    hipGraph_t graph;
    hipGraphExec_t exec;
    hipGraphNode_t node;
    bf_kernel_launch launch;     // the node's kernel, geometry and arguments
    // slabs of >= 1 GiB take the tiled form's terms-table variant: a second kernel node in front (the pre-pass)
    bool has_terms;
    hipGraphNode_t terms_node;
    bf_terms_args terms_args;
    const void *terms_func;
    dim3 terms_grid, terms_block;
    // host table updates: a ring of pinned staging buffers, so that a tick only blocks the host when kTableRing
    // updates are still in flight (a table landing on every tick never waits: the copy of tick k - 4 is long done)
    dcs_delay_vals *h_table[kTableRing];
    hipEvent_t table_copied[kTableRing]; // h_table[i] may be rewritten after this
    bool table_pending[kTableRing];
    int table_next;
    // device table updates (dcs_bf_stream_tick_*_from_global): a second instantiated graph with the slice gather
    // (bf_gather_beams_kernel) in front of the same nodes
    hipGraph_t ggraph;
    hipGraphExec_t gexec;
    hipGraphNode_t gnode_gather, gnode_terms, gnode_gen;
    bf_gather_launch gather;
    // staged tables (dcs_bf_stream_stage_table*): the stream owns a THIRD table buffer, filled on an internal stream
    // while the caller's stream runs; the consuming tick exchanges it with the context's current buffer, so the one it
    // retires is read only by work queued before that tick (released_ev marks the point).  Created on first staging.
    dcs_delay_vals *d_spare;
    hipStream_t stage_stream; // non-blocking, highest priority: its own hardware queue, not behind the generator
    hipEvent_t staged_ev;     // the staging copy / gather into d_spare has landed
    hipEvent_t released_ev;   // recorded on the caller's stream in front of the last consuming tick
    bool released_recorded;
    bool staged;              // d_spare holds a table the next plain tick makes current
};

extern "C" {

const char *dcs_error_string(int status)
{
    switch (status) {
    case DCS_OK: return "dcs: success";
    case DCS_ERR_INVALID_ARGUMENT: return "dcs error: invalid argument";
    case DCS_ERR_UNSUPPORTED: return "dcs error: this kernel does not support the requested mode";
    case DCS_ERR_NOT_READY: return "dcs error: not ready (no delay table set)";
    case DCS_ERR_OUT_OF_RANGE: return "dcs error: out of range";
    case DCS_ERR_NO_DEVICE: return "dcs error: no HIP device";
    case DCS_ERR_WRONG_DEVICE: return "dcs error: the context belongs to another device than the current one (dcs_device_set)";
    default: break;
    }
    if (status > 0) return hipGetErrorString((hipError_t)status);
    return "dcs error: unknown status";
}

int dcs_abi_version(void) { return DCS_BF_ABI_VERSION; }

int dcs_bf_default_params(dcs_bf_params *p)
{
    if (!p) return DCS_ERR_INVALID_ARGUMENT;
    // BeamformerParameters.h:7-17
    p->nr_channels = 64;
    p->nr_stations = 64;
    p->nr_beams = 16;
    p->nr_samples_per_channel = 256;
    p->sampling_period = 1e-7f;
    p->fft_size = 8192;
    p->adc_sample_rate = 1712e6;
    p->accumulations_before_new_coeffs = 256;
    p->reserved = 0;
    return DCS_OK;
}

int dcs_bf_output_bytes(const dcs_bf_params *p, int bitwidth, uint32_t nt, size_t *bytes)
{
    if (!params_ok(p) || !bytes) return DCS_ERR_INVALID_ARGUMENT;
    if (bitwidth != DCS_BF_B16 && bitwidth != DCS_BF_B32) return DCS_ERR_INVALID_ARGUMENT;
    // BeamformerCoefficientTest.cu:32-38
    const size_t elem = bitwidth == DCS_BF_B16 ? sizeof(uint16_t) : sizeof(float);
    *bytes = (size_t)nt * (size_t)p->nr_channels * (size_t)p->nr_stations * (size_t)p->nr_beams * 2u * elem;
    return DCS_OK;
}

int dcs_bf_delta_times(const dcs_bf_params *p, uint64_t t0, uint32_t nt, float *dt_out)
{
    if (!params_ok(p) || (!dt_out && nt)) return DCS_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < nt; i++) {
        const uint64_t t = t0 + i;
        // BeamformerCoefficientTest.cu:299: long timeStep = t*SAMPLING_PERIOD*1e9f*FFT_SIZE;
        // size_t -> float, three fp32 products left to right, truncation.
        volatile float a = (float)t;
        volatile float b = a * p->sampling_period;
        volatile float c = b * 1e9f;
        volatile float d = c * (float)p->fft_size;
        if (!(d < 9.2e18f)) return DCS_ERR_OUT_OF_RANGE;
        const long step_ns = (long)d;
        // ts_diff(ref, ref + step): (float)sec - (float)sec == 0, then
        // += (float)nanosec_difference / 1e9f   (BeamformerCoefficientTest.cu:14-16)
        volatile float num = (float)step_ns;
        volatile float q = num / 1e9f;
        volatile float dt = 0.0f + q;
        dt_out[i] = dt;
    }
    return DCS_OK;
}

int dcs_bf_ts_diff(const struct timespec *first, const struct timespec *last, float *dt_out)
{
    if (!first || !last || !dt_out) return DCS_ERR_INVALID_ARGUMENT;
    // BeamformerCoefficientTest.cu:12-18, operation by operation (fp32, one rounding each):
    //   float time_difference = (float)last.tv_sec - (float)first.tv_sec;
    //   long nanosec_difference = last.tv_nsec - first.tv_nsec;
    //   time_difference += (float)nanosec_difference / 1e9f;
    volatile float fl = (float)last->tv_sec, ff = (float)first->tv_sec;
    volatile float secs = fl - ff;
    const long nanosec_difference = last->tv_nsec - first->tv_nsec;
    volatile float num = (float)nanosec_difference;
    volatile float q = num / 1e9f;
    volatile float dt = secs + q;
    *dt_out = dt;
    return DCS_OK;
}

int dcs_bf_simulate_input(const dcs_bf_params *p, dcs_delay_vals *out)
{
    if (!params_ok(p) || !out) return DCS_ERR_INVALID_ARGUMENT;
    // BeamformerCoefficientTest.cu:185-196
    const size_t n = (size_t)p->nr_stations * (size_t)p->nr_beams;
    for (size_t i = 0; i < n; i++) {
        volatile float ratio = (float)i / (float)n;
        volatile float ramp = ratio * p->sampling_period;
        out[i].fDelay_s = (float)((double)ramp / 3.0);
        out[i].fDelayRate_sps = (float)2e-6;
        volatile float inv = 1.0f - ratio;
        volatile float ramp2 = inv * p->sampling_period;
        out[i].fPhase_rad = (float)((double)ramp2 / 3.0);
        out[i].fPhaseRate_radps = (float)3e-6;
    }
    return DCS_OK;
}

/* ---- device plumbing ---------------------------------------------------- */
int dcs_device_count(int *count)
{
    if (!count) return DCS_ERR_INVALID_ARGUMENT;
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e == hipErrorNoDevice) { *count = 0; return DCS_OK; }
    return (int)e;
}
int dcs_device_set(int device) { return (int)hipSetDevice(device); }
int dcs_device_synchronize(void) { return (int)hipDeviceSynchronize(); }
int dcs_device_name(int device, char *buf, size_t buflen)
{
    if (!buf || buflen == 0) return DCS_ERR_INVALID_ARGUMENT;
    hipDeviceProp_t prop;
    DCS_TRY(hipGetDeviceProperties(&prop, device));
    std::snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return DCS_OK;
}
int dcs_malloc(void **dptr, size_t bytes)
{
    if (!dptr) return DCS_ERR_INVALID_ARGUMENT;
    return (int)hipMalloc(dptr, bytes);
}
int dcs_free(void *dptr) { return (int)hipFree(dptr); }
int dcs_host_alloc(void **hptr, size_t bytes)
{
    if (!hptr) return DCS_ERR_INVALID_ARGUMENT;
    return (int)hipHostMalloc(hptr, bytes, hipHostMallocDefault);
}
int dcs_host_free(void *hptr) { return (int)hipHostFree(hptr); }
int dcs_memcpy_htod(void *dptr, const void *hptr, size_t bytes, void *stream)
{
    return (int)hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, as_stream(stream));
}
int dcs_memcpy_dtoh(void *hptr, const void *dptr, size_t bytes, void *stream)
{
    return (int)hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, as_stream(stream));
}
int dcs_memcpy_dtod(void *dst, const void *src, size_t bytes, void *stream)
{
    return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream));
}
int dcs_memcpy2d_dtoh(void *hptr, size_t dst_pitch, const void *dptr, size_t src_pitch, size_t row_bytes,
                      size_t nrows, void *stream)
{
    return (int)hipMemcpy2DAsync(hptr, dst_pitch, dptr, src_pitch, row_bytes, nrows, hipMemcpyDeviceToHost,
                                 as_stream(stream));
}
int dcs_memset(void *dptr, int value, size_t bytes, void *stream)
{
    return (int)hipMemsetAsync(dptr, value, bytes, as_stream(stream));
}
int dcs_stream_create(void **stream)
{
    if (!stream) return DCS_ERR_INVALID_ARGUMENT;
    hipStream_t s;
    DCS_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return DCS_OK;
}
int dcs_stream_destroy(void *stream) { return (int)hipStreamDestroy(as_stream(stream)); }
int dcs_stream_synchronize(void *stream) { return (int)hipStreamSynchronize(as_stream(stream)); }

int dcs_event_create(void **event)
{
    if (!event) return DCS_ERR_INVALID_ARGUMENT;
    hipEvent_t e;
    DCS_TRY(hipEventCreate(&e));
    *event = e;
    return DCS_OK;
}
int dcs_event_destroy(void *event) { return (int)hipEventDestroy(reinterpret_cast<hipEvent_t>(event)); }
int dcs_event_record(void *event, void *stream)
{
    return (int)hipEventRecord(reinterpret_cast<hipEvent_t>(event), as_stream(stream));
}
int dcs_event_synchronize(void *event) { return (int)hipEventSynchronize(reinterpret_cast<hipEvent_t>(event)); }
int dcs_event_elapsed_ms(void *start, void *stop, float *ms)
{
    if (!ms) return DCS_ERR_INVALID_ARGUMENT;
    return (int)hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start), reinterpret_cast<hipEvent_t>(stop));
}

/* ---- context ------------------------------------------------------------ */
namespace {
int prepare_tiled(dcs_bf_context *c, bool out16, const float *dt_dev, float dt0, uint32_t nt, uint32_t c0, uint32_t nc, void *d_out,
                  bf_kernel_launch *l, const float *dt_host, bool terms_table);
// the weighted beamformer calls (bf_ctx_ext.h; defined with the beamformers below)
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
const bf_ctx_ext_ops kWeightsOps = {BF_CTX_EXT_VERSION, generate_and_beamform_weighted_impl, beamform_accumulated_weighted_impl,
                                    beamform_accumulated_q8_impl, beamform_accumulated_power_impl, integrate_block_power_impl,
                                    incoherent_block_power_impl, integrate_incoherent_power_impl,
                                    spectra_sums_impl, filterbank_scales_impl, filterbank_q8_impl};
}

int dcs_bf_create(const dcs_bf_params *p, dcs_bf_context **out)
{
    if (!out) return DCS_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!params_ok(p)) return DCS_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return DCS_ERR_NO_DEVICE;
    dcs_bf_context *c = new (std::nothrow) dcs_bf_context();
    if (!c) return (int)hipErrorOutOfMemory;
    std::memset(c, 0, sizeof(*c));
    c->ext.ops = &kWeightsOps;
    c->p = *p;
    c->k = make_consts(p);
    c->n_pairs = (uint32_t)p->nr_stations * (uint32_t)p->nr_beams;
    c->pairs_pad = (c->n_pairs + 255u) & ~255u;
    {
        const uint64_t per_step = (uint64_t)c->pairs_pad * 8u;
        uint64_t steps = (64ull << 20) / per_step;
        if (steps < 1) steps = 1;
        if (steps > kDtSlotFloats) steps = kDtSlotFloats;
        c->terms_steps = (uint32_t)steps;
    }
    c->tune.nontemporal = -1;
    c->tune.xcd_remap = -1;
    c->tune.rows_same_tile = -1;
    int st = DCS_OK;
    do {
        if ((st = (int)hipGetDevice(&c->device)) != 0) break;
        if ((st = (int)bf_warm_module()) != 0) break; // load the kernels now, not in the first timed launch
        if ((st = (int)bf_warm_module_mfma()) != 0) break;
        if ((st = (int)bf_warm_module_incoherent()) != 0) break;
        if ((st = (int)bf_warm_module_filterbank()) != 0) break;
        const size_t tb = (size_t)c->n_pairs * sizeof(dcs_delay_vals);
        if ((st = (int)hipMalloc((void **)&c->d_table[0], tb)) != 0) break;
        if ((st = (int)hipMalloc((void **)&c->d_table[1], tb)) != 0) break;
        const size_t db = (size_t)kDtSlots * kDtSlotFloats * sizeof(float);
        if ((st = (int)hipMalloc((void **)&c->d_dt, db)) != 0) break;
        if ((st = (int)hipMalloc((void **)&c->d_tt_terms, (size_t)kTermsInline * c->pairs_pad * 8u)) != 0) break;
        if ((st = (int)hipMalloc((void **)&c->d_tt_flags, (size_t)kTermsInline * (c->pairs_pad / 64u) * 4u)) != 0) break;
        if ((st = (int)hipHostMalloc((void **)&c->h_dt, db, hipHostMallocDefault)) != 0) break;
        for (int i = 0; i < kDtSlots && st == 0; i++) st = (int)hipEventCreateWithFlags(&c->dt_ev[i], hipEventDisableTiming);
        if (st != 0) break;
        for (int i = 0; i < kSideStreams && st == 0; i++) {
            st = (int)hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking);
            if (st == 0) st = (int)hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming);
        }
        if (st == 0) st = (int)hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming);
        if (st != 0) break;
        // first use of the pinned->device copy path costs ~0.25 ms once: pay it here,
        // not inside the caller's first timed launch
        c->h_dt[0] = 0.0f;
        if ((st = (int)hipMemcpy(c->d_dt, c->h_dt, sizeof(float), hipMemcpyHostToDevice)) != 0) break;
        if ((st = verify_div3(&c->k)) != 0) break;
        c->div3_verified = c->k.uDiv3Exact;
        // the harness times ONE launch, the first: have the runtime set up the kernels that launch would use (the
        // whole tensor in one launch, either width) now
        for (int w = 0; w < 2; w++) {
            bf_kernel_launch l;
            const uint32_t nt_all = (uint32_t)(c->p.nr_samples_per_channel < (int)kDtInline ? c->p.nr_samples_per_channel : (int)kDtInline);
            float dts[kDtInline] = {0.0f};
            if (prepare_tiled(c, w == 1, nullptr, 0.0f, nt_all > 0 ? nt_all : 1u, 0, (uint32_t)c->p.nr_channels, nullptr, &l, dts, false) == DCS_OK && l.func) {
                hipFuncAttributes attr;
                (void)hipFuncGetAttributes(&attr, l.func);
            }
        }
    } while (0);
    if (st != 0) {
        dcs_bf_destroy(c);
        return st;
    }
    *out = c;
    return DCS_OK;
}

int dcs_bf_destroy(dcs_bf_context *c)
{
    if (!c) return DCS_OK;
    (void)hipFree(c->d_table[0]);
    (void)hipFree(c->d_table[1]);
    (void)hipFree(c->d_dt);
    (void)hipFree(c->d_terms);
    (void)hipFree(c->d_flags);
    (void)hipFree(c->d_wnorm);
    (void)hipFree(c->d_wscale);
    (void)hipFree(c->d_tt_terms);
    (void)hipFree(c->d_tt_flags);
    if (c->h_dt) (void)hipHostFree(c->h_dt);
    for (int i = 0; i < kDtSlots; i++)
        if (c->dt_ev[i]) (void)hipEventDestroy(c->dt_ev[i]);
    for (int i = 0; i < kSideStreams; i++) {
        if (c->join_ev[i]) (void)hipEventDestroy(c->join_ev[i]);
        if (c->side[i]) (void)hipStreamDestroy(c->side[i]);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    delete c;
    return DCS_OK;
}

int dcs_bf_upload_delays(dcs_bf_context *c, const dcs_delay_vals *table, void *stream)
{
    if (!c || !table) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    const int nxt = c->table_set ? (c->cur ^ 1) : c->cur;
    DCS_TRY(hipMemcpyAsync(c->d_table[nxt], table, (size_t)c->n_pairs * sizeof(dcs_delay_vals),
                           hipMemcpyHostToDevice, as_stream(stream)));
    c->cur = nxt;
    c->table_set = true;
    return DCS_OK;
}

int dcs_bf_set_delays_from_global(dcs_bf_context *c, const void *d_global, uint32_t nb_total,
                                  uint32_t beam_offset, void *stream)
{
    if (!c || !d_global) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if ((uint64_t)beam_offset + (uint64_t)c->p.nr_beams > nb_total) return DCS_ERR_OUT_OF_RANGE;
    if ((reinterpret_cast<uintptr_t>(d_global) & 15u) != 0) return DCS_ERR_INVALID_ARGUMENT;
    const int nxt = c->table_set ? (c->cur ^ 1) : c->cur;
    DCS_TRY(bf_launch_gather_beams(c->d_table[nxt], static_cast<const dcs_delay_vals *>(d_global),
                                   (uint32_t)c->p.nr_stations, (uint32_t)c->p.nr_beams, nb_total, beam_offset,
                                   as_stream(stream)));
    c->cur = nxt;
    c->table_set = true;
    return DCS_OK;
}

int dcs_bf_set_tuning(dcs_bf_context *c, const dcs_bf_tuning *t)
{
    if (!c) return DCS_ERR_INVALID_ARGUMENT;
    if (!t) { // back to the defaults
        std::memset(&c->tune, 0, sizeof(c->tune));
        c->tune.nontemporal = -1;
        c->tune.xcd_remap = -1;
        c->tune.rows_same_tile = -1;
        c->k.uDiv3Exact = c->div3_verified;
        c->k.fLowDegLimit = 500.0f;
        c->k.uHalfMath = 0u;
        std::memset(c->tuned, 0, sizeof(c->tuned)); // forget what dcs_bf_autotune measured, too
        return DCS_OK;
    }
    if (t->form < 0 || t->form > 3) return DCS_ERR_INVALID_ARGUMENT;
    if (t->nontemporal < -1 || t->nontemporal > 1) return DCS_ERR_INVALID_ARGUMENT;
    if (t->chan_per_block < 0 || t->chan_per_block > (1 << 24)) return DCS_ERR_INVALID_ARGUMENT;
    if (t->tiles_per_block != 0 && t->tiles_per_block != 1 && t->tiles_per_block != 2 && t->tiles_per_block != 4)
        return DCS_ERR_INVALID_ARGUMENT;
    if (t->waves_per_block != 0 && t->waves_per_block != 4 && t->waves_per_block != 8 && t->waves_per_block != 16)
        return DCS_ERR_INVALID_ARGUMENT;
    if (t->rows_per_wave < 0 || t->rows_per_wave > 4) return DCS_ERR_INVALID_ARGUMENT;
    if (t->rows_same_tile < -1 || t->rows_same_tile > 1) return DCS_ERR_INVALID_ARGUMENT;
    if (t->xcd_remap < -1 || t->xcd_remap > 1) return DCS_ERR_INVALID_ARGUMENT;
    if (t->math_mode < 0 || t->math_mode > 15) return DCS_ERR_INVALID_ARGUMENT;
    if ((t->math_mode & 4) && t->nontemporal == 0) return DCS_ERR_UNSUPPORTED; // the b16 arithmetic form exists with nontemporal stores only
    if (t->wg_per_cu < -1 || t->wg_per_cu == 1 || t->wg_per_cu > 7) return DCS_ERR_INVALID_ARGUMENT;
    c->tune = *t;
    // math_mode bit 0: keep the 5-op divide; bit 1: keep the full polynomials
    c->k.uDiv3Exact = (t->math_mode & 1) ? 0u : c->div3_verified;
    c->k.fLowDegLimit = (t->math_mode & 2) ? 0.0f : 500.0f;
    // bit 2: b16 output uses the binary16-sized sincos (tiled form, waves outside the slow class)
    c->k.uHalfMath = (t->math_mode & 4) ? 1u : 0u;
    return DCS_OK;
}

namespace {

// Launch geometry of the tiled form for ONE launch of nt time steps x nc channels (DESIGN.md "launch
// geometry"; measured on MI355X: profiles/r01_geometry_sweep.md, profiles/r02_autotune.md).  The write
// rate the HBM system sustains falls with the number of stores a wave issues before it retires, so the
// fp32 walk is kept SHORT; the optimum is flat within ~2 % around these points for every shape swept:
//   fp32, plenty of work: 1 tile x 12 channels per workgroup (3 stores per wave), at most 6 workgroups per CU;
//   fp32, rows of >= 2048 tiles (>= 2 MiB: one row outlasts the resident workgroups): 10 channels, no limit;
//   fp32, <= 32 MiB of output in > 1024 workgroups (launch-bound): 2 tiles x 16 channels (fewer, fatter workgroups);
//   fp16 (VALU-bound): 1 tile x 128 channels to amortise the per-workgroup set-up, halved while that
//         leaves the chip fewer than 2048 workgroups (down to 16);
//   any launch whose workgroups are all resident at once (<= 8 per CU): no residency limit -- the unused
//         dynamic LDS behind it costs a small launch 1-2 us and buys nothing there.
// Order of precedence per knob: the caller's explicit dcs_bf_set_tuning value, then (large launches
// only) what dcs_bf_autotune measured for this context, then the rule above.
struct bf_geom {
    int tpb;
    uint32_t cpb;
    int wpc; // 0 = unlimited
    bool ntstore;
};

uint64_t tiled_blocks(uint32_t n_pairs, bool out16, int tpb, uint32_t cpb, uint32_t nc, uint32_t nt)
{
    const uint32_t ppb = 64u * (out16 ? 4u : 2u) * (uint32_t)tpb;
    return (uint64_t)((n_pairs + ppb - 1) / ppb) * ((nc + cpb - 1) / cpb) * nt;
}

// Large launches of the tiled form read their pairs' terms from a table written by a pre-pass kernel instead
// of computing them in every workgroup (bf_kernels.hip, TERMS): form 0 decides by size, form 1 never, form 3 always.
bool want_terms_table(const dcs_bf_context *c, bool out16, const bf_geom &g, uint32_t nc, uint32_t nt)
{
    if (DCS_PROBE_KNOB(c, nomath) || !g.ntstore || nt > kTermsInline) return false;
    if (c->tune.form == 3) return true;
    if (c->tune.form != 0) return false;
    // the pre-pass is one more kernel (~2 us) and kernel boundary (~1.5 us) per call and buys 2-4 % of the main
    // kernel's time: it breaks even at 1-2 GiB of output per launch (64 x 64 x 4096, 128 MiB in 21 us, lost 8 %
    // to it; the 1.3 GB slab of a 200 us streaming tick lost 2 %; 64 x 256 x 8192, 1 GiB, was level)
    const uint64_t bytes = (uint64_t)nt * nc * c->n_pairs * (out16 ? 4u : 8u);
    return bytes >= (2ull << 30) && tiled_blocks(c->n_pairs, out16, g.tpb, g.cpb, nc, nt) > 256u * 8u;
}

bf_geom shape_default_geometry(const dcs_bf_context *c, bool out16, uint32_t nc, uint32_t nt)
{
    constexpr uint64_t kResident = 256u * 8u; // workgroups of 256 threads the chip holds at once
    bf_geom g;
    g.ntstore = c->tune.nontemporal < 0 ? true : c->tune.nontemporal != 0;
    g.tpb = 1;
    const bool half = out16 && c->k.uHalfMath != 0u;
    if (out16) {
        g.cpb = 128u;
        g.wpc = 0;
        while (g.cpb > 16u && tiled_blocks(c->n_pairs, true, 1, g.cpb, nc, nt) < kResident) g.cpb >>= 1;
    } else {
        g.cpb = 12u;
        g.wpc = 6;
        const uint32_t tiles = (c->n_pairs + 127u) / 128u;
        if (tiles >= 2048u) {
            g.cpb = 10u;
            g.wpc = 0;
        }
        const uint64_t bytes = (uint64_t)nt * nc * c->n_pairs * 8u;
        // launches of a quarter of a GiB up to the terms-table variant's 2 GiB: 12 channels WITHOUT the residency limit
        // was among the best two geometries on four boxes of four (64 x 256 x 8192: 905-912 Gcoeff/s against 872-887 with it)
        if (bytes >= (256ull << 20) && bytes < (2ull << 30) && tiles < 2048u) g.wpc = 0;
        if (bytes <= (32ull << 20) && tiled_blocks(c->n_pairs, false, 1, g.cpb, nc, nt) > 1024u) {
            g.tpb = 2;
            g.cpb = 16u;
            g.wpc = 0;
        }
    }
    // Large launches take the terms-table variant (no per-workgroup set-up, 30-50 VGPRs): its walks are
    // shorter still -- fp32 2 stores per wave (8 channels), at most 6 workgroups per CU; fp16 64 channels,
    // 32 with the b16 arithmetic form (profiles/r02_autotune.md, profiles/r02_fp16.md)
    if (want_terms_table(c, out16, g, nc, nt)) {
        g.tpb = 1;
        if (out16) {
            // fp16 is VALU-issue- and power-bound (27 / 21 vector operations per coefficient); beside that, what decides is the
            // number of channel rows the resident workgroups hold open, chan_per_block x workgroups per CU.  b16 arithmetic
            // form: a ridge at 100-150 rows (25-38 MiB of output) on every box swept, and a cliff (-12 %) beyond whose position
            // moves between boxes (140-190 rows): 20 channels x 6 workgroups per CU.  fp32-grade form: ridge at 200-320 rows,
            // cliff at 64 x 6: 48 channels x 5 (profiles/r03_fp16.md)
            g.cpb = half ? 20u : 48u;
            g.wpc = half ? 6 : 5;
        } else {
            g.cpb = 8u;
            g.wpc = 6;
        }
    }
    // rows of at most 4 tiles (<= 4 KiB): consecutive rows are nearly adjacent in memory, and in a small launch a
    // workgroup does better writing 16 of them, two tiles wide (64 KiB contiguous), than a short walk; a large launch of
    // such rows (16 x 16 x 32768: 128 MiB) is an ordinary store stream again, best at 10 channels x 6 workgroups per CU
    // on both boxes it was swept on (profiles/r02_autotune.md)
    if (!out16 && (c->n_pairs + 127u) / 128u <= 4u) {
        const uint64_t bytes = (uint64_t)nt * nc * c->n_pairs * 8u;
        if (bytes <= (32ull << 20)) {
            g.tpb = c->n_pairs > 128u ? 2 : 1;
            g.cpb = 16u;
            g.wpc = 0;
        } else {
            g.tpb = 1;
            g.cpb = 10u;
            g.wpc = 6;
        }
    }
    return g;
}

int tuned_slot(const dcs_bf_context *c, bool out16) { return out16 ? (c->k.uHalfMath != 0u ? 2 : 1) : 0; }

bf_geom pick_geometry(const dcs_bf_context *c, bool out16, uint32_t nc, uint32_t nt)
{
    constexpr uint64_t kResident = 256u * 8u;
    bf_geom g = shape_default_geometry(c, out16, nc, nt);
    const dcs_bf_context::tuned_geom &t = c->tuned[tuned_slot(c, out16)][want_terms_table(c, out16, g, nc, nt) ? 1 : 0];
    if (t.valid && tiled_blocks(c->n_pairs, out16, t.tpb, (uint32_t)t.cpb, nc, nt) > kResident) {
        g.tpb = t.tpb;
        g.cpb = (uint32_t)t.cpb;
        g.wpc = t.wpc > 0 ? t.wpc : 0;
    }
    if (c->tune.tiles_per_block) g.tpb = c->tune.tiles_per_block;
    if (c->tune.chan_per_block) g.cpb = (uint32_t)c->tune.chan_per_block;
    if (c->tune.wg_per_cu != 0) g.wpc = c->tune.wg_per_cu > 0 ? c->tune.wg_per_cu : 0;
    else if (tiled_blocks(c->n_pairs, out16, g.tpb, g.cpb, nc, nt) <= kResident) g.wpc = 0;
    return g;
}

// Dynamic LDS a launch asks for so that exactly k workgroups fit a CU's 160 KiB (gfx950): the
// kernel's own staging buffer (TPB tiles x 64*PPL pairs x 8 B) is static -- and absent from the
// terms-table variant, which has no LDS of its own at all.
uint32_t lds_pad_for(int k, bool out16, int tpb, bool terms_table)
{
    const uint32_t kLds = 160u * 1024u, stat = terms_table ? 0u : (uint32_t)tpb * (out16 ? 256u : 128u) * 8u;
    uint32_t per = (kLds / (uint32_t)k) & ~1023u; // k * per <= 160 KiB < (k + 1) * per for k <= 7
    if (per > 64u * 1024u) per = 64u * 1024u;      // default per-workgroup limit
    return per > stat ? per - stat : 0u;
}

int prepare_tiled(dcs_bf_context *c, bool out16, const float *dt_dev, float dt0, uint32_t nt, uint32_t c0,
                  uint32_t nc, void *d_out, bf_kernel_launch *l, const float *dt_host = nullptr, bool terms_table = false)
{
    bf_tiled_args a;
    std::memset(&a, 0, sizeof(a));
    a.delays = c->d_table[c->cur];
    a.out = d_out;
    a.dt_dev = dt_dev;
    a.dt0 = dt0;
    a.n_pairs = c->n_pairs;
    a.c0 = c0;
    a.nc = nc;
    a.nt = nt;
    a.k = c->k;
    if (terms_table) {
        a.terms = c->d_tt_terms;
        a.flags = c->d_tt_flags;
        a.pairs_pad = c->pairs_pad;
    }
    const bf_geom g = pick_geometry(c, out16, nc, nt);
    const int tpb = g.tpb;
    const bool ntstore = g.ntstore;
    a.chan_per_block = g.cpb;
    a.xcd_remap = c->tune.xcd_remap > 0 ? 1u : 0u;
#ifdef DCS_PROBES
    a.pace = (uint32_t)c->probe.pace;
#endif
    const int st = (int)bf_prepare_tiled(a, dt_host, out16, tpb | (DCS_PROBE_KNOB(c, nomath) ? 0x100 : 0) | (c->tuning_now ? 0x200 : 0), ntstore, l);
    if (st == DCS_OK && g.wpc > 0) l->shared = lds_pad_for(g.wpc, out16, tpb, terms_table);
    return st;
}

// Arguments of the pre-pass kernel of the terms-table variant (it also writes the tiles that need the slow path).
void fill_terms_table_args(const dcs_bf_context *c, bool out16, float dt0, uint32_t nt, uint32_t c0, uint32_t nc, void *d_out,
                           const float *dt_host, bf_terms_args *ta)
{
    std::memset(ta, 0, sizeof(*ta));
    ta->delays = c->d_table[c->cur];
    ta->terms = c->d_tt_terms;
    ta->flags = c->d_tt_flags;
    ta->dt_dev = nullptr;
    ta->dt0 = dt0;
    ta->dt_inline[0] = dt0;
    if (nt > 1 && dt_host) std::memcpy(ta->dt_inline, dt_host, (size_t)nt * sizeof(float));
    ta->n_pairs = c->n_pairs;
    ta->pairs_pad = c->pairs_pad;
    ta->nt = nt;
    ta->k = c->k;
    ta->out = d_out;
    ta->c0 = c0;
    ta->nc = nc;
    ta->out16 = out16 ? 1u : 0u;
}

int launch_tiled(dcs_bf_context *c, bool out16, const float *dt_dev, float dt0, uint32_t nt, uint32_t c0,
                 uint32_t nc, void *d_out, hipStream_t stream, const float *dt_host = nullptr)
{
    const bool tt = dt_dev == nullptr && (nt == 1 || dt_host != nullptr) &&
                    want_terms_table(c, out16, pick_geometry(c, out16, nc, nt), nc, nt);
    if (tt) {
        bf_terms_args ta;
        fill_terms_table_args(c, out16, dt0, nt, c0, nc, d_out, dt_host, &ta);
        const hipError_t e = bf_launch_terms(ta, stream);
        if (e != hipSuccess) return (int)e;
    }
    bf_kernel_launch l;
    int st = prepare_tiled(c, out16, dt_dev, dt0, nt, c0, nc, d_out, &l, dt_host, tt);
    if (st != DCS_OK || l.func == nullptr) return st;
    void *params[] = {&l.args};
    return (int)hipLaunchKernel(l.func, l.grid, l.block, params, l.shared, stream);
}

// Steps that block on an event, allocate or copy from pinned staging cannot be part of a stream capture.  They ask
// first and refuse with a status, BEFORE anything is enqueued: the caller's capture stays valid (a HIP error from
// deep inside -- hipEventSynchronize or hipMalloc under capture -- would have invalidated it).
int refuse_if_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    DCS_TRY(hipStreamIsCapturing(stream, &cs));
    return cs == hipStreamCaptureStatusNone ? DCS_OK : DCS_ERR_UNSUPPORTED;
}

// The number of this beamformer call for its class words (bf_bform_terms_args::epoch): counts up, and starts again --
// behind a clearing of the words -- before it would run out of the 30 bits it has.
int next_flag_epoch(dcs_bf_context *c, hipStream_t s, uint32_t *epoch)
{
    if (c->flag_epoch >= (1u << 30) - 2u) {
        DCS_TRY(bf_launch_clear_words(c->d_flags, c->terms_steps * (c->pairs_pad / 64u), s));
        c->flag_epoch = 0;
    }
    *epoch = ++c->flag_epoch;
    return DCS_OK;
}

// The tag alone makes a call's class words its own only while the calls reach the device in the order they were numbered
// in.  A captured call keeps its number, so its replays run after calls with higher ones, whose words it could neither
// overwrite (atomicMax) nor recognise; a call after the counter has started again meets the same from a graph captured
// before.  So the first beamformer call made on a capturing stream, and every beamformer call of that context after it,
// zeroes its nt words on the caller's stream in front of the pre-pass (one small launch more, a kernel node in the graph):
// whatever ran before, the words then hold this call's classes.  A context that never captures keeps its launches as they are.
int clear_class_words(dcs_bf_context *c, uint32_t nt, hipStream_t s)
{
    if (!c->flags_cleared) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        DCS_TRY(hipStreamIsCapturing(s, &cs));
        if (cs == hipStreamCaptureStatusNone) return DCS_OK;
        c->flags_cleared = true;
    }
    DCS_TRY(bf_launch_clear_words(c->d_flags, nt, s));
    return DCS_OK;
}

// The terms table (up to 64 MiB) is only needed by the rows form and the fused kernel:
// allocate it when one of them is first used.  Not capturable (hipMalloc): a first call on a
// capturing stream is refused up front (make one call outside the capture).
int ensure_terms(dcs_bf_context *c, hipStream_t stream)
{
    if (c->d_terms && c->d_flags) return DCS_OK;
    {
        const int cap = refuse_if_capturing(stream);
        if (cap != DCS_OK) return cap;
    }
    if (!c->d_terms) DCS_TRY(hipMalloc((void **)&c->d_terms, (size_t)c->terms_steps * c->pairs_pad * 8u));
    if (!c->d_flags) {
        const size_t nb = (size_t)c->terms_steps * (c->pairs_pad / 64u) * 4u;
        DCS_TRY(hipMalloc((void **)&c->d_flags, nb));
        // epoch 0: no call has that number.  On the caller's stream (not capturing: asked above), in front of the launches of
        // the call that allocates: a hipMemset on the null stream is not ordered against a non-blocking stream, and the words
        // of a first call's pre-pass could be zeroed under it
        DCS_TRY(bf_launch_clear_words(c->d_flags, (uint32_t)(nb / 4u), stream));
        c->flag_epoch = 0;
    }
    return DCS_OK;
}

// Row-streaming form: terms pre-pass, then short waves in address order.
int launch_rows(dcs_bf_context *c, bool out16, const float *dt_dev, float dt0, uint32_t nt, uint32_t c0,
                uint32_t nc, void *d_out, hipStream_t stream)
{
    if (nt > c->terms_steps) return DCS_ERR_INVALID_ARGUMENT;
    int st_alloc = ensure_terms(c, stream);
    if (st_alloc != DCS_OK) return st_alloc;
    bf_terms_args ta;
    std::memset(&ta, 0, sizeof(ta));
    ta.delays = c->d_table[c->cur];
    ta.terms = c->d_terms;
    ta.flags = c->d_flags;
    ta.dt_dev = dt_dev;
    ta.dt0 = dt0;
    ta.dt_inline[0] = dt0;
    ta.n_pairs = c->n_pairs;
    ta.pairs_pad = c->pairs_pad;
    ta.nt = nt;
    ta.k = c->k;
    hipError_t e = bf_launch_terms(ta, stream);
    if (e != hipSuccess) return (int)e;
    bf_rows_args a;
    std::memset(&a, 0, sizeof(a));
    a.terms = c->d_terms;
    a.flags = c->d_flags;
    a.out = d_out;
    a.n_pairs = c->n_pairs;
    a.pairs_pad = c->pairs_pad;
    a.c0 = c0;
    a.nc = nc;
    a.nt = nt;
    a.D = c->k.fDenominator;
    a.y = c->k.fRcpDenominator;
    a.div3 = c->k.uDiv3Exact;
    // defaults (profiles/r01_geometry_sweep.md): 8 waves share one tile and interleave 16 rows
    const bool same_tile = c->tune.rows_same_tile < 0 ? true : c->tune.rows_same_tile != 0;
    const int nw = c->tune.waves_per_block ? c->tune.waves_per_block : (same_tile ? 8 : 4);
    const int rpw = c->tune.rows_per_wave ? c->tune.rows_per_wave : (out16 ? 4 : 2);
    const bool ntstore = c->tune.nontemporal < 0 ? true : c->tune.nontemporal != 0;
    const bool xcd = c->tune.xcd_remap < 0 ? !same_tile : c->tune.xcd_remap != 0;
    a.same_tile = same_tile ? 1u : 0u;
#ifdef DCS_PROBES
    a.pace = (uint32_t)c->probe.pace;
#endif
    if (c->tune.wg_per_cu > 0) { // rows form: only when asked for (no default limit)
        uint32_t per = (160u * 1024u / (uint32_t)c->tune.wg_per_cu) & ~1023u;
        a.lds_pad = per > 64u * 1024u ? 64u * 1024u : per;
    }
    return (int)bf_launch_rows(a, out16, nw, rpw, ntstore, xcd, DCS_PROBE_KNOB(c, nomath) != 0, stream);
}

// form 1 = tiled (long-lived waves), 2 = rows (short waves); 0 = library default
int launch_form(dcs_bf_context *c, bool out16, const float *dt_dev, float dt0, uint32_t nt, uint32_t c0,
                uint32_t nc, void *d_out, hipStream_t stream)
{
    const int form = c->tune.form ? c->tune.form : 1;
    return form != 2 ? launch_tiled(c, out16, dt_dev, dt0, nt, c0, nc, d_out, stream)
                     : launch_rows(c, out16, dt_dev, dt0, nt, c0, nc, d_out, stream);
}

// Where a call's fDeltaTime values come from: the verifier's recipe for time indices
// [t0, t0 + nt) (dcs_bf_delta_times), or the caller's own values (dcs_bf_generate_dt / _at).
struct dt_source {
    const float *values; // nullptr: derive from the time index
    uint64_t t0;
};
// the calls behind bf_ctx_ext_ops take both: the caller's values where there are any, else the time index
dt_source dt_or_index(const float *dt, uint64_t t) { return dt_source{dt, dt ? 0 : t}; }

int fill_dt(const dcs_bf_context *c, const dt_source &src, uint32_t off, uint32_t n, float *dst)
{
    if (src.values) {
        std::memcpy(dst, src.values + off, (size_t)n * sizeof(float));
        return DCS_OK;
    }
    return dcs_bf_delta_times(&c->p, src.t0 + off, n, dst);
}

// Can every fDeltaTime of a call's nt time steps be worked out?  The multi-launch calls ask BEFORE anything else happens
// on the context or the stream (allocation, the capture check, the first enqueue), so that a time index which overflows
// the verifier's nanosecond step (dcs_bf_delta_times: DCS_ERR_OUT_OF_RANGE) costs nothing but the status -- not a tensor
// written up to the chunk that holds it.  The step RN(RN(RN((float)t * SAMPLING_PERIOD) * 1e9f) * FFT_SIZE) does not decrease
// as t grows (the conversion rounds monotonically, and so does every product by a positive constant: params_ok), and
// nothing else in the recipe can fail, so the LAST index decides; a range that wraps round 2^64 is out of range by itself.
int check_dt_range(const dcs_bf_context *c, const dt_source &src, uint32_t nt)
{
    if (src.values || nt == 0) return DCS_OK;
    const uint64_t t_last = src.t0 + (uint64_t)(nt - 1u);
    if (t_last < src.t0) return DCS_ERR_OUT_OF_RANGE;
    float dt;
    return dcs_bf_delta_times(&c->p, t_last, 1, &dt);
}

// Stage n fDeltaTime values through a pinned slot into device memory on `stream`.  Not capturable: callers check
// refuse_if_capturing() before their first launch.
int stage_dt(dcs_bf_context *c, const dt_source &src, uint32_t off, uint32_t n, hipStream_t stream, const float **dt_dev)
{
    const int slot = c->dt_next;
    c->dt_next = (c->dt_next + 1) % kDtSlots;
    if (c->dt_used[slot]) DCS_TRY(hipEventSynchronize(c->dt_ev[slot])); // slot still in flight?
    float *h = c->h_dt + (size_t)slot * kDtSlotFloats;
    float *d = c->d_dt + (size_t)slot * kDtSlotFloats;
    int st = fill_dt(c, src, off, n, h);
    if (st != DCS_OK) return st;
    DCS_TRY(hipMemcpyAsync(d, h, (size_t)n * sizeof(float), hipMemcpyHostToDevice, stream));
    DCS_TRY(hipEventRecord(c->dt_ev[slot], stream));
    c->dt_used[slot] = true;
    *dt_dev = d;
    return DCS_OK;
}

int generate_slab_impl(dcs_bf_context *c, int bitwidth, const dt_source &src, uint32_t nt, uint32_t c0, uint32_t nc,
                       void *d_out, size_t out_bytes, void *stream)
{
    if (!c || (!d_out && nt && nc)) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if (bitwidth != DCS_BF_B16 && bitwidth != DCS_BF_B32) return DCS_ERR_INVALID_ARGUMENT;
    if (!c->table_set) return DCS_ERR_NOT_READY;
    if ((uint64_t)c0 + nc > (uint64_t)c->p.nr_channels) return DCS_ERR_OUT_OF_RANGE;
    const bool out16 = bitwidth == DCS_BF_B16;
    const size_t eb = out16 ? 4 : 8;
    const size_t step_bytes = (size_t)nc * c->n_pairs * eb;
    if (out_bytes < step_bytes * nt) return DCS_ERR_INVALID_ARGUMENT;
    {
        const int st_range = check_dt_range(c, src, nt); // the whole call's time indices, before the first chunk is launched
        if (st_range != DCS_OK) return st_range;
    }
    hipStream_t s = as_stream(stream);
    if (nt > 1 && (c->tune.form == 2 || nt > kDtInline)) { // the fDeltaTime values will be staged through pinned memory
        const int cap = refuse_if_capturing(s);
        if (cap != DCS_OK) return cap;
    }
    for (uint32_t done = 0; done < nt;) {
        uint32_t n = (nt - done) < kDtSlotFloats ? (nt - done) : kDtSlotFloats;
        if (n > c->terms_steps) n = c->terms_steps;
        char *dst = static_cast<char *>(d_out) + (size_t)done * step_bytes;
        int st;
        if (n == 1) {
            float dt;
            if ((st = fill_dt(c, src, done, 1, &dt)) != DCS_OK) return st;
            st = launch_form(c, out16, nullptr, dt, 1, c0, nc, dst, s);
        } else if (c->tune.form != 2 && n <= kDtInline) {
            // tiled form, few time steps: their dt values ride in the kernel arguments (no copy in front)
            float dts[kDtInline];
            if ((st = fill_dt(c, src, done, n, dts)) != DCS_OK) return st;
            st = launch_tiled(c, out16, nullptr, dts[0], n, c0, nc, dst, s, dts);
        } else {
            const float *dt_dev = nullptr;
            if ((st = stage_dt(c, src, done, n, s, &dt_dev)) != DCS_OK) return st;
            st = launch_form(c, out16, dt_dev, 0.0f, n, c0, nc, dst, s);
        }
        if (st != DCS_OK) return st;
        done += n;
    }
    return DCS_OK;
}

int generate_impl(dcs_bf_context *c, int kernel, int bitwidth, const dt_source &src, uint32_t nt, void *d_out,
                  size_t out_bytes, void *stream)
{
    if (!c) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if (bitwidth != DCS_BF_B16 && bitwidth != DCS_BF_B32) return DCS_ERR_INVALID_ARGUMENT;
    // BeamformerCoefficientTest.cu:40-50 (the reference throws)
    if (kernel == DCS_BF_COMBINED_COEFF_GEN_AND_BEAMFORMER_SINGLE_CHANNEL) return DCS_ERR_UNSUPPORTED;
    if (kernel == DCS_BF_NAIVE && bitwidth == DCS_BF_B16) return DCS_ERR_UNSUPPORTED;
    if (kernel != DCS_BF_NAIVE && kernel != DCS_BF_MULTIPLE_CHANNELS &&
        kernel != DCS_BF_MULTIPLE_CHANNELS_AND_TIMESTAMPS)
        return DCS_ERR_INVALID_ARGUMENT;
    if (!d_out && nt) return DCS_ERR_INVALID_ARGUMENT;
    if (!c->table_set) return DCS_ERR_NOT_READY;
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (kernel == DCS_BF_MULTIPLE_CHANNELS_AND_TIMESTAMPS)
        return generate_slab_impl(c, bitwidth, src, nt, 0, C, d_out, out_bytes, stream);

    const bool out16 = bitwidth == DCS_BF_B16;
    const size_t step_bytes = (size_t)C * c->n_pairs * (out16 ? 4 : 8);
    if (out_bytes < step_bytes * nt) return DCS_ERR_INVALID_ARGUMENT;
    hipStream_t s = as_stream(stream);
    // The time steps write disjoint tensors and read the same table: from 8 of them on, MULTIPLE_CHANNELS' launches go
    // round the context's side streams between a fork and a join on the caller's stream -- its kernel (terms through LDS,
    // a barrier, then the walk) takes ~3 us of latency on an empty chip, and four queues overlap that: 256 launches in
    // 0.67 ms instead of 0.84.  (NAIVE's loop is bound by the host's launch rate and ran 8 % slower spread out: it stays on
    // the caller's stream.  The pattern is capturable.)
    const bool fan = nt >= 8u && kernel == DCS_BF_MULTIPLE_CHANNELS && !want_terms_table(c, out16, pick_geometry(c, out16, C, 1), C, 1);
    // every fDeltaTime is worked out (and found in range) BEFORE the first launch and before the fork: a bad time index
    // costs nothing but the status
    float dt_small[kDtInline];
    float *dts = dt_small;
    if (nt > kDtInline) {
        dts = new (std::nothrow) float[nt];
        if (!dts) return (int)hipErrorOutOfMemory;
    }
    int st = nt ? fill_dt(c, src, 0, nt, dts) : DCS_OK;
    bool forked = false;
    if (st == DCS_OK && fan) {
        st = (int)hipEventRecord(c->fork_ev, s);
        for (int k = 0; k < kSideStreams && st == DCS_OK; k++) st = (int)hipStreamWaitEvent(c->side[k], c->fork_ev, 0);
        forked = st == DCS_OK;
    }
    // host time loop, one launch per time step: BeamformerCoefficientTest.cu:230-250
    for (uint32_t i = 0; i < nt && st == DCS_OK; i++) {
        hipStream_t s_step = forked ? c->side[i % kSideStreams] : s;
        char *dst = static_cast<char *>(d_out) + (size_t)i * step_bytes;
#ifdef DCS_PROBES
        if (c->probe.fail_at_step > 0 && i + 1u == (uint32_t)c->probe.fail_at_step) { // injected (error-path tests)
            st = (int)hipErrorLaunchFailure;
            break;
        }
#endif
        if (kernel == DCS_BF_NAIVE) {
            bf_naive_args a;
            std::memset(&a, 0, sizeof(a));
            a.delays = c->d_table[c->cur];
            a.out = reinterpret_cast<float *>(dst);
            a.dt = dts[i];
            a.n_pairs = c->n_pairs;
            a.c0 = 0;
            a.nc = C;
            a.k = c->k;
            st = (int)bf_launch_naive(a, s_step);
        } else {
            st = launch_tiled(c, out16, nullptr, dts[i], 1, 0, C, dst, s_step);
        }
    }
    if (dts != dt_small) delete[] dts;
    // the join happens on EVERY way out of the loop: whatever the side streams were given runs before anything the
    // caller enqueues next (outside a capture), and a capture is left with no unjoined fork.  The first failure is
    // what is returned.
    if (forked) {
        for (int k = 0; k < kSideStreams; k++) {
            int j = (int)hipEventRecord(c->join_ev[k], c->side[k]);
            if (j == DCS_OK) j = (int)hipStreamWaitEvent(s, c->join_ev[k], 0);
            if (st == DCS_OK) st = j;
        }
    }
    return st;
}

// dt[i] = ts_diff(ref, cur[i]) for a (current, reference) pair per time step.
int dts_from_timespecs(const struct timespec *cur, const struct timespec *ref, uint32_t nt, float *dt)
{
    for (uint32_t i = 0; i < nt; i++) {
        const int st = dcs_bf_ts_diff(ref, &cur[i], &dt[i]);
        if (st != DCS_OK) return st;
    }
    return DCS_OK;
}

} // namespace

int dcs_bf_generate_slab(dcs_bf_context *c, int bitwidth, uint64_t t0, uint32_t nt, uint32_t c0, uint32_t nc,
                         void *d_out, size_t out_bytes, void *stream)
{
    return generate_slab_impl(c, bitwidth, dt_source{nullptr, t0}, nt, c0, nc, d_out, out_bytes, stream);
}

int dcs_bf_generate(dcs_bf_context *c, int kernel, int bitwidth, uint64_t t0, uint32_t nt, void *d_out,
                    size_t out_bytes, void *stream)
{
    return generate_impl(c, kernel, bitwidth, dt_source{nullptr, t0}, nt, d_out, out_bytes, stream);
}

int dcs_bf_generate_dt(dcs_bf_context *c, int kernel, int bitwidth, const float *dt, uint32_t nt, void *d_out,
                       size_t out_bytes, void *stream)
{
    if (!dt && nt) return DCS_ERR_INVALID_ARGUMENT;
    return generate_impl(c, kernel, bitwidth, dt_source{dt, 0}, nt, d_out, out_bytes, stream);
}

int dcs_bf_generate_slab_dt(dcs_bf_context *c, int bitwidth, const float *dt, uint32_t nt, uint32_t c0, uint32_t nc,
                            void *d_out, size_t out_bytes, void *stream)
{
    if (!dt && nt) return DCS_ERR_INVALID_ARGUMENT;
    return generate_slab_impl(c, bitwidth, dt_source{dt, 0}, nt, c0, nc, d_out, out_bytes, stream);
}

int dcs_bf_generate_at(dcs_bf_context *c, int kernel, int bitwidth, const struct timespec *cur,
                       const struct timespec *ref, uint32_t nt, void *d_out, size_t out_bytes, void *stream)
{
    if ((!cur && nt) || !ref) return DCS_ERR_INVALID_ARGUMENT;
    float small[kDtInline];
    float *dt = small;
    if (nt > kDtInline) {
        dt = new (std::nothrow) float[nt];
        if (!dt) return (int)hipErrorOutOfMemory;
    }
    int st = dts_from_timespecs(cur, ref, nt, dt);
    // the values are consumed (kernel arguments / pinned staging slots) before generate_impl returns
    if (st == DCS_OK) st = generate_impl(c, kernel, bitwidth, dt_source{dt, 0}, nt, d_out, out_bytes, stream);
    if (dt != small) delete[] dt;
    return st;
}

namespace {
// Per-input beam weights: the normalised weights and scales of the pre-pass (bf_weights_args).  Not capturable (hipMalloc):
// a first weighted call on a capturing stream is refused up front, as ensure_terms does.
int ensure_weights(dcs_bf_context *c, hipStream_t stream)
{
    if (c->d_wnorm && c->d_wscale) return DCS_OK;
    {
        const int cap = refuse_if_capturing(stream);
        if (cap != DCS_OK) return cap;
    }
    if (!c->d_wnorm) DCS_TRY(hipMalloc((void **)&c->d_wnorm, (size_t)c->n_pairs * sizeof(float)));
    if (!c->d_wscale) DCS_TRY(hipMalloc((void **)&c->d_wscale, (size_t)c->p.nr_beams * sizeof(float)));
    return DCS_OK;
}

bool weights_ok(const float *d_weights) { return d_weights && !(reinterpret_cast<uintptr_t>(d_weights) & 3u); }

// The terms pre-pass of both beamformers: draws the call's number for the class words (*epoch) and makes the terms of nt time
// steps -- with d_weights, the normalised weights and scales as well.  dt_dev, dt0, dt_inline: as bf_launch_bform_terms takes them.
int launch_bform_terms(dcs_bf_context *c, const float *d_weights, uint32_t nt, const float *dt_dev, float dt0, const float *dt_inline,
                       hipStream_t s, uint32_t *epoch)
{
    const int st_ep = next_flag_epoch(c, s, epoch);
    if (st_ep != DCS_OK) return st_ep;
    const int st_clr = clear_class_words(c, nt, s);
    if (st_clr != DCS_OK) return st_clr;
    bf_bform_terms_args ta;
    std::memset(&ta, 0, sizeof(ta));
    ta.delays = c->d_table[c->cur];
    ta.terms = c->d_terms;
    ta.flags = c->d_flags;
    ta.epoch = *epoch;
    ta.dt_dev = dt_dev;
    ta.dt0 = dt0;
    ta.n_pairs = c->n_pairs;
    ta.A = (uint32_t)c->p.nr_stations;
    ta.B = (uint32_t)c->p.nr_beams;
    ta.nt = nt;
    ta.k = c->k;
    const bf_weights_args wa = {d_weights, c->d_wnorm, c->d_wscale};
    return (int)(d_weights ? bf_launch_bform_terms_weighted(ta, wa, dt_inline, s) : bf_launch_bform_terms(ta, dt_inline, s));
}

// d_weights: nullptr (the unweighted call) or [B][A] fp32 weights in device memory (include/dcs_beam_weights.h)
int beamform_impl(dcs_bf_context *c, const dt_source &src, uint32_t nt, const int8_t *d_antenna,
                  size_t antenna_bytes, float *d_beams, size_t beams_bytes, void *stream, const float *d_weights = nullptr)
{
    if (!c || (nt && (!d_antenna || !d_beams))) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if (nt % 16u) return DCS_ERR_INVALID_ARGUMENT; // INTERNAL_TIME_SAMPLES, BeamformerParameters.h:51
    if (!c->table_set) return DCS_ERR_NOT_READY;
    const uint32_t A = (uint32_t)c->p.nr_stations, B = (uint32_t)c->p.nr_beams, C = (uint32_t)c->p.nr_channels;
    // BeamformerCoefficientTest.cu:25-26 (sizes of the antenna and beam tensors)
    if (antenna_bytes < (size_t)A * C * nt * 2u) return DCS_ERR_INVALID_ARGUMENT;
    if (beams_bytes < (size_t)B * C * nt * 2u * sizeof(float)) return DCS_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(d_antenna) & 3u) || (reinterpret_cast<uintptr_t>(d_beams) & 7u))
        return DCS_ERR_INVALID_ARGUMENT;
    {
        const int st_range = check_dt_range(c, src, nt); // the whole call's time indices, before the first chunk is launched
        if (st_range != DCS_OK) return st_range;
    }
    hipStream_t s = as_stream(stream);
    {
        int st_alloc = ensure_terms(c, s);
        if (st_alloc == DCS_OK && d_weights) st_alloc = ensure_weights(c, s);
        if (st_alloc != DCS_OK) return st_alloc;
    }
    const bf_weights_args wa = {d_weights, c->d_wnorm, c->d_wscale};
    uint32_t chunk = c->terms_steps & ~15u; // time steps per launch: what the terms table holds
    if (chunk > kDtSlotFloats) chunk = kDtSlotFloats;
    if (chunk == 0) return DCS_ERR_UNSUPPORTED;
    if (nt > kDtInline) { // more time steps than ride in the kernel arguments: staged through pinned memory
        const int cap = refuse_if_capturing(s);
        if (cap != DCS_OK) return cap;
    }
    for (uint32_t done = 0; done < nt;) {
        const uint32_t n = (nt - done) < chunk ? (nt - done) : chunk;
        // up to 256 time steps per launch: their fDeltaTime values travel in the terms kernel's arguments (the reference's
        // block of 256 samples is then two launches and nothing else); longer launches stage a table through pinned memory
        const float *dt_dev = nullptr;
        float dt_val[kDtInline];
        const bool inl = n <= kDtInline;
        int st = inl ? fill_dt(c, src, done, n, dt_val) : stage_dt(c, src, done, n, s, &dt_dev);
        if (st != DCS_OK) return st;
        uint32_t epoch = 0;
        st = launch_bform_terms(c, d_weights, n, dt_dev, 0.0f, inl ? dt_val : nullptr, s, &epoch);
        if (st != DCS_OK) return st;
        bf_beamform_args a;
        std::memset(&a, 0, sizeof(a));
        a.terms = c->d_terms;
        a.flags = c->d_flags;
        a.epoch = epoch;
        a.ant = d_antenna;
        a.beams = d_beams;
        a.A = A;
        a.B = B;
        a.C = C;
        a.nt16 = n / 16u;
        a.tex0 = done / 16u;
        a.nt16_total = nt / 16u;
        // enough workgroups to fill the chip, but keep a few channels per workgroup
        // so the staged terms lines are reused from L1
        uint32_t cpb = 4; // 4 / 8 / 16 / 32 measured: 4 is best by 1 % at 64 antennas and by 5 % at 256 (profiles/r01_fused.md)
        while (cpb > 1 && (uint64_t)((B + 15u) / 16u) * ((C + cpb - 1) / cpb) * a.nt16 < 2048u) cpb >>= 1;
        a.chan_per_block = cpb;
        a.k = c->k;
        DCS_TRY(bf_launch_beamform(a, d_weights ? &wa : nullptr, s));
        done += n;
    }
    return DCS_OK;
}
} // namespace

int dcs_bf_generate_and_beamform(dcs_bf_context *c, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                 size_t antenna_bytes, float *d_beams, size_t beams_bytes, void *stream)
{
    if (t0 % 16u) return DCS_ERR_INVALID_ARGUMENT; // whole 16-sample blocks
    return beamform_impl(c, dt_source{nullptr, t0}, nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream);
}

int dcs_bf_generate_and_beamform_dt(dcs_bf_context *c, const float *dt, uint32_t nt, const int8_t *d_antenna,
                                    size_t antenna_bytes, float *d_beams, size_t beams_bytes, void *stream)
{
    if (!dt && nt) return DCS_ERR_INVALID_ARGUMENT;
    return beamform_impl(c, dt_source{dt, 0}, nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream);
}

namespace {
// What a call of the matrix-core beamformer writes to d_beams, and what it applies on the way.  kFloat: the beams, (re, im)
// fp32 per sample; kInt8: the same quantised (include/dcs_beam_quant.h), a quarter the size; kBlockPower: one float per beam
// and 16-sample block (include/dcs_beam_power.h), 4-byte aligned.
struct bacc_output {
    enum { kFloat, kInt8, kBlockPower } kind;
    const float *d_weights; // nullptr (unweighted) or [B][A] fp32 weights in device memory (include/dcs_beam_weights.h)
    bf_quant_args quant;    // kInt8 only: the quantiser's gains and counters
    size_t block_bytes() const // per beam and 16-sample block
    {
        return kind == kBlockPower ? sizeof(float) : 32u * (kind == kInt8 ? sizeof(int8_t) : sizeof(float));
    }
    uintptr_t align_mask() const { return kind == kBlockPower ? 3u : 7u; }
};

int beamform_acc_impl(dcs_bf_context *c, const dt_source &src, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                      void *d_beams, size_t beams_bytes, void *stream, const bacc_output &out = {bacc_output::kFloat, nullptr, {}})
{
    if (!c || (nt && (!d_antenna || !d_beams))) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if (nt % 16u) return DCS_ERR_INVALID_ARGUMENT; // INTERNAL_TIME_SAMPLES, BeamformerParameters.h:51
    if (!c->table_set) return DCS_ERR_NOT_READY;
    const uint32_t A = (uint32_t)c->p.nr_stations, B = (uint32_t)c->p.nr_beams, C = (uint32_t)c->p.nr_channels;
    if (A > 256u) return DCS_ERR_UNSUPPORTED; // the coefficient planes of one workgroup must fit 64 KiB of LDS
    if (antenna_bytes < (size_t)A * C * nt * 2u) return DCS_ERR_INVALID_ARGUMENT;
    if (beams_bytes < (size_t)B * C * (nt / 16u) * out.block_bytes()) return DCS_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(d_antenna) & 15u) || (reinterpret_cast<uintptr_t>(d_beams) & out.align_mask()))
        return DCS_ERR_INVALID_ARGUMENT;
    if ((out.d_weights || out.kind != bacc_output::kFloat) && (c->tune.math_mode & 8)) return DCS_ERR_UNSUPPORTED; // the fp32 fma-chain form has no weights, no quantiser, no detector
    if (nt == 0) return DCS_OK;
    {
        const int st_range = check_dt_range(c, src, 1); // the one coefficient time, before anything is allocated
        if (st_range != DCS_OK) return st_range;
    }
    hipStream_t s = as_stream(stream);
    {
        int st_alloc = ensure_terms(c, s);
        if (st_alloc == DCS_OK && out.d_weights) st_alloc = ensure_weights(c, s);
        if (st_alloc != DCS_OK) return st_alloc;
    }
    float dt_coeff = 0.0f; // ONE coefficient time for the whole block of samples: by value, in the kernel arguments
    int st = fill_dt(c, src, 0, 1, &dt_coeff);
    if (st != DCS_OK) return st;
    uint32_t epoch = 0;
    st = launch_bform_terms(c, out.d_weights, 1, nullptr, dt_coeff, nullptr, s, &epoch);
    if (st != DCS_OK) return st;
    bf_bacc_args a;
    std::memset(&a, 0, sizeof(a));
    a.terms = c->d_terms;
    a.flags = c->d_flags;
    a.epoch = epoch;
    a.ant = d_antenna;
    a.beams = static_cast<float *>(d_beams);
    a.A = A;
    a.B = B;
    a.C = C;
    a.nT16 = nt / 16u;
    a.k = c->k;
    a.fp32_chain = (c->tune.math_mode & 8) ? 1u : 0u; // math_mode bit 3: the fp32 fma-chain form
#ifdef DCS_PROBES
    // the A/B switches of profiles/r02_fused.md / r03_fused.md: dcs_probe_set_knobs, or (tools/measure.py bfacc driven
    // through the ordinary wrappers with DCS_LIB_PATH=probes/libdcs_probes.so) the environment
    auto knob = [](int32_t v, const char *env) { const char *e = std::getenv(env); return (uint32_t)(v ? v : (e ? std::atoi(e) : 0)); };
    a.max_rounds = knob(c->probe.bacc_rounds, "DCS_BACC_ROUNDS");
    a.probe = knob(c->probe.bacc_probe, "DCS_BACC_PROBE");
    a.unstaged = knob(c->probe.bacc_unstaged, "DCS_BACC_UNSTAGED");
    a.plain_stores = knob(c->probe.bacc_plain, "DCS_BACC_PLAIN");
    a.no_share = knob(c->probe.bacc_no_share, "DCS_BACC_NOSHARE");
    a.wg_per_cu = knob(c->probe.bacc_wg_per_cu, "DCS_BACC_WPC");
    a.order = knob(c->probe.bacc_order, "DCS_BACC_ORDER");
    a.nbt_force = knob(c->probe.bacc_nbt, "DCS_BACC_NBT");
    a.nw_force = knob(c->probe.bacc_waves, "DCS_BACC_WAVES");
#endif
    const bf_weights_args wa = {out.d_weights, c->d_wnorm, c->d_wscale};
    return (int)bf_launch_beamform_acc(a, out.d_weights ? &wa : nullptr, out.kind == bacc_output::kInt8 ? &out.quant : nullptr,
                                       out.kind == bacc_output::kBlockPower, s);
}

// include/dcs_beam_weights.h, reached through the table at the head of every context (bf_ctx_ext.h)
int generate_and_beamform_weighted_impl(dcs_bf_context *c, const float *dt, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                        size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                        void *stream)
{
    if (!c || !weights_ok(d_weights)) return DCS_ERR_INVALID_ARGUMENT;
    if (!dt && t0 % 16u) return DCS_ERR_INVALID_ARGUMENT; // whole 16-sample blocks
    return beamform_impl(c, dt_or_index(dt, t0), nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream, d_weights);
}

int beamform_accumulated_weighted_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                       const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, float *d_beams,
                                       size_t beams_bytes, void *stream)
{
    if (!c || !weights_ok(d_weights)) return DCS_ERR_INVALID_ARGUMENT;
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_beams, beams_bytes,
                             stream, {bacc_output::kFloat, d_weights, {}});
}

// include/dcs_beam_quant.h, reached the same way
int beamform_accumulated_q8_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                 size_t antenna_bytes, const float *d_weights, const float *d_quant_gains, int8_t *d_beams_q8,
                                 size_t beams_bytes, unsigned long long *d_clip_count, void *stream)
{
    if (!c || !weights_ok(d_quant_gains) || (d_weights && !weights_ok(d_weights)) || (reinterpret_cast<uintptr_t>(d_clip_count) & 7u))
        return DCS_ERR_INVALID_ARGUMENT;
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_beams_q8, beams_bytes,
                             stream, {bacc_output::kInt8, d_weights, {d_quant_gains, d_clip_count}});
}

// include/dcs_beam_power.h, reached the same way
int beamform_accumulated_power_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                    size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                    void *stream)
{
    if (!c || !d_block_power || (d_weights && !weights_ok(d_weights))) return DCS_ERR_INVALID_ARGUMENT;
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_block_power, power_bytes,
                             stream, {bacc_output::kBlockPower, d_weights, {}});
}

int integrate_block_power_impl(dcs_bf_context *c, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                               uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes, void *stream)
{
    if (!c || !weights_ok(d_block_power) || !weights_ok(d_spectra)) return DCS_ERR_INVALID_ARGUMENT;
    if (blocks_per_spectrum == 0u || nr_blocks % blocks_per_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    const uint32_t B = (uint32_t)c->p.nr_beams, C = (uint32_t)c->p.nr_channels;
    const uint64_t n_spectra = nr_blocks / blocks_per_spectrum;
    if (power_bytes < (size_t)C * nr_blocks * B * sizeof(float)) return DCS_ERR_INVALID_ARGUMENT;
    if (spectra_bytes < (size_t)n_spectra * C * B * sizeof(float)) return DCS_ERR_INVALID_ARGUMENT;
    bf_pint_args a;
    std::memset(&a, 0, sizeof(a));
    a.block_power = d_block_power;
    a.spectra = d_spectra;
    a.total = n_spectra * C * B;
    a.B = B;
    a.C = C;
    a.nr_blocks = nr_blocks;
    a.n = blocks_per_spectrum;
    a.accumulate = accumulate ? 1u : 0u;
    return (int)bf_launch_power_integrate(a, as_stream(stream));
}

// include/dcs_incoherent_beam.h, reached the same way.  No coefficients: no delay table, no terms, nothing allocated, and
// math_mode plays no part.
int incoherent_block_power_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                uint32_t *d_block_power, size_t power_bytes, void *stream)
{
    if (!c || !d_block_power || (d_weights && !weights_ok(d_weights)) || (nt && !d_antenna)) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if (nt % 16u) return DCS_ERR_INVALID_ARGUMENT;
    const uint32_t A = (uint32_t)c->p.nr_stations, C = (uint32_t)c->p.nr_channels;
    if (A > 256u) return DCS_ERR_UNSUPPORTED; // as the float call
    if (antenna_bytes < (size_t)A * C * nt * 2u) return DCS_ERR_INVALID_ARGUMENT;
    if (power_bytes < (size_t)C * (nt / 16u) * sizeof(uint32_t)) return DCS_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(d_antenna) & 15u) || (reinterpret_cast<uintptr_t>(d_block_power) & 3u))
        return DCS_ERR_INVALID_ARGUMENT;
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
    if (!c || !d_block_power || !d_spectra || ((reinterpret_cast<uintptr_t>(d_block_power) | reinterpret_cast<uintptr_t>(d_spectra)) & 3u))
        return DCS_ERR_INVALID_ARGUMENT;
    if (blocks_per_spectrum == 0u || nr_blocks % blocks_per_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    const uint64_t n_spectra = nr_blocks / blocks_per_spectrum;
    if (power_bytes < (size_t)C * nr_blocks * sizeof(uint32_t)) return DCS_ERR_INVALID_ARGUMENT;
    if (spectra_bytes < (size_t)n_spectra * C * sizeof(float)) return DCS_ERR_INVALID_ARGUMENT;
    bf_incoh_int_args a;
    std::memset(&a, 0, sizeof(a));
    a.block_power = d_block_power;
    a.spectra = d_spectra;
    a.total = n_spectra * C;
    a.C = C;
    a.nr_blocks = nr_blocks;
    a.n = blocks_per_spectrum;
    a.accumulate = accumulate ? 1u : 0u;
    return (int)bf_launch_incoherent_integrate(a, as_stream(stream));
}

// include/dcs_filterbank.h, reached the same way.  No coefficients and nothing allocated; nr_beams is the caller's, so the
// one set of calls serves detected (the context's beams) and incoherent (1) spectra.
// have >= x * y * z * w, the product taken without overflow
bool holds(size_t have, uint64_t x, uint64_t y, uint64_t z, uint64_t w)
{
    const unsigned __int128 xy = (unsigned __int128)x * y, zw = (unsigned __int128)z * w;
    if ((xy >> 64) || (zw >> 64)) return xy == 0 || zw == 0;
    const unsigned __int128 need = xy * zw;
    return !(need >> 64) && (uint64_t)need <= (uint64_t)have;
}

bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int spectra_sums_impl(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                      uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream)
{
    if (!c || !d_spectra || !d_sums || misaligned(d_spectra, 3u) || misaligned(d_sums, 7u) || nr_beams == 0u)
        return DCS_ERR_INVALID_ARGUMENT;
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
    if (!c || !d_sums || !d_scales || misaligned(d_sums, 7u) || misaligned(d_scales, 7u) || nr_beams == 0u || count == 0u ||
        count >= (1ull << 53))
        return DCS_ERR_INVALID_ARGUMENT;
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
    if (!c || !d_spectra || !d_scales || !d_filterbank || misaligned(d_spectra, 3u) || misaligned(d_scales, 7u) ||
        misaligned(d_filterbank, 15u) || misaligned(d_clip_count, 7u) || nr_beams == 0u || (flags & ~1u) ||
        first_spectrum > out_spectra || nr_spectra > out_spectra - first_spectrum)
        return DCS_ERR_INVALID_ARGUMENT;
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
    a.descending = flags & 1u;
    a.level = level;
    return (int)bf_launch_filterbank_q8(a, as_stream(stream));
}
} // namespace

int dcs_bf_beamform_accumulated(dcs_bf_context *c, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                float *d_beams, size_t beams_bytes, void *stream)
{
    return beamform_acc_impl(c, dt_source{nullptr, t_coeff}, nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream);
}

int dcs_bf_beamform_accumulated_dt(dcs_bf_context *c, float dt_coeff, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                   float *d_beams, size_t beams_bytes, void *stream)
{
    return beamform_acc_impl(c, dt_source{&dt_coeff, 0}, nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream);
}

int dcs_bf_autotune(dcs_bf_context *c, int bitwidth, void *d_out, size_t out_bytes, void *stream,
                    dcs_bf_tuning *chosen)
{
    if (!c || !d_out) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    if (bitwidth != DCS_BF_B16 && bitwidth != DCS_BF_B32) return DCS_ERR_INVALID_ARGUMENT;
    if (!c->table_set) return DCS_ERR_NOT_READY;
    const bool out16 = bitwidth == DCS_BF_B16;
    const size_t row = (size_t)c->n_pairs * (out16 ? 4u : 8u);
    uint64_t nc64 = out_bytes / row;
    if (nc64 > (uint64_t)c->p.nr_channels) nc64 = (uint64_t)c->p.nr_channels;
    if (nc64 == 0) return DCS_ERR_INVALID_ARGUMENT;
    const uint32_t nc = (uint32_t)nc64;
    // a buffer that holds several whole time steps is tuned as one launch of that many (up to 256, which
    // travel in the kernel arguments): the reference's own tensor is 256 small time steps, not one
    uint64_t nt64 = out_bytes / (row * nc);
    if (nt64 > kDtInline) nt64 = kDtInline;
    const uint32_t nt_tune = nc == (uint32_t)c->p.nr_channels && nt64 > 1 ? (uint32_t)nt64 : 1u;
    hipStream_t s = as_stream(stream);
    {
        const int cap = refuse_if_capturing(s); // the tuner blocks on events
        if (cap != DCS_OK) return cap;
    }
    // (which of the two variants launches of this size take: decided from the shape's default geometry, as pick_geometry does)
    dcs_bf_context::tuned_geom &slot =
        c->tuned[tuned_slot(c, out16)][want_terms_table(c, out16, shape_default_geometry(c, out16, nc, nt_tune), nc, nt_tune) ? 1 : 0];

    auto report = [&]() {
        if (!chosen) return;
        *chosen = c->tune;
        chosen->tiles_per_block = slot.tpb;
        chosen->chan_per_block = slot.cpb;
        chosen->wg_per_cu = slot.wpc;
        chosen->nontemporal = 1;
    };
    if (slot.valid) { // measured before for this context (shape) and width: dcs_bf_set_tuning(ctx, NULL) forgets it
        report();
        return DCS_OK;
    }

    struct cand { int tpb, cpb, wpc; double best_ms; }; // wpc: workgroups per CU (-1 = unlimited)
    // fp32: the short walks around the optimum, unlimited and with 5-7 workgroups per CU (fewer waves in flight
    // keep the store stream closer to address order: the best point moves to a slightly longer walk and is
    // ~1 % higher, profiles/r01_store_patterns.md); fp16: VALU-bound, long walks
    static const int k32[][3] = {{1, 6, -1}, {1, 7, -1}, {1, 8, -1}, {1, 9, -1}, {1, 10, -1}, {1, 11, -1}, {1, 12, -1}, {1, 13, -1},
                                 {1, 14, -1}, {1, 16, -1}, {1, 7, 7}, {1, 8, 7}, {1, 9, 7}, {1, 10, 7}, {1, 11, 7}, {1, 12, 7},
                                 {1, 13, 7}, {1, 7, 6}, {1, 8, 6}, {1, 9, 6}, {1, 10, 6}, {1, 11, 6}, {1, 12, 6}, {1, 13, 6},
                                 {1, 14, 6}, {1, 8, 5}, {1, 9, 5}, {1, 10, 5}, {1, 11, 5}, {1, 12, 5}, {1, 14, 5}, {1, 16, 5}, {2, 6, -1}, {2, 8, -1}};
    static const int k16[][3] = {{1, 16, -1}, {1, 24, -1}, {1, 32, -1}, {1, 48, -1}, {1, 64, -1}, {1, 96, -1}, {1, 128, -1},
                                 {1, 192, -1}, {1, 256, -1}, {1, 24, 6}, {1, 32, 6}, {1, 48, 6}, {1, 64, 6}, {1, 32, 7},
                                 {1, 64, 7}, {1, 128, 7}, {2, 32, -1}, {2, 64, -1},
                                 // the short walks under a residency cap the b16 arithmetic form peaks at (24-30 MiB held open)
                                 {1, 16, 6}, {1, 16, 7}, {1, 20, 5}, {1, 20, 6}, {1, 24, 4}, {1, 24, 5}, {1, 28, 4}, {1, 28, 5}, {1, 32, 4},
                                 {1, 32, 5}, {1, 40, 4}};
    const int(*tab)[3] = out16 ? k16 : k32;
    int ncand = out16 ? (int)(sizeof(k16) / sizeof(k16[0])) : (int)(sizeof(k32) / sizeof(k32[0]));
    cand cands[40];
    static_assert(sizeof(k32) / sizeof(k32[0]) < 40 && sizeof(k16) / sizeof(k16[0]) < 40, "cands[] too small");
    for (int i = 0; i < ncand; i++) cands[i] = {tab[i][0], tab[i][1], tab[i][2], 1e30};
    // the library's own choice for this shape always takes part (and wins ties, below)
    const bf_geom dflt = shape_default_geometry(c, out16, nc, nt_tune);
    int i_default = -1;
    for (int i = 0; i < ncand; i++)
        if (cands[i].tpb == dflt.tpb && cands[i].cpb == (int)dflt.cpb && (cands[i].wpc > 0 ? cands[i].wpc : 0) == dflt.wpc) i_default = i;
    if (i_default < 0) {
        i_default = ncand;
        cands[ncand++] = {dflt.tpb, (int)dflt.cpb, dflt.wpc > 0 ? dflt.wpc : -1, 1e30};
    }

    if (tiled_blocks(c->n_pairs, out16, dflt.tpb, dflt.cpb, nc, nt_tune) <= 256u * 8u) {
        // every workgroup of this launch is resident at once: launch-bound, nothing to tune -- the tuned
        // geometry only ever applies to launches that oversubscribe the chip (pick_geometry)
        slot.valid = true;
        slot.tpb = dflt.tpb;
        slot.cpb = (int32_t)dflt.cpb;
        slot.wpc = dflt.wpc > 0 ? dflt.wpc : -1;
        report();
        return DCS_OK;
    }
    const dcs_bf_tuning saved = c->tune;
    c->tuning_now = true;
    auto use = [&](const cand &k) {
        c->tune.form = saved.form == 2 ? 0 : saved.form; // the tiled form as production launches will run it
        c->tune.tiles_per_block = k.tpb;
        c->tune.chan_per_block = k.cpb;
        c->tune.wg_per_cu = k.wpc;
        c->tune.nontemporal = 1;
    };
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int st = (int)hipEventCreate(&e0);
    if (st == 0) st = (int)hipEventCreate(&e1);
    // After a change of access pattern the first ~20 ms of launches run 3-10 % slower than
    // steady state (profiles/r01_bench_profile.md), so every trial first settles on its own
    // geometry (untimed), then times ~3 ms worth of launches under one event pair.  Two
    // interleaved rounds; a candidate's score is its better round.
    auto time_launches = [&](int n, float *ms) -> int {
        int r = (int)hipEventRecord(e0, s);
        for (int k = 0; k < n && r == 0; k++) r = dcs_bf_generate_slab(c, bitwidth, 1, nt_tune, 0, nc, d_out, out_bytes, stream);
        if (r == 0) r = (int)hipEventRecord(e1, s);
        if (r == 0) r = (int)hipEventSynchronize(e1);
        if (r == 0) r = (int)hipEventElapsedTime(ms, e0, e1);
        return r;
    };
    float cal_ms = 0.0f;
    for (int i = 0; i < 10 && st == 0; i++) st = dcs_bf_generate_slab(c, bitwidth, 1, nt_tune, 0, nc, d_out, out_bytes, stream);
    if (st == 0) st = time_launches(4, &cal_ms);
    const double one = cal_ms > 0.0f ? cal_ms / 4.0 : 1.0; // ms per launch at the current geometry
    const int n_settle = (int)std::fmin(400.0, std::fmax(8.0, std::ceil(20.0 / one)));
    const int n_timed = (int)std::fmin(200.0, std::fmax(4.0, std::ceil(3.0 / one)));
    for (int rnd = 0; rnd < 2 && st == 0; rnd++) {
        double best_so_far = 1e30;
        for (int i = 0; i < ncand; i++) best_so_far = std::fmin(best_so_far, cands[i].best_ms);
        for (int i = 0; i < ncand && st == 0; i++) {
            // second round: only candidates within 4 % of the first round's best (the device also
            // slows by ~1 % over the first seconds of sustained load, so a short tuner is a better one)
            if (rnd == 1 && i != i_default && cands[i].best_ms > 1.04 * best_so_far) continue;
            use(cands[i]);
            for (int k = 0; k < n_settle && st == 0; k++) st = dcs_bf_generate_slab(c, bitwidth, 1, nt_tune, 0, nc, d_out, out_bytes, stream);
            float ms = 0.0f;
            if (st == 0) st = time_launches(n_timed, &ms);
            if (st == 0 && ms / n_timed < cands[i].best_ms) cands[i].best_ms = ms / n_timed;
        }
    }
    // Play-off: the short trials rank neighbours within their noise (2-3 %), so the four best and
    // the library default run again, longer (settle, then ~12 ms timed, three interleaved rounds;
    // the mean decides).  A challenger replaces the default only if it is more than 0.7 % faster:
    // below that the ranking is noise, and the default is the geometry the profiles describe.
    int order[40];
    for (int i = 0; i < ncand; i++) order[i] = i;
    for (int i = 0; i < ncand; i++) // selection sort, ncand <= 40
        for (int j = i + 1; j < ncand; j++)
            if (cands[order[j]].best_ms < cands[order[i]].best_ms) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
    int finalists[5];
    int nfinal = 0;
    for (int i = 0; i < ncand && nfinal < 4; i++)
        if (order[i] != i_default) finalists[nfinal++] = order[i];
    finalists[nfinal++] = i_default;
    double final_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int n_final = (int)std::fmin(800.0, std::fmax(8.0, std::ceil(12.0 / one)));
    for (int rnd = 0; rnd < 3 && st == 0; rnd++) {
        for (int f = 0; f < nfinal && st == 0; f++) {
            use(cands[finalists[f]]);
            for (int i = 0; i < n_settle && st == 0; i++) st = dcs_bf_generate_slab(c, bitwidth, 1, nt_tune, 0, nc, d_out, out_bytes, stream);
            float ms = 0.0f;
            if (st == 0) st = time_launches(n_final, &ms);
            final_ms[f] += ms / n_final;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    int best = i_default;
    double best_ms = final_ms[nfinal - 1] / 1.007; // what a challenger has to beat
    for (int f = 0; f + 1 < nfinal && st == 0; f++)
        if (final_ms[f] < best_ms) { best_ms = final_ms[f]; best = finalists[f]; }
    if (st == 0) {
        // leave the device settled on the chosen geometry (still under the tuner's kernel symbols)
        use(cands[best]);
        for (int k = 0; k < n_settle && st == 0; k++) st = dcs_bf_generate_slab(c, bitwidth, 1, nt_tune, 0, nc, d_out, out_bytes, stream);
    }
    c->tune = saved;
    c->tuning_now = false;
    if (st != 0) return st;
    slot.valid = true;
    slot.tpb = cands[best].tpb;
    slot.cpb = cands[best].cpb;
    slot.wpc = cands[best].wpc;
    report();
    return DCS_OK;
}

int dcs_bf_gpu_utilisation(const dcs_bf_params *p, float kernel_ms, float out[2])
{
    if (!params_ok(p) || !out) return DCS_ERR_INVALID_ARGUMENT;
    // BeamformerCoefficientTest.cu:426-430,447-448
    const float fRateOfFFTs_Hz = ((float)p->adc_sample_rate) / ((float)p->fft_size);
    const float fTransferTimePerPacket_s = 1 / fRateOfFFTs_Hz;
    float single = (kernel_ms / 1000.0) / (p->nr_samples_per_channel * fTransferTimePerPacket_s);
    float multiple = single / ((float)p->accumulations_before_new_coeffs);
    single *= 4;
    multiple *= 4;
    out[0] = single;
    out[1] = multiple;
    return DCS_OK;
}

/* ---- streaming ---------------------------------------------------------- */
// The graph holds ONE kernel node (the tiled generator for one time step of the
// slab) -- two for slabs whose pairs' terms come from the pre-pass.  A tick rewrites the
// nodes' arguments in the instantiated graph -- fDeltaTime by value, and the delay-table
// buffer when a new table has landed -- and replays it: no host synchronisation, no
// memcpy node.  A second instantiated graph has the slice gather of a device-resident
// table in front of the same nodes (dcs_bf_stream_tick_*_from_global).
namespace {

void kernel_node_params(const bf_kernel_launch &l, void **params, hipKernelNodeParams *np)
{
    std::memset(np, 0, sizeof(*np));
    np->func = const_cast<void *>(l.func);
    np->gridDim = l.grid;
    np->blockDim = l.block;
    np->sharedMemBytes = l.shared;
    np->kernelParams = params;
    np->extra = nullptr;
}

void terms_node_params(const dcs_bf_stream *s, void **params, hipKernelNodeParams *tp)
{
    std::memset(tp, 0, sizeof(*tp));
    tp->func = const_cast<void *>(s->terms_func);
    tp->gridDim = s->terms_grid;
    tp->blockDim = s->terms_block;
    tp->kernelParams = params;
}

void gather_node_params(dcs_bf_stream *s, void **params, hipKernelNodeParams *gp)
{
    bf_gather_launch &g = s->gather;
    params[0] = &g.local;
    params[1] = &g.global;
    params[2] = &g.n_ant;
    params[3] = &g.nb_local;
    params[4] = &g.nb_total;
    params[5] = &g.beam_offset;
    std::memset(gp, 0, sizeof(*gp));
    gp->func = const_cast<void *>(g.func);
    gp->gridDim = g.grid;
    gp->blockDim = g.block;
    gp->kernelParams = params;
}

// Build (gather ->) (terms ->) generator; `with_gather` selects the second graph.
int build_stream_graph(dcs_bf_stream *s, bool with_gather, hipGraph_t *graph, hipGraphExec_t *exec, hipGraphNode_t *n_gather,
                       hipGraphNode_t *n_terms, hipGraphNode_t *n_gen)
{
    DCS_TRY(hipGraphCreate(graph, 0));
    hipGraphNode_t prev = nullptr;
    if (with_gather) {
        void *gparams[6];
        hipKernelNodeParams gp;
        gather_node_params(s, gparams, &gp);
        DCS_TRY(hipGraphAddKernelNode(n_gather, *graph, nullptr, 0, &gp));
        prev = *n_gather;
    }
    if (s->has_terms) { // pre-pass node; the generator node depends on it
        void *tparams[] = {&s->terms_args};
        hipKernelNodeParams tp;
        terms_node_params(s, tparams, &tp);
        DCS_TRY(hipGraphAddKernelNode(n_terms, *graph, prev ? &prev : nullptr, prev ? 1 : 0, &tp));
        prev = *n_terms;
    }
    void *params[] = {&s->launch.args};
    hipKernelNodeParams np;
    kernel_node_params(s->launch, params, &np);
    DCS_TRY(hipGraphAddKernelNode(n_gen, *graph, prev ? &prev : nullptr, prev ? 1 : 0, &np));
    DCS_TRY(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
    return DCS_OK;
}

// Rewrite the arguments of the generator (and pre-pass) node of `exec` for this tick (fDeltaTime, the table buffer it
// reads) and replay it.
int replay(dcs_bf_stream *s, float dt, const dcs_delay_vals *delays, hipGraphExec_t exec, hipGraphNode_t n_gather,
           hipGraphNode_t n_terms, hipGraphNode_t n_gen)
{
    s->launch.args.a.dt0 = dt;
    s->launch.args.a.delays = delays;
    if (n_gather) {
        void *gparams[6];
        hipKernelNodeParams gp;
        gather_node_params(s, gparams, &gp);
        DCS_TRY(hipGraphExecKernelNodeSetParams(exec, n_gather, &gp));
    }
    if (s->has_terms) {
        s->terms_args.dt0 = dt;
        s->terms_args.dt_inline[0] = dt;
        s->terms_args.delays = delays;
        void *tparams[] = {&s->terms_args};
        hipKernelNodeParams tp;
        terms_node_params(s, tparams, &tp);
        DCS_TRY(hipGraphExecKernelNodeSetParams(exec, n_terms, &tp));
    }
    void *params[] = {&s->launch.args};
    hipKernelNodeParams np;
    kernel_node_params(s->launch, params, &np);
    DCS_TRY(hipGraphExecKernelNodeSetParams(exec, n_gen, &np));
    return (int)hipGraphLaunch(exec, s->stream);
}

// The staging machinery of a stream, created by its first dcs_bf_stream_stage_table* call (a stream that never stages
// allocates nothing more).  What a failed call created stays and is completed by the next one; dcs_bf_stream_end frees it.
int ensure_staging(dcs_bf_stream *s)
{
    if (!s->d_spare) DCS_TRY(hipMalloc((void **)&s->d_spare, (size_t)s->ctx->n_pairs * sizeof(dcs_delay_vals)));
    if (!s->stage_stream) {
        // the highest priority takes a hardware queue of its own pool: the gather must not queue behind the generator
        // kernel of the running tick, as it would on a queue the caller's stream shares
        int least = 0, greatest = 0;
        DCS_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        DCS_TRY(hipStreamCreateWithPriority(&s->stage_stream, hipStreamNonBlocking, greatest));
    }
    if (!s->staged_ev) DCS_TRY(hipEventCreateWithFlags(&s->staged_ev, hipEventDisableTiming));
    if (!s->released_ev) DCS_TRY(hipEventCreateWithFlags(&s->released_ev, hipEventDisableTiming));
    return DCS_OK;
}

// Checks shared by both staging calls; on success the internal stream may write d_spare (it has waited until no work
// queued on the caller's stream reads that buffer any more).
int begin_staging(dcs_bf_stream *s)
{
    const int cap = refuse_if_capturing(s->stream); // a cross-stream wait on the internal stream would join the capture
    if (cap != DCS_OK) return cap;
    const int st = ensure_staging(s);
    if (st != DCS_OK) return st;
    if (s->released_recorded) DCS_TRY(hipStreamWaitEvent(s->stage_stream, s->released_ev, 0));
    return DCS_OK;
}

// A tick with no table of its own while one is staged: the caller's stream waits (device side) for the staging, the
// replay reads d_spare, and only once it is enqueued does d_spare become the context's current buffer.
int consume_staged(dcs_bf_stream *s, float dt)
{
    dcs_bf_context *c = s->ctx;
    DCS_TRY(hipStreamWaitEvent(s->stream, s->staged_ev, 0));
    // everything queued so far may read the context's current buffer, nothing after this point will once it is retired
    DCS_TRY(hipEventRecord(s->released_ev, s->stream));
    s->released_recorded = true;
    const int st = replay(s, dt, s->d_spare, s->exec, nullptr, s->terms_node, s->node);
    if (st != DCS_OK) return st; // nothing committed: the context still reads its table, the staged one stays pending
    dcs_delay_vals *retired = c->d_table[c->cur];
    c->d_table[c->cur] = s->d_spare;
    s->d_spare = retired;
    s->staged = false;
    return DCS_OK;
}

// include/dcs_stream_staging.h, reached through the table at the head of every stream (bf_stream_ext.h)
int stage_table_impl(dcs_bf_stream *s, const dcs_delay_vals *table, int flags)
{
    if (!s || !table) return DCS_ERR_INVALID_ARGUMENT;
    if (flags != 0 && flags != DCS_BF_STAGE_CALLER_PINNED) return DCS_ERR_INVALID_ARGUMENT;
    dcs_bf_context *c = s->ctx;
    DCS_CHECK_DEVICE(c);
    const size_t tb = (size_t)c->n_pairs * sizeof(dcs_delay_vals);
    const int st = begin_staging(s);
    if (st != DCS_OK) return st;
    const void *src = table;
    int r = -1;
    if (flags == 0) { // through the ring of pinned buffers the host-table ticks use: the caller's array is free on return
        r = s->table_next;
        s->table_next = (r + 1) % kTableRing;
        if (s->table_pending[r]) DCS_TRY(hipEventSynchronize(s->table_copied[r])); // the copy of four stagings ago
        std::memcpy(s->h_table[r], table, tb);
        src = s->h_table[r];
    }
    DCS_TRY(hipMemcpyAsync(s->d_spare, src, tb, hipMemcpyHostToDevice, s->stage_stream));
    if (r >= 0) {
        DCS_TRY(hipEventRecord(s->table_copied[r], s->stage_stream));
        s->table_pending[r] = true;
    }
    DCS_TRY(hipEventRecord(s->staged_ev, s->stage_stream));
    s->staged = true;
    return DCS_OK;
}

int stage_table_from_global_impl(dcs_bf_stream *s, const void *d_global, uint32_t nb_total, uint32_t beam_offset,
                                 void *ready_event)
{
    if (!s || !d_global) return DCS_ERR_INVALID_ARGUMENT;
    dcs_bf_context *c = s->ctx;
    DCS_CHECK_DEVICE(c);
    if ((uint64_t)beam_offset + (uint64_t)c->p.nr_beams > nb_total) return DCS_ERR_OUT_OF_RANGE;
    if ((reinterpret_cast<uintptr_t>(d_global) & 15u) != 0) return DCS_ERR_INVALID_ARGUMENT;
    const int st = begin_staging(s);
    if (st != DCS_OK) return st;
    if (ready_event) DCS_TRY(hipStreamWaitEvent(s->stage_stream, reinterpret_cast<hipEvent_t>(ready_event), 0));
    DCS_TRY(bf_launch_gather_beams(s->d_spare, static_cast<const dcs_delay_vals *>(d_global), (uint32_t)c->p.nr_stations,
                                   (uint32_t)c->p.nr_beams, nb_total, beam_offset, s->stage_stream));
    DCS_TRY(hipEventRecord(s->staged_ev, s->stage_stream));
    s->staged = true;
    return DCS_OK;
}

const bf_stream_ext_ops kStagingOps = {BF_STREAM_EXT_VERSION, stage_table_impl, stage_table_from_global_impl};

} // namespace

int dcs_bf_stream_begin(dcs_bf_context *c, int bitwidth, uint32_t c0, uint32_t nc, void *d_out, size_t out_bytes,
                        void *stream, dcs_bf_stream **out)
{
    if (!c || !out || !d_out) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    *out = nullptr;
    if (bitwidth != DCS_BF_B16 && bitwidth != DCS_BF_B32) return DCS_ERR_INVALID_ARGUMENT;
    if (!c->table_set) return DCS_ERR_NOT_READY;
    if ((uint64_t)c0 + nc > (uint64_t)c->p.nr_channels || nc == 0) return DCS_ERR_OUT_OF_RANGE;
    const bool out16 = bitwidth == DCS_BF_B16;
    if (out_bytes < (size_t)nc * c->n_pairs * (out16 ? 4 : 8)) return DCS_ERR_INVALID_ARGUMENT;
    {
        const int cap = refuse_if_capturing(as_stream(stream)); // allocates and instantiates
        if (cap != DCS_OK) return cap;
    }

    dcs_bf_stream *s = new (std::nothrow) dcs_bf_stream();
    if (!s) return (int)hipErrorOutOfMemory;
    std::memset(static_cast<void *>(s), 0, sizeof(*s));
    s->ext.ops = &kStagingOps;
    s->ctx = c;
    s->stream = as_stream(stream);
    int st = DCS_OK;
    do {
        s->has_terms = want_terms_table(c, out16, pick_geometry(c, out16, nc, 1), nc, 1);
        if ((st = prepare_tiled(c, out16, nullptr, 0.0f, 1, c0, nc, d_out, &s->launch, nullptr, s->has_terms)) != 0) break;
        if (s->launch.func == nullptr) { st = DCS_ERR_INVALID_ARGUMENT; break; }
        if (s->has_terms) {
            fill_terms_table_args(c, out16, 0.0f, 1, c0, nc, d_out, nullptr, &s->terms_args);
            if ((st = (int)bf_prepare_terms(s->terms_args, &s->terms_func, &s->terms_grid, &s->terms_block)) != 0) break;
            if (s->terms_func == nullptr) { st = DCS_ERR_INVALID_ARGUMENT; break; }
        }
        // the gather node's launch: its pointers and the global table's width are rewritten per tick, the grid never changes
        if ((st = (int)bf_prepare_gather_beams(c->d_table[c->cur ^ 1], c->d_table[c->cur], (uint32_t)c->p.nr_stations,
                                               (uint32_t)c->p.nr_beams, (uint32_t)c->p.nr_beams, 0u, &s->gather)) != 0) break;
        if (s->gather.func == nullptr) { st = DCS_ERR_INVALID_ARGUMENT; break; }
        for (int i = 0; i < kTableRing && st == 0; i++) {
            st = (int)hipHostMalloc((void **)&s->h_table[i], (size_t)c->n_pairs * sizeof(dcs_delay_vals), hipHostMallocDefault);
            if (st == 0) st = (int)hipEventCreateWithFlags(&s->table_copied[i], hipEventDisableTiming);
        }
        if (st != 0) break;
        if ((st = build_stream_graph(s, false, &s->graph, &s->exec, nullptr, &s->terms_node, &s->node)) != 0) break;
        if ((st = build_stream_graph(s, true, &s->ggraph, &s->gexec, &s->gnode_gather, &s->gnode_terms, &s->gnode_gen)) != 0) break;
    } while (0);
    if (st != 0) {
        dcs_bf_stream_end(s);
        return st;
    }
    *out = s;
    return DCS_OK;
}

int dcs_bf_stream_tick_dt(dcs_bf_stream *s, float dt, const dcs_delay_vals *new_table)
{
    if (!s) return DCS_ERR_INVALID_ARGUMENT;
    dcs_bf_context *c = s->ctx;
    DCS_CHECK_DEVICE(c);
    if (s->staged) return new_table ? DCS_ERR_INVALID_ARGUMENT : consume_staged(s, dt);
    if (new_table) {
        // stage through pinned memory into the IDLE table buffer; replays already
        // queued keep reading the current one (their arguments are baked in)
        const int r = s->table_next;
        s->table_next = (r + 1) % kTableRing;
        if (s->table_pending[r]) DCS_TRY(hipEventSynchronize(s->table_copied[r])); // the copy of four updates ago
        std::memcpy(s->h_table[r], new_table, (size_t)c->n_pairs * sizeof(dcs_delay_vals));
        const int nxt = c->cur ^ 1;
        DCS_TRY(hipMemcpyAsync(c->d_table[nxt], s->h_table[r], (size_t)c->n_pairs * sizeof(dcs_delay_vals),
                               hipMemcpyHostToDevice, s->stream));
        DCS_TRY(hipEventRecord(s->table_copied[r], s->stream));
        s->table_pending[r] = true;
        c->cur = nxt;
    }
    return replay(s, dt, c->d_table[c->cur], s->exec, nullptr, s->terms_node, s->node);
}

int dcs_bf_stream_tick(dcs_bf_stream *s, uint64_t t, const dcs_delay_vals *new_table)
{
    if (!s) return DCS_ERR_INVALID_ARGUMENT;
    float dt;
    const int st = dcs_bf_delta_times(&s->ctx->p, t, 1, &dt);
    if (st != DCS_OK) return st;
    return dcs_bf_stream_tick_dt(s, dt, new_table);
}

int dcs_bf_stream_tick_at(dcs_bf_stream *s, const struct timespec *cur, const struct timespec *ref,
                          const dcs_delay_vals *new_table)
{
    if (!s) return DCS_ERR_INVALID_ARGUMENT;
    float dt;
    const int st = dcs_bf_ts_diff(ref, cur, &dt);
    if (st != DCS_OK) return st;
    return dcs_bf_stream_tick_dt(s, dt, new_table);
}

int dcs_bf_stream_tick_dt_from_global(dcs_bf_stream *s, float dt, const void *d_global, uint32_t nb_total, uint32_t beam_offset)
{
    if (!s || !d_global) return DCS_ERR_INVALID_ARGUMENT;
    dcs_bf_context *c = s->ctx;
    DCS_CHECK_DEVICE(c);
    if ((uint64_t)beam_offset + (uint64_t)c->p.nr_beams > nb_total) return DCS_ERR_OUT_OF_RANGE;
    if ((reinterpret_cast<uintptr_t>(d_global) & 15u) != 0) return DCS_ERR_INVALID_ARGUMENT;
    if (s->staged) return DCS_ERR_INVALID_ARGUMENT; // a staged table is pending: the next plain tick takes it
    // the gather node writes the IDLE table buffer (replays already queued read the current one), the nodes
    // behind it read it: all inside one graph launch, ordered by the graph's edges
    const int nxt = c->cur ^ 1;
    s->gather.local = c->d_table[nxt];
    s->gather.global = static_cast<const dcs_delay_vals *>(d_global);
    s->gather.nb_total = nb_total;
    s->gather.beam_offset = beam_offset;
    c->cur = nxt;
    return replay(s, dt, c->d_table[c->cur], s->gexec, s->gnode_gather, s->gnode_terms, s->gnode_gen);
}

int dcs_bf_stream_tick_from_global(dcs_bf_stream *s, uint64_t t, const void *d_global, uint32_t nb_total, uint32_t beam_offset)
{
    if (!s) return DCS_ERR_INVALID_ARGUMENT;
    float dt;
    const int st = dcs_bf_delta_times(&s->ctx->p, t, 1, &dt);
    if (st != DCS_OK) return st;
    return dcs_bf_stream_tick_dt_from_global(s, dt, d_global, nb_total, beam_offset);
}

int dcs_bf_stream_tick_at_from_global(dcs_bf_stream *s, const struct timespec *cur, const struct timespec *ref,
                                      const void *d_global, uint32_t nb_total, uint32_t beam_offset)
{
    if (!s) return DCS_ERR_INVALID_ARGUMENT;
    float dt;
    const int st = dcs_bf_ts_diff(ref, cur, &dt);
    if (st != DCS_OK) return st;
    return dcs_bf_stream_tick_dt_from_global(s, dt, d_global, nb_total, beam_offset);
}

int dcs_bf_stream_end(dcs_bf_stream *s)
{
    if (!s) return DCS_OK;
    (void)hipStreamSynchronize(s->stream);
    // the staging machinery: a table staged but never consumed is dropped with the buffer that holds it -- the one buffer
    // the stream owns now (the context's two, whichever they are after exchanges, stay the context's)
    if (s->stage_stream) {
        (void)hipStreamSynchronize(s->stage_stream);
        (void)hipStreamDestroy(s->stage_stream);
    }
    if (s->staged_ev) (void)hipEventDestroy(s->staged_ev);
    if (s->released_ev) (void)hipEventDestroy(s->released_ev);
    if (s->d_spare) (void)hipFree(s->d_spare);
    if (s->exec) (void)hipGraphExecDestroy(s->exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    if (s->gexec) (void)hipGraphExecDestroy(s->gexec);
    if (s->ggraph) (void)hipGraphDestroy(s->ggraph);
    for (int i = 0; i < kTableRing; i++) {
        if (s->table_copied[i]) (void)hipEventDestroy(s->table_copied[i]);
        if (s->h_table[i]) (void)hipHostFree(s->h_table[i]);
    }
    delete s;
    return DCS_OK;
}

#ifdef DCS_PROBES
/* include/dcs_probes.h -- the probes build only */
int dcs_probe_set_knobs(dcs_bf_context *c, const dcs_probe_knobs *k)
{
    if (!c) return DCS_ERR_INVALID_ARGUMENT;
    if (!k) {
        std::memset(&c->probe, 0, sizeof(c->probe));
        return DCS_OK;
    }
    if (k->pace < 0 || k->pace > 4096 || k->fail_at_step < 0) return DCS_ERR_INVALID_ARGUMENT;
    c->probe = *k;
    return DCS_OK;
}
#endif

} // extern "C"
