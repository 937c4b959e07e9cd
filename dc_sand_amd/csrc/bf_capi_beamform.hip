// bf_capi_beamform.hip -- both beamformers of include/dcs_beamformer.h, and their weighted, quantised, detecting and
// complex-product calls (bf_ctx_ext.h): the terms table and its class words, the terms pre-pass, the launches.  Host code only; the
// kernels are in bf_kernels.hip and bf_beamform_mfma.hip.  A call behind the table begins with the device-free checks of its
// entry (bf_arg_checks.h), the ones its companion has made already; beamform_impl and beamform_acc_impl keep all of their own,
// since this library's exports call them directly.

#include <cstdlib>
#include <cstring>

#include "bf_host.h"

using namespace bf_host;

namespace {

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

} // namespace

namespace bf_host {

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

} // namespace bf_host

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

namespace {
// What a call of the matrix-core beamformer writes to d_beams, and what it applies on the way.  kFloat: the beams, (re, im)
// fp32 per sample; kInt8: the same quantised (include/dcs_beam_quant.h), a quarter the size; kBlockPower: one float per beam
// and 16-sample block (include/dcs_beam_power.h), 4-byte aligned.  complex: the true complex product instead of the
// element-wise one (include/dcs_beam_complex.h); with kInt8, include/dcs_beam_complex_quant.h.
struct bacc_output {
    enum { kFloat, kInt8, kBlockPower } kind;
    const float *d_weights; // nullptr (unweighted) or [B][A] fp32 weights in device memory (include/dcs_beam_weights.h)
    bf_quant_args quant;    // kInt8 only: the quantiser's gains and counters
    const bf_complex_args *complex = nullptr;
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
    if ((out.d_weights || out.kind != bacc_output::kFloat || out.complex) && (c->tune.math_mode & 8)) return DCS_ERR_UNSUPPORTED; // the fp32 fma-chain form has no weights, no quantiser, no detector, no complex product
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
                                       out.kind == bacc_output::kBlockPower, out.complex, s);
}

} // namespace

namespace bf_host {

// include/dcs_beam_weights.h, reached through the table at the head of every context (bf_ctx_ext.h)
int generate_and_beamform_weighted_impl(dcs_bf_context *c, const float *dt, uint64_t t0, uint32_t nt, const int8_t *d_antenna,
                                        size_t antenna_bytes, const float *d_weights, float *d_beams, size_t beams_bytes,
                                        void *stream)
{
    if (int e = generate_and_beamform_weighted_args(c, dt, t0, nt, d_weights)) return e;
    return beamform_impl(c, dt_or_index(dt, t0), nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream, d_weights);
}

int beamform_accumulated_weighted_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                       const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, float *d_beams,
                                       size_t beams_bytes, void *stream)
{
    if (int e = beamform_accumulated_weighted_args(c, nt, d_weights)) return e;
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_beams, beams_bytes,
                             stream, {bacc_output::kFloat, d_weights, {}});
}

// include/dcs_beam_quant.h, reached the same way
int beamform_accumulated_q8_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                 size_t antenna_bytes, const float *d_weights, const float *d_quant_gains, int8_t *d_beams_q8,
                                 size_t beams_bytes, unsigned long long *d_clip_count, void *stream)
{
    if (int e = beamform_accumulated_q8_args(c, nt, d_weights, d_quant_gains, d_clip_count)) return e;
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_beams_q8, beams_bytes,
                             stream, {bacc_output::kInt8, d_weights, {d_quant_gains, d_clip_count}});
}

// include/dcs_beam_power.h, reached the same way
int beamform_accumulated_power_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                    size_t antenna_bytes, const float *d_weights, float *d_block_power, size_t power_bytes,
                                    void *stream)
{
    if (int e = beamform_accumulated_power_args(c, nt, d_weights, d_block_power)) return e;
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_block_power, power_bytes,
                             stream, {bacc_output::kBlockPower, d_weights, {}});
}

// include/dcs_beam_complex.h, reached the same way: the float call and the detecting call with the true complex product
int beamform_accumulated_complex_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt, const int8_t *d_antenna,
                                      size_t antenna_bytes, const float *d_weights, uint32_t flags, float *d_beams, size_t beams_bytes,
                                      void *stream)
{
    if (int e = beamform_accumulated_complex_args(c, nt, d_weights, flags, d_beams)) return e;
    const bf_complex_args cx = {flags & DCS_BF_COMPLEX_CONJ};
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_beams, beams_bytes, stream,
                             {bacc_output::kFloat, d_weights, {}, &cx});
}

int beamform_accumulated_complex_power_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                            const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                            float *d_block_power, size_t power_bytes, void *stream)
{
    if (int e = beamform_accumulated_complex_power_args(c, nt, d_weights, flags, d_block_power)) return e;
    const bf_complex_args cx = {flags & DCS_BF_COMPLEX_CONJ};
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_block_power, power_bytes, stream,
                             {bacc_output::kBlockPower, d_weights, {}, &cx});
}

// include/dcs_beam_complex_quant.h, reached the same way: the complex product's floats quantised in the kernel's epilogue
int beamform_accumulated_complex_q8_impl(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                         const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights, uint32_t flags,
                                         const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                         unsigned long long *d_clip_count, void *stream)
{
    if (int e = beamform_accumulated_complex_q8_args(c, nt, d_weights, flags, d_quant_gains, d_beams_q8, d_clip_count)) return e;
    const bf_complex_args cx = {flags & DCS_BF_COMPLEX_CONJ};
    return beamform_acc_impl(c, dt_or_index(dt_coeff, t_coeff), nt, d_antenna, antenna_bytes, d_beams_q8, beams_bytes, stream,
                             {bacc_output::kInt8, d_weights, {d_quant_gains, d_clip_count}, &cx});
}

} // namespace bf_host

extern "C" {

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

} // extern "C"
