// bf_capi_stream.hip -- the streams of include/dcs_beamformer.h (dcs_bf_stream_*) and the staging calls behind
// include/dcs_stream_staging.h (bf_stream_ext.h).  Host code only; the kernels are in bf_kernels.hip.

#include <cstring>
#include <new>

#include "../../include/dcs_stream_staging.h" // DCS_BF_STAGE_CALLER_PINNED
#include "bf_stream_ext.h"
#include "bf_host.h"

using namespace bf_host;

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

extern "C" {

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

} // extern "C"
