// bf_kernels.h -- host-callable launchers of the gfx950 kernels in
// bf_kernels.hip (internal to libdcs_beamformer.so; the public boundary is
// include/dcs_beamformer.h).
#ifndef DCS_BF_KERNELS_H
#define DCS_BF_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf_math.h"

// One tiled launch: time steps [0, nt) x channels [c0, c0+nc) x all pairs.
struct bf_tiled_args {
    const dcs_delay_vals *delays; // compact table [n_pairs]
    void *out;                    // [nt][nc][n_pairs] of {re,im} (fp32 pair or half2)
    const float *dt_dev;          // fDeltaTime per time step (device), or nullptr
    float dt0;                    // used when dt_dev == nullptr and nt == 1
    uint32_t n_pairs;
    uint32_t c0, nc;              // channel slab
    uint32_t nt;
    uint32_t chan_per_block;      // channels a workgroup walks
    uint32_t n_tile_groups;       // ceil(n_pairs / pairs per workgroup)
    uint32_t n_cblocks;           // ceil(nc / chan_per_block)
    uint32_t xcd_remap;           // workgroups sharing blockIdx % 8 (one XCD) take consecutive (tile, channel block)s
#ifdef DCS_PROBES
    uint32_t pace;                // probes build only: 64-cycle sleeps before each store of the fast loop
#endif
    dcs_bf_consts k;
    // terms-table variant (nullptr: the workgroups compute and stage their pairs' terms themselves):
    const float *terms;           // [nt][pairs_pad][2], written by bf_launch_terms just before
    const uint32_t *flags;        // [nt][pairs_pad/64]
    uint32_t pairs_pad;
};
// The same with fDeltaTime of up to kDtInline time steps by value (kernel arguments): the reference's
// default tensor (256 time steps, 134 MB) is a 22 us kernel, and a pinned->device copy of the dt table
// in front of it cost another 9 us.  Used when a.dt_dev == nullptr and a.nt > 1; dt_inline[0] == a.dt0.
// One-time-step launches (the per-time-step host loops of NAIVE / MULTIPLE_CHANNELS, every streaming
// tick) take the 0.1 KiB bf_tiled_args alone: those loops are bound by the host's launch rate.
constexpr uint32_t kDtInline = 256;
struct bf_tiled_args_inl {
    bf_tiled_args a;
    float dt_inline[kDtInline];
};

// A resolved launch (kernel instantiation, geometry, final arguments): what
// bf_launch_tiled enqueues, and what a hipGraph kernel node is built from.
struct bf_kernel_launch {
    const void *func; // nullptr: nothing to launch (empty shape)
    dim3 grid, block;
    uint32_t shared; // dynamic LDS bytes requested (occupancy limiter; the kernel does not use them)
    bf_tiled_args_inl args; // the kernel's parameter is `args` (inline form) or `args.a` (same address)
};
// dt_inline: nullptr, or a.nt values (a.nt <= kDtInline) that travel in the kernel arguments
hipError_t bf_prepare_tiled(const bf_tiled_args &a, const float *dt_inline, bool out16, int tiles_per_block,
                            bool nontemporal, bf_kernel_launch *out);

// Row-streaming form: a terms table written by bf_launch_terms, then one short
// wave per (1-KiB tile, rows_per_wave channel rows).
struct bf_terms_args {
    const dcs_delay_vals *delays; // [n_pairs]
    float *terms;                 // [nt][pairs_pad][2]
    uint32_t *flags;              // [nt][pairs_pad/64]
    const float *dt_dev;          // or nullptr -> dt_inline (nt <= kTermsInline; dt_inline[0] == dt0)
    float dt0;
    uint32_t n_pairs, pairs_pad, nt;
    dcs_bf_consts k;
    float dt_inline[8];
    // slow-path duty (tiled form's terms-table variant; nullptr otherwise): the output tensor
    // [nt][nc][n_pairs] of {re,im} and its channel slab, as in bf_tiled_args
    void *out;
    uint32_t c0, nc, out16;
};
constexpr uint32_t kTermsInline = 8;
hipError_t bf_launch_terms(const bf_terms_args &a, hipStream_t stream);
// the same launch resolved but not enqueued (a hipGraph kernel node is built from it); *func == nullptr: nothing to launch
hipError_t bf_prepare_terms(const bf_terms_args &a, const void **func, dim3 *grid, dim3 *block);

struct bf_rows_args {
    const float *terms;
    const uint32_t *flags;
    void *out; // [nt][nc][n_pairs]
    uint32_t n_pairs, pairs_pad;
    uint32_t c0, nc, nt;
    uint32_t n_colgroups, n_rowgroups; // filled by the launcher
    uint32_t xcd_remap;
    uint32_t div3; // dcs_bf_consts::uDiv3Exact
    uint32_t same_tile; // the workgroup's waves share one tile and interleave rows
#ifdef DCS_PROBES
    uint32_t pace;      // probes build only: 64-cycle sleeps before each store
#endif
    uint32_t lds_pad;   // host only: dynamic LDS the launch asks for (occupancy limiter, unused by the kernel)
    float D, y;
};
hipError_t bf_launch_rows(const bf_rows_args &a, bool out16, int waves_per_block, int rows_per_wave,
                          bool nontemporal, bool xcd_remap, bool nomath, hipStream_t stream);

// Fused coefficient generation + beamforming (table indexed [b*A + a]).
struct bf_bform_terms_args {
    const dcs_delay_vals *delays; // [B][A]
    float *terms;                 // [nt][A][B][2]
    uint32_t *flags;              // [nt]: atomicMax of (epoch << 2) | class; words of earlier epochs count as the lowest class
    uint32_t epoch;               // this call's number (1 .. 2^30 - 2), from the context
    const float *dt_dev;          // [nt], or nullptr: nt == 1 and fDeltaTime is dt0 (by value: nothing to stage)
    float dt0;
    uint32_t n_pairs, A, B, nt;
    dcs_bf_consts k;
};
struct bf_bform_terms_args_inl {
    bf_bform_terms_args a;
    float dt_inline[kDtInline];
};
// dt_inline: nullptr (fDeltaTime from a.dt_dev, or a.dt0 when nt == 1), or a.nt <= kDtInline values that travel in the
// kernel arguments
hipError_t bf_launch_bform_terms(const bf_bform_terms_args &a, const float *dt_inline, hipStream_t stream);

// Per-input beam weights (include/dcs_beam_weights.h).  The weighted pre-pass reads the caller's
// g[b][a] and, besides the terms, writes for the beamformers ghat[a][b] = g[b][a] / s_b (the terms table's [A][B] order)
// and s_b = max_a |g[b][a]| per beam (NaN when a weight of the beam is not finite); the terms of a pair whose weight is 0
// are written as (0, 0), so that antenna's coefficient is finite (1, 0) whatever its delay values are.
struct bf_weights_args {
    const float *g; // [B][A], the caller's weights (device)
    float *gn;      // [A][B]: ghat
    float *gs;      // [B]: s_b
};
// words[0 .. n) = 0: the class words of a call's time steps (clear_class_words, bf_capi.hip)
hipError_t bf_launch_clear_words(uint32_t *words, uint32_t n, hipStream_t stream);
// The weighted form of bf_launch_bform_terms: one more row of workgroups makes gn and gs
hipError_t bf_launch_bform_terms_weighted(const bf_bform_terms_args &a, const bf_weights_args &w, const float *dt_inline,
                                          hipStream_t stream);

struct bf_beamform_args {
    const float *terms;    // [nt16*16][A][B][2] for this launch's time steps
    const uint32_t *flags; // [nt16*16], epoch-tagged (bf_bform_terms_args)
    uint32_t epoch;
    const int8_t *ant;     // [C][nt16_total][A][16][2]
    float *beams;          // [C][nt16_total][B][16][2]
    uint32_t A, B, C;
    uint32_t nt16;         // 16-sample blocks in this launch
    uint32_t tex0;         // first of them within the whole tensor
    uint32_t nt16_total;
    uint32_t chan_per_block;
    uint32_t n_bgroups, n_cblocks; // filled by the launcher
    dcs_bf_consts k;
};
// w: nullptr, or the weights: w->gn, w->gs as bf_launch_bform_terms_weighted wrote them (w->g unused)
hipError_t bf_launch_beamform(const bf_beamform_args &a, const bf_weights_args *w, hipStream_t stream);

// Beamformer with coefficient reuse on the matrix cores (bf_beamform_mfma.hip): the coefficients of ONE time
// (terms table [A][B] from bf_launch_bform_terms with nt = 1) applied to nT16 blocks of 16 samples.
struct bf_bacc_args {
    const float *terms;    // [A][B][2]
    const uint32_t *flags; // [1]: (epoch << 2) | highest pair class of the table
    uint32_t epoch;
    const int8_t *ant;     // [C][nT16][A][16][2]
    float *beams;          // [C][nT16][B][16][2]
    uint32_t A, B, C, nT16;
    uint32_t fp32_chain;   // 0: exact fixed-point contraction on the int8 matrix pipe; 1: fp32 fma chain (v_mfma_f32_16x16x4_f32)
    uint32_t share_off;    // staged int8 form: LDS offset of the coefficient exchange (filled by the launcher; 0 = none)
#ifdef DCS_PROBES
    // A/B switches of the measurements in profiles/r02_fused.md / r03_fused.md (include/dcs_probes.h: dcs_probe_knobs);
    // the product build has none of them -- BACC_KNOB() below reads as a constant 0 there
    uint32_t max_rounds;   // cap on the rounds of sample blocks per workgroup (0 = the launcher's choice)
    uint32_t no_share;     // staged int8 form: every wave makes all its coefficients
    uint32_t plain_stores; // int8 form: ordinary instead of nontemporal stores
    uint32_t wg_per_cu;    // staged int8 form: at most this many workgroups resident per CU (0 = as many as fit)
    uint32_t unstaged;     // int8 form, <= 64 antennas: operands straight from global memory instead of through LDS
    uint32_t order;        // workgroup numbering: 0 = the launcher's choice, 1 = as dispatched (round 2), 2 = a contiguous eighth per XCD, 3 = sharers always grouped
    uint32_t nbt_force;    // staged form: beam tiles per workgroup (1, 2, 4, 8; 0 = the launcher's choice)
    uint32_t nw_force;     // staged form: waves per workgroup (8, 16; 0 = the launcher's choice)
    uint32_t probe;        // 1 = stores only, 2 = loads and stores without arithmetic, 3 = stores without coefficients either,
                           // 4 = as 3 with one contiguous KiB per store instruction
#endif
    uint32_t tiles_per_wg, n_bgroups, n_tgroups, nbt_log2, xcd_group; // filled by the launcher
    dcs_bf_consts k;
};
// Dispatch number -> logical workgroup number that puts G consecutive logical workgroups on ONE XCD (the hardware deals
// workgroup w to XCD w % 8) while the eight XCDs work on eight neighbouring groups: XCD x = w % 8's q-th workgroup
// (q = w / 8) is member q % G of group (q / G) * 8 + x.  A bijection of [0, total): by construction on the whole multiples
// of 8 G, identity on the tail and for G <= 1.  (bf_beamform_mfma.hip says when it is used.)
__host__ __device__ inline uint32_t bf_xcd_grouped(uint32_t w, uint32_t total, uint32_t G)
{
    if (G <= 1u) return w;
    const uint32_t full = total - total % (8u * G);
    if (w >= full) return w;
    const uint32_t x = w & 7u, q = w >> 3;
    return ((q / G) * 8u + x) * G + q % G;
}

#ifdef DCS_PROBES
#define BACC_KNOB(a, f) ((a).f)
#else
#define BACC_KNOB(a, f) 0u
#endif
// Quantised int8 beam output (include/dcs_beam_quant.h): a.beams is then the int8 tensor
// [C][nT16][B][16][2], written by the quantised kernels' epilogue from the floats the float kernels would have stored
struct bf_quant_args {
    const float *gains;        // [B]: the beams' quantisation gains (device)
    unsigned long long *clips; // [B]: clipped components per beam, added to; or nullptr: no counting
};
// The true complex product sum_a w_a x_a instead of the element-wise one (include/dcs_beam_complex.h; DESIGN.md section
// 5.13): a kernel argument of its own, so that bf_bacc_args -- and with it every other kernel -- stays as it is
struct bf_complex_args {
    uint32_t conj; // non-zero: sum_a conj(w_a) x_a
};
// w: nullptr, or the weights as for bf_launch_beamform; q: nullptr, or the quantiser; power: detected beam power
// (include/dcs_beam_power.h): a.beams is then the block power tensor [C][nT16][B], one float per beam
// and 16-sample block, written by the detecting kernels' epilogue from the floats the float kernels would have stored;
// cx: nullptr, or the complex product.  All four exist for the int8 form's kStaged and kChain only (a.fp32_chain must be
// 0), and q excludes power (q with cx: include/dcs_beam_complex_quant.h).
hipError_t bf_launch_beamform_acc(const bf_bacc_args &a, const bf_weights_args *w, const bf_quant_args *q, bool power,
                                  const bf_complex_args *cx, hipStream_t stream);
hipError_t bf_warm_module_mfma();

// The incoherent beam (bf_incoherent.hip; include/dcs_incoherent_beam.h): the sample tensor as
// rows = C * nT16 rows of A * 32 bytes, each summed to one exact dword of block_power [C][nT16]
struct bf_incoh_args {
    const int8_t *ant;     // [rows][A][16][2], 16-byte aligned
    const float *weights;  // nullptr (every antenna), or [A] flags: antenna a takes part iff weights[a] != 0
    uint32_t *block_power; // [rows]
    uint64_t rows;
    uint64_t n_groups;     // filled by the launcher: groups of rows that a wave carries at once
    uint32_t A;            // 1 .. 256
};
hipError_t bf_launch_incoherent_power(const bf_incoh_args &a, hipStream_t stream);
hipError_t bf_warm_module_incoherent();

// Full-Stokes detection (bf_stokes.hip; include/dcs_stokes.h): two int8 beam tensors as
// rows = C * nT16 * B rows of 32 bytes each, every row pair reduced to nr_stokes exact dwords of block_stokes [C][nT16][B][nr_stokes]
struct bf_stokes_args {
    const int8_t *beams_x; // [rows][16][2], 16-byte aligned; polarisation x
    const int8_t *beams_y; // the same of polarisation y; may be beams_x
    int32_t *block_stokes; // [rows][nr_stokes], aligned to 4 * nr_stokes bytes
    uint64_t rows;
    uint64_t n_groups;     // filled by the launcher: groups of rows that a wave carries at once
    uint32_t nr_stokes;    // 1 (I) or 4 (I, Q, U, V)
};
hipError_t bf_launch_stokes_block(const bf_stokes_args &a, hipStream_t stream);
hipError_t bf_warm_module_stokes();

// The integrator of every post-detection output (bf_integrate.hip): blocks [C][nr_blocks][bs] summed
// n at a time into out [nr_blocks / n][C][bs].  The element type selects the rule: float words are added in order, one rounded
// add each; 32-bit integer words exactly, in 64 bits, and the sum converted once
enum bf_integrate_type { BF_INTEGRATE_F32, BF_INTEGRATE_U32 /* built for bs == 1 */, BF_INTEGRATE_I32 };
struct bf_integrate_args {
    const void *blocks;  // words of the type the launch names
    float *out;
    uint64_t total;      // (nr_blocks / n) * C * bs
    uint32_t bs;         // words per (channel, block): B; 1; B * nr_stokes; A (A + 1)
    uint32_t C;
    uint32_t nr_blocks;  // a multiple of n
    uint32_t n;          // blocks per output row, >= 1
    uint32_t accumulate; // non-zero: float sums start from what out holds, integer sums are added to it once rounded
};
hipError_t bf_launch_integrate(bf_integrate_type type, const bf_integrate_args &a, hipStream_t stream);
hipError_t bf_warm_module_integrate();

// Incoherent dedispersion (bf_dedisperse.hip; include/dcs_dedisperse.h).
// The delay table int32 [nr_dm][C] of a band and DMs, in fp64 rounded once per operation
struct bf_dmdelay_args {
    const double *dms; // [nr_dm], 8-byte aligned; read when the work runs
    int32_t *delays;   // [nr_dm][C]
    uint64_t total;    // nr_dm * C
    uint32_t C;
    double freq_first, freq_step, sample_time;
};
hipError_t bf_launch_dm_delays(const bf_dmdelay_args &a, hipStream_t stream);
// Filterbanks uint8 [B][in_spectra][C] shifted by the table and summed over the columns into out uint32 [B][nr_dm][out_spectra],
// words first_out .. first_out + T - 1 of every series
struct bf_dedisp_args {
    const uint8_t *in;     // 16-byte aligned
    const int32_t *delays; // [nr_dm][C]; read when the work runs; an entry outside [0, max_delay] drops its term
    const uint8_t *mask;   // nullptr (every column), or [C]: a zero byte drops the column
    uint32_t *out;
    uint64_t in_spectra, first, out_spectra, first_out;
    uint32_t C, B, T, nr_dm, max_delay;
    uint32_t t_tiles, dm_tiles; // filled by the launcher: tiles of output times and of DMs
};
hipError_t bf_launch_dedisperse(const bf_dedisp_args &a, hipStream_t stream);
hipError_t bf_warm_module_dedisperse();

// The single-pulse search on the DM-time planes (bf_single_pulse.hip; include/dcs_single_pulse.h).
// A series is one (beam, DM) pair: series s begins at word s * plane_spectra of the planes.
// {sum x, sum x^2 mod 2^64} of words first .. first + T - 1 of every series
struct bf_dtsums_args {
    const uint32_t *plane; // [series][plane_spectra]
    uint64_t *sums;        // [series][2]
    uint64_t plane_spectra, first;
    uint32_t T;
    uint32_t accumulate;   // non-zero: added to what sums holds
};
hipError_t bf_launch_dm_time_sums(const bf_dtsums_args &a, uint64_t series, hipStream_t stream);
// Per series, width index i and block k of block_len times: {the largest boxcar sum of width widths[i], its first time} into
// peaks [series][nr_widths][peak_blocks][2] at block first_block + k; {0, 0xffffffff} for a width outside [1, max_width]
struct bf_boxcar_args {
    const uint32_t *plane;  // [series][plane_spectra]; words first .. first + T + max_width - 2 of a series are read
    const uint32_t *widths; // [nr_widths]; read when the work runs
    uint32_t *peaks;
    uint64_t plane_spectra, first, peak_blocks, first_block;
    uint32_t T, nr_widths, max_width, block_len;
    uint32_t run;           // filled by the launcher: blocks that a workgroup takes, one after the other
    uint32_t segments;      // filled by the launcher: such runs per series
};
hipError_t bf_launch_boxcar_peaks(const bf_boxcar_args &a, uint64_t series, hipStream_t stream);
// Peaks and sums -> snr [series][nr_widths][peak_blocks] and best [series][peak_blocks], blocks first_block .. + nr_blocks - 1
struct bf_peaksnr_args {
    const uint32_t *peaks;
    const uint32_t *widths;
    const uint64_t *sums;
    float *snr;
    uint32_t *best;         // nullptr: not wanted
    uint64_t peak_blocks, first_block, count;
    uint64_t total;         // series * nr_blocks
    uint32_t nr_blocks, nr_widths, max_width;
};
hipError_t bf_launch_peak_snr(const bf_peaksnr_args &a, hipStream_t stream);
hipError_t bf_warm_module_single_pulse();

// The correlator (bf_correlator.hip; include/dcs_correlator.h): the sample tensor
// [C][nT16][A][16][2] -> exact visibilities int32 [C][nr_vis][NB][2] of the pairs b <= a, each summed over n blocks
struct bf_corr_args {
    const int8_t *ant; // 16-byte aligned
    int32_t *vis;      // 8-byte aligned
    uint64_t NB;       // filled by the launcher: A (A + 1) / 2
    uint64_t items;    // filled by the launcher: C * nr_vis * units
    uint32_t A;        // 1 .. 256
    uint32_t C;
    uint32_t nT16;     // blocks of the tensor, >= nr_vis * n
    uint32_t n;        // blocks per visibility, 1 .. 4095
    uint32_t nr_vis;
    uint32_t tiles;    // filled by the launcher: 16-antenna tiles
    uint32_t st;       // filled by the launcher: squares of 4 x 4 tiles along the diagonal
    uint32_t units;    // filled by the launcher: units (the tile pairs a wave takes at once) per (channel, visibility)
};
hipError_t bf_launch_correlate(const bf_corr_args &a, hipStream_t stream);
hipError_t bf_warm_module_correlator();

// The digital down-converter (bf_ddc.hip; include/dcs_ddc.h): real int8 [nr_inputs][in_stride] ->
// float [band][input][out_stride][{re, im}], nr_out outputs per row, output m from samples 16 m .. 16 m + T - 1
struct bf_ddc_digits_args {
    const int32_t *taps; // [band][T][{re, im}]
    int8_t *digits;      // 16 T bytes, 16-byte aligned
    uint32_t T;          // 64, 128, 192, 256
    uint32_t nr_bands;   // 1, 2
};
hipError_t bf_launch_ddc_tap_digits(const bf_ddc_digits_args &a, hipStream_t stream);
struct bf_ddc_args {
    const int8_t *x;      // 16-byte aligned
    const int8_t *digits; // the table of bf_launch_ddc_tap_digits for (T, nr_bands)
    float *out;           // 8-byte aligned
    uint64_t in_stride;   // bytes, % 16 == 0, >= 16 (nr_out - 1) + T
    uint64_t out_stride;  // pairs, >= nr_out
    uint64_t items;       // filled by the launcher: nr_inputs * spans
    uint32_t nr_inputs;
    uint32_t nr_out;
    uint32_t T;
    uint32_t nr_bands;
    uint32_t spans;       // filled by the launcher: the spans of outputs of a row, one workgroup each
    uint32_t u0[2];       // per band: the phase word of output 0 of the call
    uint32_t step16[2];   // per band: 16 phase_step, the phase step per output
    float gain[2];
};
hipError_t bf_launch_ddc(const bf_ddc_args &a, hipStream_t stream);
hipError_t bf_warm_module_ddc();

// The candidate sifter (bf_candidates.hip; include/dcs_candidates.h): the cells (beam, DM, block)
// of blocks first_block .. first_block + nr_blocks - 1 at or above threshold that no cell within the two radii beats, as
// records of eight words in ascending (beam, DM, block).  A segment is a row of a tile: kCandTileBlocks cells of one DM
struct bf_cand_args {
    const float *snr;      // [B][nr_dm][nr_widths][peak_blocks]
    const uint32_t *peaks; // [B][nr_dm][nr_widths][peak_blocks][2], 8-byte aligned
    uint32_t *cands;       // [max_candidates][8], 8-byte aligned; nullptr where max_candidates == 0
    uint32_t *count;       // {found, written}
    uint64_t *marks;       // the workspace: [segments] ballots of the candidates ...
    uint32_t *places;      // ... and [segments] counts, which the scan makes the segments' first places in the list
    uint64_t peak_blocks, first_block;
    uint64_t segments;     // B * nr_dm * k_tiles < 2^32
    uint32_t B, nr_dm, nr_blocks, nr_widths, dm_radius, block_radius, max_candidates;
    float threshold;
    uint32_t dm_tiles, k_tiles; // filled by the launcher: tiles along the DMs and along the blocks
};
hipError_t bf_launch_find_candidates(const bf_cand_args &a, hipStream_t stream);
hipError_t bf_warm_module_candidates();

// The polyphase channeliser (bf_channeliser.hip; include/dcs_channeliser.h): float [nr_inputs][in_stride][2]
// -> FIR of P rows of N pairs, N-point butterfly network -> [N][out_blocks][out_inputs][16][2] as floats (out) or quantised
// (out_q8, with gains and counters); exactly one of out and out_q8 is set
struct bf_chan_args {
    const float *in;       // 8-byte aligned
    const float *taps;     // [P][N]
    const float *twiddles; // [N / 2][2], 8-byte aligned
    const float *gains;    // out_q8 only: [nr_inputs][N]
    float *out;            // 16-byte aligned, or nullptr
    int8_t *out_q8;        // 16-byte aligned, or nullptr
    unsigned long long *clip_count; // out_q8 only: [nr_inputs], or nullptr
    uint64_t in_stride;    // pairs, >= (nr_spectra + P - 1) N
    uint64_t out_blocks, first_block;
    uint64_t items;        // filled by the launcher
    uint32_t N, P, nr_inputs, nr_spectra, order, out_inputs, first_input;
    uint32_t groups;       // filled by the launcher: the groups of inputs that share an item
};
hipError_t bf_launch_channelise(const bf_chan_args &a, hipStream_t stream);
hipError_t bf_warm_module_channeliser();

// The RFI flagger (bf_rfi.hip; include/dcs_rfi.h) on the filterbanks uint8 [B][in_spectra][C].  The
// window is rows first .. first + nr_blocks * block_len - 1 of every beam, nr_blocks blocks of block_len rows.
// {sum x, sum x^2} per (beam, block, channel), and the sum over the channels of every row of the window
struct bf_rfi_moments_args {
    const uint8_t *in;   // 16-byte aligned
    uint32_t *cell_sums; // [B][nr_blocks][C][2]
    uint32_t *zero_dm;   // nullptr, or [B][nr_blocks * block_len]: zeroed by the launcher, added to by the kernel
    uint64_t in_spectra, first;
    uint32_t C, B, nr_blocks, block_len;
    uint32_t lanes, tiles; // filled by the launcher: lanes of 16 channels per row (a power of two <= 64), channel tiles per row
};
hipError_t bf_launch_rfi_moments(const bf_rfi_moments_args &a, hipStream_t stream);
// cell sums and the zero-DM series -> cell flags, channel masks, spectrum flags, counts; the thresholds by value
struct bf_rfi_flags_args {
    const uint32_t *cell_sums; // [B][nr_blocks][C][2]
    const uint32_t *zero_dm;   // nullptr, or [B][nr_blocks * block_len]
    uint8_t *cell_flags;       // [B][nr_blocks][C]
    uint8_t *channel_mask;     // [B][C]
    uint8_t *spectrum_flags;   // nullptr with zero_dm, or [B][nr_blocks * block_len]
    uint32_t *counts;          // [B][3]
    double mean_thr, mean_floor, var_thr, var_floor, zero_dm_thr, zero_dm_floor;
    uint32_t C, B, nr_blocks, block_len, max_bad_blocks;
};
hipError_t bf_launch_rfi_flags(const bf_rfi_flags_args &a, hipStream_t stream);
// the window with every flagged byte replaced by fill, into rows first_out .. of out uint8 [B][out_spectra][C]
struct bf_rfi_clean_args {
    const uint8_t *in;             // 16-byte aligned
    uint8_t *out;                  // 16-byte aligned; may be in where the rows are the same ones
    const uint8_t *cell_flags;     // nullptr (none), or [B][nr_blocks][C]
    const uint8_t *channel_mask;   // nullptr (none), or [B][C]: a zero byte replaces the channel
    const uint8_t *spectrum_flags; // nullptr (none), or [B][nr_blocks * block_len]
    unsigned long long *replaced;  // nullptr, or [B]: grows by the bytes replaced
    uint64_t in_spectra, first, out_spectra, first_out;
    uint32_t C, B, nr_blocks, block_len, fill;
    uint32_t lanes, tiles;         // filled by the launcher, as bf_rfi_moments_args
};
hipError_t bf_launch_rfi_clean(const bf_rfi_clean_args &a, hipStream_t stream);
hipError_t bf_warm_module_rfi();

// 8-bit search filterbanks (bf_filterbank.hip; include/dcs_filterbank.h).  Spectra are float
// [T][C][B], beam fastest; cb = C * B.
// Running sums {s1, s2} per (channel, beam) over the T spectra, in order, in fp64
struct bf_fbsums_args {
    const float *spectra;
    double *sums;        // [C][B][2]
    uint64_t cb;
    uint32_t T;
    uint32_t accumulate; // non-zero: the sums start from what sums holds
};
hipError_t bf_launch_spectra_sums(const bf_fbsums_args &a, hipStream_t stream);
// Sums -> scales {mu, k} float [C][B][2], in fp64 rounded once per operation
struct bf_fbscales_args {
    const double *sums;
    float *scales;
    uint64_t cb;
    uint64_t count; // spectra behind the sums: 1 .. 2^53 - 1
    float target_std;
};
hipError_t bf_launch_filterbank_scales(const bf_fbscales_args &a, hipStream_t stream);
// Spectra normalised with the scales, quantised and transposed into out uint8 [B][out_spectra][C], rows first .. first + T - 1
struct bf_fbq8_args {
    const float *spectra;
    const float *scales;               // [C][B][2], 8-byte aligned; read when the work runs
    uint8_t *out;                      // 16-byte aligned
    unsigned long long *clip_count;    // [B], added to; or nullptr: no counting
    uint64_t out_spectra, first;
    uint32_t C, B, T;
    uint32_t slices;                   // filled by the launcher: time slices a workgroup walks (gridDim.y runs of them)
    uint32_t descending;               // non-zero: channel c lands in column C - 1 - c
    float level;
};
hipError_t bf_launch_filterbank_q8(const bf_fbq8_args &a, hipStream_t stream);
hipError_t bf_warm_module_filterbank();

// One coefficient per lane, one time step (reference kernel a1's shape).
struct bf_naive_args {
    const dcs_delay_vals *delays;
    float *out; // [nc][n_pairs][2]
    float dt;
    uint32_t n_pairs;
    uint32_t c0, nc;
    dcs_bf_consts k;
};
hipError_t bf_launch_naive(const bf_naive_args &a, hipStream_t stream);

// local[a][b] = global[a][beam_offset + b]: the launch resolved but not enqueued (the kernel takes these six
// scalars as its parameters, in this order; a hipGraph kernel node is built from it -- dcs_bf_stream_tick_*_from_global)
struct bf_gather_launch {
    const void *func; // nullptr: nothing to launch
    dim3 grid, block;
    dcs_delay_vals *local;
    const dcs_delay_vals *global;
    uint32_t n_ant, nb_local, nb_total, beam_offset;
};
hipError_t bf_prepare_gather_beams(dcs_delay_vals *local, const dcs_delay_vals *global, uint32_t n_ant, uint32_t n_beams_local,
                                   uint32_t n_beams_total, uint32_t beam_offset, bf_gather_launch *out);
hipError_t bf_launch_gather_beams(dcs_delay_vals *local, const dcs_delay_vals *global,
                                  uint32_t n_ant, uint32_t n_beams_local, uint32_t n_beams_total,
                                  uint32_t beam_offset, hipStream_t stream);

hipError_t bf_warm_module();
hipError_t bf_launch_verify_div3(float D, float y, uint32_t *d_mismatches, hipStream_t stream);

#endif
