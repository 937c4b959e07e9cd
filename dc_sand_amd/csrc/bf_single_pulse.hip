// bf_single_pulse.hip -- the single-pulse search on the DM-time planes (include/dcs_single_pulse.h),
// gfx950 only: the exact sums of every (beam, DM) series, the boxcar peaks per width and block of times, and the peaks as
// signal-to-noise.  Sums and peaks are integer arithmetic mod 2^64 and mod 2^32, so nothing in them depends on an order.
//
// bf_boxcar_peaks_kernel.  A workgroup of four waves owns one series and a run of consecutive blocks that together cover at
// most kSegment = 4096 times:
//
//  * it stages the run's nt + max_width - 1 words from global memory once, for all widths: every lane takes four
//    consecutive words per tile of 1024, counted from the 16-byte boundary at or below the run's first word, as one 16-byte
//    load where all four lie inside the window and word by word under guards elsewhere (the head, the tail, and every series
//    whose first word is not 16-byte aligned is shifted, not slowed).  Nothing outside the window [first, first + T +
//    max_width - 1) of the series is read, whatever the width list holds;
//  * the words become an inclusive prefix sum mod 2^32: four words in the lane, a wave scan of the lanes' totals, and the
//    carries of the (tile, wave) totals, which every wave scans for itself out of 36 words of LDS.  The prefix is stored with
//    one 16-byte write per lane and tile; P[t] = the sum of the words below t lies at s_p[t + mis + 3].  The prefix wraps at
//    realistic sizes (8191 words of about 2^20), which unsigned arithmetic does not mind: S_w[t] = P[t + w] - P[t] is exact
//    mod 2^32 for every width;
//  * a wave then takes a block and kBatch = 8 widths of the list at a time.  The widths are the same in every lane: one
//    vector load per batch, issued a batch ahead, and v_readlane_b32 make scalars of them; consecutive lanes take consecutive t, so the LDS reads -- P[t] once, P[t + w] per width -- have
//    no bank conflict, and the eight sums of a time are independent of each other.  A lane keeps per width the largest
//    sum of its times and the first time that has it, and makes the 64-bit key (sum << 32) | ~t of them, which orders by
//    the sum first and by the EARLIER time then.  The eight reductions over the wave's lanes run as one: three steps
//    that each halve the keys a lane carries, three on the one that is left, 10 exchanges instead of 48; eight lanes
//    store {sum, time} with one 8-byte store each.  A width outside [1, max_width] sums nothing (w = 0) and stores
//    {0, 0xffffffff}.  No wave waits for another after the prefix, and nothing is atomic;
//  * every offset into the planes and the peaks is 64-bit.
//
// bf_dm_time_sums_kernel: one workgroup per series, 16-byte loads with the same guards, 64-bit accumulators.
// bf_peak_snr_kernel: one lane per (series, block), looping over the widths; fp64 rounded once per operation (the build has
// -ffp-contract=off; the divides and the square root are the correctly rounded ones, as bf_filterbank.hip's scales rely on).

#include "bf_host.h"

#include <hip/hip_runtime.h>

// The single-pulse search on the DM-time planes (include/dcs_single_pulse.h).
// A series is one (beam, DM) pair: series s begins at word s * plane_spectra of the planes.
// {sum x, sum x^2 mod 2^64} of words first .. first + T - 1 of every series
struct bf_dtsums_args {
    const uint32_t *plane; // [series][plane_spectra]
    uint64_t *sums;        // [series][2]
    uint64_t plane_spectra, first;
    uint32_t T;
    uint32_t accumulate;   // non-zero: added to what sums holds
};
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

namespace {

constexpr uint32_t kThreads = 256;                 // four waves
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kSegment = 4096;                // times of a workgroup's run of blocks at the most
constexpr uint32_t kMaxWidth = 4096;               // as include/dcs_single_pulse.h
constexpr uint32_t kTileWords = 4u * kThreads;     // words that the workgroup loads at once
// staged words, counted from the 16-byte boundary at or below the first: at most 3 + kSegment + kMaxWidth - 1
constexpr uint32_t kTiles = (3u + kSegment + kMaxWidth - 1u + kTileWords - 1u) / kTileWords;
constexpr uint32_t kPrefixWords = 4u + kTiles * kTileWords; // four zero words in front: P[0] where the first word is aligned

constexpr uint32_t kBatch = 8;                     // widths that a wave carries through a block at once

static_assert(kBatch == 8u, "the batch's reduction leaves width j in the lanes with (lane >> 3) == j");
static_assert(kTiles == 9u && kTiles * kWaves <= 64u, "one lane per (tile, wave) total");
static_assert(kPrefixWords * 4u + kTiles * kWaves * 4u <= 40u * 1024u, "four workgroups per CU");

// inclusive scan over the lanes of a wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)x, d);
        if (lane >= d) x += o;
    }
    return x;
}

// The four words q .. q + 3, counted from the 16-byte boundary mis words below src, of which [mis, mis + n) exist: one
// 16-byte load where all four exist, else zeros -- and load_ragged_quad's loads afterwards.  Two functions, so that a
// caller's 16-byte loads are all in flight before the first ragged quad, which only the first and the last lane of a
// window have, makes it wait
__device__ __forceinline__ bool whole_quad(uint32_t mis, uint64_t n, uint64_t q) { return q >= mis && q - mis + 3u < n; }

__device__ __forceinline__ void load_whole_quad(const uint32_t *src, uint32_t mis, uint64_t n, uint64_t q, uint32_t v[4])
{
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (whole_quad(mis, n, q)) w = *reinterpret_cast<const uint4 *>(src + (q - mis));
    v[0] = w.x;
    v[1] = w.y;
    v[2] = w.z;
    v[3] = w.w;
}

__device__ __forceinline__ void load_ragged_quad(const uint32_t *src, uint32_t mis, uint64_t n, uint64_t q, uint32_t v[4])
{
    if (!whole_quad(mis, n, q) && q + 3u >= mis && q < mis + n) { // some of the four exist
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) v[i] = q + i >= mis && q + i - mis < n ? src[q + i - mis] : 0u;
    }
}

// One step of the batch's reduction: of the 2 H keys a lane carries, the lanes with bit 8 H set go on with the upper H and
// the others with the lower H, each taking its partner's largest for them.  H is a template argument so that every index
// into key is a constant and the keys stay in registers
template <uint32_t H>
__device__ __forceinline__ void halve_keys(uint64_t (&key)[kBatch], uint32_t lane)
{
    const bool upper = (lane & (8u * H)) != 0u;
#pragma unroll
    for (uint32_t j = 0; j < H; j++) {
        const uint64_t send = upper ? key[j] : key[j + H], keep = upper ? key[j + H] : key[j];
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)send, (int)(8u * H));
        key[j] = o > keep ? o : keep;
    }
}

__global__ void __launch_bounds__(kThreads) bf_boxcar_peaks_kernel(const bf_boxcar_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_p[kPrefixWords];
    __shared__ uint32_t s_tot[kTiles * kWaves];

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const size_t series = blockIdx.x / a.segments;
    const uint32_t blk0 = (blockIdx.x % a.segments) * a.run; // the run's first block
    const uint32_t t0 = blk0 * a.block_len;                  // < T
    const uint32_t span = a.run * a.block_len;               // <= kSegment
    const uint32_t nt = a.T - t0 < span ? a.T - t0 : span;   // the run's times
    const uint32_t n = nt + a.max_width - 1u;                // the words they need: inside the series' window
    const uint32_t *src = a.plane + series * (size_t)a.plane_spectra + (size_t)a.first + t0;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) >> 2) & 3u;
    const uint32_t tiles = (mis + n + kTileWords - 1u) / kTileWords; // <= kTiles

    // a tile past the window loads nothing and holds zeros: every tile is scanned, so that the nine scans, which do not
    // depend on each other, run side by side instead of six dependent cross-lane steps at a time
    uint32_t v[kTiles][4], incl[kTiles];
#pragma unroll
    for (uint32_t k = 0; k < kTiles; k++) load_whole_quad(src, mis, n, k * kTileWords + 4u * tid, v[k]);
#pragma unroll
    for (uint32_t k = 0; k < kTiles; k++) load_ragged_quad(src, mis, n, k * kTileWords + 4u * tid, v[k]);
#pragma unroll
    for (uint32_t k = 0; k < kTiles; k++) {
        v[k][1] += v[k][0];
        v[k][2] += v[k][1];
        v[k][3] += v[k][2];
        incl[k] = v[k][3];
    }
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
#pragma unroll
        for (uint32_t k = 0; k < kTiles; k++) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl[k], d);
            if (lane >= d) incl[k] += o;
        }
    }
    if (lane == 63u) {
#pragma unroll
        for (uint32_t k = 0; k < kTiles; k++) s_tot[k * kWaves + wave] = incl[k];
    }
    if (tid < 4u) s_p[tid] = 0u;
    __syncthreads();
    // the carry into (tile, wave): the totals before it, in the order of the words
    const uint32_t tot = lane < kTiles * kWaves ? s_tot[lane] : 0u;
    const uint32_t carry = wave_scan(tot, lane) - tot;
#pragma unroll
    for (uint32_t k = 0; k < kTiles; k++) {
        if (k < tiles) {
            const uint32_t base = (uint32_t)__shfl((int)carry, (int)(k * kWaves + wave)) + (incl[k] - v[k][3]);
            *reinterpret_cast<uint4 *>(&s_p[4u + k * kTileWords + 4u * tid]) =
                make_uint4(base + v[k][0], base + v[k][1], base + v[k][2], base + v[k][3]);
        }
    }
    __syncthreads();

    const uint32_t off = mis + 3u; // P[t] at s_p[t + off]: the words in front of the first are zero, and so is P[0]
    const uint32_t nb = (nt + a.block_len - 1u) / a.block_len;
    const uint32_t batches = (a.nr_widths - 1u) / kBatch + 1u; // nr_widths >= 1: the launcher's
    // Lane l's width of a batch: widths[8 * batch + (l >> 3)], or 0 -- which sums nothing -- where it takes no part or the
    // list has ended.  One vector load per batch: the list changes between replays and the kernel stores to global memory, so
    // the compiler would not read it through the scalar cache, and eight dependent loads per batch cost more than the sums
    auto width_of_lane = [&](uint32_t batch) -> uint32_t {
        const uint32_t i = batch * kBatch + (lane >> 3);
        const uint32_t wl = batch < batches && i < a.nr_widths ? a.widths[i] : 0u;
        return wl - 1u < a.max_width ? wl : 0u;
    };
    // the (batch, block) pairs in turn, blocks fastest: pair number wave, wave + kWaves, ...; the next pair's widths are
    // loaded under this pair's sums
    uint32_t batch = wave / nb, kb = wave % nb;
    uint32_t wl = width_of_lane(batch);
    while (batch < batches) {
        const uint32_t i0 = batch * kBatch;
        uint32_t next_batch = batch, next_kb = kb + kWaves;
        for (; next_kb >= nb; next_kb -= nb) next_batch++; // nb >= 1: at most kWaves rounds
        const uint32_t next_wl = width_of_lane(next_batch);
        uint32_t w[kBatch]; // the same in every lane
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) w[j] = (uint32_t)__builtin_amdgcn_readlane((int)wl, (int)(8u * j));
        const uint32_t tb = kb * a.block_len;
        const uint32_t te = nt - tb < a.block_len ? nt : tb + a.block_len;
        // per width the largest sum of this lane's times and its first time.  The times ascend, so "strictly larger" keeps
        // the first; the start {0, the lane's first time} is right whatever the first sum is
        const uint32_t t_first = tb + lane;
        uint32_t bs[kBatch], bt[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) {
            bs[j] = 0u;
            bt[j] = t_first;
        }
        for (uint32_t t = t_first; t < te; t += 64u) {
            const uint32_t p0 = s_p[t + off];
#pragma unroll
            for (uint32_t j = 0; j < kBatch; j++) {
                const uint32_t s = s_p[t + w[j] + off] - p0;
                bt[j] = s > bs[j] ? t : bt[j];
                bs[j] = s > bs[j] ? s : bs[j];
            }
        }
        // the keys (sum << 32) | ~time order by the sum first and by the EARLIER time then; 0, for a lane without a time, is
        // below every key: a time is at most 2^32 - 2, so a key's low word is at least 1
        uint64_t key[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++) key[j] = t_first < te ? ((uint64_t)bs[j] << 32) | (uint32_t)~(t0 + bt[j]) : 0u;
        // eight reductions over 64 lanes as one: each of the first three steps halves the keys a lane carries -- the lanes
        // with the step's bit set go on with the upper half of them -- and three more reduce the one that is left.  Lane l then
        // holds the largest key of width i0 + ((l >> 3) & 7): 10 key exchanges per batch instead of 48
        halve_keys<4>(key, lane);
        halve_keys<2>(key, lane);
        halve_keys<1>(key, lane);
#pragma unroll
        for (int x = 4; x > 0; x >>= 1) {
            const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)key[0], x);
            key[0] = o > key[0] ? o : key[0];
        }
        const uint32_t i = i0 + (lane >> 3);
        if ((lane & 7u) == 0u && i < a.nr_widths) {
            uint32_t *out = a.peaks + ((series * a.nr_widths + i) * (size_t)a.peak_blocks + (size_t)a.first_block + blk0 + kb) * 2u;
            *reinterpret_cast<uint2 *>(out) = wl != 0u ? make_uint2((uint32_t)(key[0] >> 32), ~(uint32_t)key[0]) : make_uint2(0u, 0xffffffffu);
        }
        batch = next_batch;
        kb = next_kb;
        wl = next_wl;
    }
}

__global__ void __launch_bounds__(kThreads) bf_dm_time_sums_kernel(const bf_dtsums_args a)
{
    __shared__ uint64_t s_part[kWaves][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const size_t series = blockIdx.x;
    const uint32_t *src = a.plane + series * (size_t)a.plane_spectra + (size_t)a.first;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) >> 2) & 3u;
    const uint64_t end = (uint64_t)a.T + mis;
    uint64_t s1 = 0u, s2 = 0u;
    for (uint64_t q = 4u * tid; q < end; q += kTileWords) {
        uint32_t v[4];
        load_whole_quad(src, mis, a.T, q, v);
        load_ragged_quad(src, mis, a.T, q, v);
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint64_t x = v[i];
            s1 += x;
            s2 += x * x;
        }
    }
#pragma unroll
    for (int x = 32; x > 0; x >>= 1) {
        s1 += (uint64_t)__shfl_xor((unsigned long long)s1, x);
        s2 += (uint64_t)__shfl_xor((unsigned long long)s2, x);
    }
    if (lane == 0u) {
        s_part[wave][0] = s1;
        s_part[wave][1] = s2;
    }
    __syncthreads();
    if (tid < 2u) {
        uint64_t s = a.accumulate ? a.sums[2u * series + tid] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kWaves; k++) s += s_part[k][tid];
        a.sums[2u * series + tid] = s;
    }
}

__global__ void __launch_bounds__(256) bf_peak_snr_kernel(const bf_peaksnr_args a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // series * nr_blocks + k
    if (g >= a.total) return;
    const size_t series = g / a.nr_blocks;
    const size_t block = (size_t)a.first_block + g % a.nr_blocks;
    const double N = (double)a.count;
    const double mean = (double)a.sums[2u * series] / N;
    const double var = (double)a.sums[2u * series + 1u] / N - mean * mean;
    float top = -__builtin_inff();
    uint32_t best = 0xffffffffu;
    for (uint32_t i = 0; i < a.nr_widths; i++) {
        const size_t at = (series * a.nr_widths + i) * (size_t)a.peak_blocks + block;
        const uint32_t w = a.widths[i];
        float snr = -__builtin_inff();
        if (w - 1u < a.max_width) {
            snr = 0.0f;
            if (var > 0.0) { // false for a NaN
                const double num = (double)a.peaks[2u * at] - (double)w * mean;
                const double den = sqrt((double)w * var);
                snr = (float)(num / den);
            }
        }
        a.snr[at] = snr;
        if (snr > top) {
            top = snr;
            best = i;
        }
    }
    if (a.best) a.best[series * (size_t)a.peak_blocks + block] = best;
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_single_pulse()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_boxcar_peaks_kernel));
}

static hipError_t bf_launch_dm_time_sums(const bf_dtsums_args &a, uint64_t series, hipStream_t stream)
{
    if (series == 0u) return hipSuccess;
    if (series > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_dm_time_sums_kernel, dim3((uint32_t)series), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_boxcar_peaks(const bf_boxcar_args &args, uint64_t series, hipStream_t stream)
{
    if (series == 0u || args.T == 0u || args.nr_widths == 0u) return hipSuccess;
    if (args.max_width < 1u || args.max_width > kMaxWidth || args.block_len < 64u || args.block_len > kSegment || args.block_len % 64u)
        return hipErrorInvalidValue; // what the staging buffer is sized for
    bf_boxcar_args a = args;
    a.run = kSegment / a.block_len;
    const uint32_t nr_blocks = (a.T - 1u) / a.block_len + 1u;
    a.segments = (nr_blocks - 1u) / a.run + 1u;
    const unsigned __int128 blocks = (unsigned __int128)series * a.segments;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_boxcar_peaks_kernel, dim3((uint32_t)blocks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_peak_snr(const bf_peaksnr_args &a, hipStream_t stream)
{
    if (a.total == 0u) return hipSuccess;
    const uint64_t blocks = (a.total + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_peak_snr_kernel, dim3((uint32_t)blocks), dim3(256u), 0, stream, a);
    return hipGetLastError();
}

// The host side of include/dcs_single_pulse.h, behind the table as in bf_integrate.hip.  Nothing allocated; of the context only
// its device is used.  A series is one (beam, DM) pair; nr_beams * nr_dm of them fit 64 bits.
namespace bf_host {

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

} // namespace bf_host
