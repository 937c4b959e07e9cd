// bf_candidates.hip -- the candidate sifter on the signal-to-noise planes (include/dcs_candidates.h),
// gfx950 only.  Compares and integer counts, nothing else: no result depends on an order of evaluation, nothing is atomic,
// and no workgroup waits for another -- three launches on the stream order the three steps.
//
// A tile is kCandTileDms = 16 DMs by kCandTileBlocks = 64 blocks of one beam, one workgroup of four waves; a segment is one
// row of a tile, 64 cells of one DM, one lane each.  Segments are numbered (beam, DM, tile of blocks): that is the order of
// the list, so the concatenation of the segments' candidates IS the list, whatever number of tiles a row of blocks takes.
//
// bf_cand_tile_kernel.  The workgroup collapses the width axis of its tile and of a halo of dm_radius rows and block_radius
// columns around it, once per cell, into LDS: consecutive lanes take consecutive blocks of a row, so every load of a width's
// plane is coalesced along k.  A cell that does not exist -- outside [0, nr_dm) x [first_block, first_block + nr_blocks) --
// is stored as a NaN: an existing cell's s is never one (the collapse starts from -infinity and never takes a NaN), a NaN
// beats nothing, equals nothing and is not >= threshold, so the window needs no bounds of its own.  A wave then takes rows
// wave, wave + 4, ...: each lane holds its cell against the (2 dm_radius + 1)(2 block_radius + 1) cells of the window, LDS
// reads at consecutive addresses; the row's ballot is the segment's 64 marks, its popcount the segment's count.
// bf_cand_scan_kernel.  One workgroup of 1024 lanes makes the counts an exclusive prefix in place, kScanSpan = 4096 segments
// per round with the carry in a register, and writes d_count.
// bf_cand_scatter_kernel.  Tile by tile again; a tile without marks ends at once, so on a plane with few candidates the
// second collapse touches few tiles.  A tile with marks is staged as before, with the width index kept for the tile's own
// cells; a marked lane's place is the segment's prefix plus the popcount of the marks below its lane, and where that is
// below max_candidates it counts the window's members and writes its record as two 16-byte stores.
// Every offset into the planes and the records is 64-bit.

#include "bf_host.h"

#include "bf_arg_checks.h" // the tile's sides and the largest radius: what the workspace figure is made of

#include <hip/hip_runtime.h>

// The candidate sifter (include/dcs_candidates.h): the cells (beam, DM, block)
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

namespace {

constexpr uint32_t kThreads = 256;                            // four waves
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kRows = kCandTileDms, kCols = kCandTileBlocks;
constexpr uint32_t kHaloRows = kRows + 2u * kCandMaxRadius;   // 32
constexpr uint32_t kHaloCols = kCols + 2u * kCandMaxRadius;   // 80
constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kScanWaves = kScanThreads / 64u;
constexpr uint32_t kScanItems = 4;                            // consecutive segments of a lane
constexpr uint32_t kScanSpan = kScanThreads * kScanItems;     // segments of a round
constexpr uint32_t kNoWidth = 0xffffffffu;

static_assert(kCols == 64u, "a segment's marks are one wave's ballot");
static_assert(kRows % kWaves == 0u, "every wave takes the same number of rows");
static_assert(kHaloRows * kHaloCols * 4u + kRows * kCols * 4u <= 16u * 1024u, "the staged tile: 14 KiB of LDS");

// a record's half, stored at once: d_cands is 8-byte aligned, which a 16-byte global store does not mind
struct __attribute__((packed, aligned(8))) half_record {
    uint32_t w[4];
};

struct tile_at {
    uint32_t b, kt;
    uint32_t m0, k0; // the tile's first DM, and its first block counted from first_block
};

__device__ __forceinline__ tile_at tile_of(const bf_cand_args &a, uint32_t bid)
{
    tile_at t;
    t.kt = bid % a.k_tiles;
    const uint32_t rest = bid / a.k_tiles;
    t.b = rest / a.dm_tiles;
    t.m0 = (rest % a.dm_tiles) * kRows;
    t.k0 = t.kt * kCols;
    return t;
}

__device__ __forceinline__ size_t segment_of(const bf_cand_args &a, const tile_at &t, uint32_t m)
{
    return ((size_t)t.b * a.nr_dm + m) * a.k_tiles + t.kt;
}

// Rule 1 for the N widths from index i of a cell: their loads together, then the compares in the order of the widths
template <uint32_t N>
__device__ __forceinline__ void take_widths(const float *p, size_t pitch, uint32_t i, float &s, uint32_t &best)
{
    float v[N];
#pragma unroll
    for (uint32_t j = 0; j < N; j++) v[j] = p[(size_t)(i + j) * pitch];
#pragma unroll
    for (uint32_t j = 0; j < N; j++) {
        if (v[j] > s) { // false for a NaN
            s = v[j];
            best = i + j;
        }
    }
}

// The tile and its halo, the width axis collapsed: s of halo cell (hr, hc) at s_s[hr * cols + hc], cols = 64 + 2 block_radius;
// a NaN where the cell does not exist.  With kBest the width index of the tile's own cells goes to s_best[r * 64 + c]
template <bool kBest>
__device__ __forceinline__ void stage_tile(const bf_cand_args &a, const tile_at &t, float *s_s, uint32_t *s_best)
{
    const uint32_t rows = kRows + 2u * a.dm_radius, cols = kCols + 2u * a.block_radius;
    for (uint32_t idx = threadIdx.x; idx < rows * cols; idx += kThreads) {
        const uint32_t hr = idx / cols, hc = idx % cols;
        const int64_t m = (int64_t)t.m0 + hr - a.dm_radius, k = (int64_t)t.k0 + hc - a.block_radius;
        float s = __builtin_nanf("");
        uint32_t best = kNoWidth;
        if (m >= 0 && m < (int64_t)a.nr_dm && k >= 0 && k < (int64_t)a.nr_blocks) {
            s = -__builtin_inff();
            const float *p = a.snr + ((size_t)t.b * a.nr_dm + (size_t)m) * a.nr_widths * (size_t)a.peak_blocks +
                             ((size_t)a.first_block + (size_t)k);
            // the loads of eight (then four) widths in flight together: a lane has about ten cells and the chip few
            // workgroups of this kernel, so the loads' latency is what there is to hide
            const size_t pitch = (size_t)a.peak_blocks;
            uint32_t i = 0;
            for (; i + 8u <= a.nr_widths; i += 8u) take_widths<8>(p, pitch, i, s, best);
            if (i + 4u <= a.nr_widths) {
                take_widths<4>(p, pitch, i, s, best);
                i += 4u;
            }
            for (; i < a.nr_widths; i++) take_widths<1>(p, pitch, i, s, best);
        }
        s_s[idx] = s;
        if (kBest) {
            const uint32_t r = hr - a.dm_radius, c = hc - a.block_radius; // wrap below the tile: >= kRows, >= kCols
            if (r < kRows && c < kCols) s_best[r * kCols + c] = best;
        }
    }
}

__global__ void __launch_bounds__(kThreads) bf_cand_tile_kernel(const bf_cand_args a)
{
    __shared__ float s_s[kHaloRows * kHaloCols];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const tile_at t = tile_of(a, blockIdx.x);
    stage_tile<false>(a, t, s_s, nullptr);
    __syncthreads();
    const uint32_t dr = a.dm_radius, br = a.block_radius, cols = kCols + 2u * br;
    for (uint32_t r = wave; r < kRows && t.m0 + r < a.nr_dm; r += kWaves) {
        const float sp = s_s[(r + dr) * cols + lane + br];
        bool cand = sp >= a.threshold; // false for a cell that does not exist
        if (cand) {
            for (uint32_t dq = 0; dq <= 2u * dr && cand; dq++) {
                const float *row = &s_s[(r + dq) * cols + lane];
                for (uint32_t dk = 0; dk <= 2u * br; dk++) {
                    const float sq = row[dk];
                    const bool first = dq < dr || (dq == dr && dk < br); // (m_Q, k_Q) before (m_P, k_P)
                    if (sq > sp || (sq == sp && first)) cand = false;
                }
            }
        }
        const uint64_t marks = __ballot(cand);
        if (lane == 0u) {
            const size_t seg = segment_of(a, t, t.m0 + r);
            a.marks[seg] = marks;
            a.places[seg] = (uint32_t)__popcll(marks);
        }
    }
}

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

__global__ void __launch_bounds__(kScanThreads) bf_cand_scan_kernel(const bf_cand_args a)
{
    __shared__ uint32_t s_tot[kScanWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0u; // the candidates of the rounds before: the same in every lane
    for (uint64_t base = 0; base < a.segments; base += kScanSpan) {
        const uint64_t at = base + (uint64_t)kScanItems * tid;
        uint32_t v[kScanItems], sum = 0u;
#pragma unroll
        for (uint32_t j = 0; j < kScanItems; j++) {
            v[j] = at + j < a.segments ? a.places[at + j] : 0u;
            sum += v[j];
        }
        const uint32_t incl = wave_scan(sum, lane);
        if (lane == 63u) s_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kScanWaves; w++) {
            const uint32_t tot = s_tot[w];
            all += tot;
            before += w < wave ? tot : 0u;
        }
        uint32_t x = carry + before + (incl - sum);
#pragma unroll
        for (uint32_t j = 0; j < kScanItems; j++) {
            if (at + j < a.segments) a.places[at + j] = x;
            x += v[j];
        }
        carry += all;
        __syncthreads(); // s_tot is written again in the next round
    }
    if (tid == 0u) {
        a.count[0] = carry;
        a.count[1] = carry < a.max_candidates ? carry : a.max_candidates;
    }
}

__global__ void __launch_bounds__(kThreads) bf_cand_scatter_kernel(const bf_cand_args a)
{
    __shared__ float s_s[kHaloRows * kHaloCols];
    __shared__ uint32_t s_best[kRows * kCols];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const tile_at t = tile_of(a, blockIdx.x);
    // marks that still have a place in the list: none, and the tile is not staged
    int any = 0;
    for (uint32_t r = wave; r < kRows && t.m0 + r < a.nr_dm; r += kWaves) {
        const size_t seg = segment_of(a, t, t.m0 + r);
        any |= a.marks[seg] != 0u && a.places[seg] < a.max_candidates;
    }
    if (!__syncthreads_or(any)) return;
    stage_tile<true>(a, t, s_s, s_best);
    __syncthreads();
    const uint32_t dr = a.dm_radius, br = a.block_radius, cols = kCols + 2u * br;
    for (uint32_t r = wave; r < kRows && t.m0 + r < a.nr_dm; r += kWaves) {
        const uint32_t m = t.m0 + r;
        const size_t seg = segment_of(a, t, m);
        const uint64_t marks = a.marks[seg];
        const uint64_t place = (uint64_t)a.places[seg] + (uint32_t)__popcll(marks & ((1ull << lane) - 1ull));
        if (!((marks >> lane) & 1ull) || place >= a.max_candidates) continue;
        uint32_t members = 0u;
        for (uint32_t dq = 0; dq <= 2u * dr; dq++) {
            const float *row = &s_s[(r + dq) * cols + lane];
            for (uint32_t dk = 0; dk <= 2u * br; dk++) members += row[dk] >= a.threshold ? 1u : 0u;
        }
        const float sp = s_s[(r + dr) * cols + lane + br];
        const uint32_t best = s_best[r * kCols + lane]; // a width index: a candidate's s is above -infinity
        const size_t k = (size_t)a.first_block + t.k0 + lane;
        const size_t cell = (((size_t)t.b * a.nr_dm + m) * a.nr_widths + best) * (size_t)a.peak_blocks + k;
        const uint2 peak = *reinterpret_cast<const uint2 *>(a.peaks + 2u * cell); // {value, time}
        half_record *out = reinterpret_cast<half_record *>(a.cands + (size_t)place * 8u);
        out[0] = half_record{{t.b, m, best, (uint32_t)k}};
        out[1] = half_record{{peak.y, peak.x, __float_as_uint(sp), members}};
    }
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_candidates()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_cand_tile_kernel));
}

// The tile kernel, the scan, and -- where a record can be written -- the scatter; an empty shape launches the scan alone,
// which zeroes d_count
static hipError_t bf_launch_find_candidates(const bf_cand_args &args, hipStream_t stream)
{
    if (args.dm_radius > kCandMaxRadius || args.block_radius > kCandMaxRadius) return hipErrorInvalidValue; // what the LDS tile is sized for
    bf_cand_args a = args;
    a.k_tiles = (uint32_t)(((uint64_t)a.nr_blocks + kCols - 1u) / kCols);
    a.dm_tiles = (uint32_t)(((uint64_t)a.nr_dm + kRows - 1u) / kRows);
    const unsigned __int128 segments = candidates_segments(a.B, a.nr_dm, a.nr_blocks);
    const unsigned __int128 tiles = (unsigned __int128)a.B * a.dm_tiles * a.k_tiles;
    if (segments > 0xffffffffull || tiles > 0x7fffffffull) return hipErrorInvalidValue;
    a.segments = (uint64_t)segments;
    if (tiles) {
        hipLaunchKernelGGL(bf_cand_tile_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(bf_cand_scan_kernel, dim3(1u), dim3(kScanThreads), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    if (tiles && a.max_candidates) {
        hipLaunchKernelGGL(bf_cand_scatter_kernel, dim3((uint32_t)tiles), dim3(kThreads), 0, stream, a);
        return hipGetLastError();
    }
    return hipSuccess;
}

// The host side of include/dcs_candidates.h, behind the table as in bf_integrate.hip.  Nothing allocated; of the context only
// its device is used.  The counts and a record's block are 32-bit words: a call with 2^32 cells or more, or with a block past
// 2^32, is not supported.
namespace bf_host {

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

} // namespace bf_host
