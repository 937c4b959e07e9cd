// bf_rfi.hip -- the RFI flagger on the 8-bit search filterbanks (include/dcs_rfi.h), gfx950 only:
// the statistics pass, the flags from the statistics, and the cleaned filterbank.  Every quantity is an integer and every sum
// exact, so nothing here depends on an order of summation or on the launch geometry; the only atomics are integer adds.
//
// The two hot kernels share one geometry.  A workgroup of 256 threads owns one beam, one block of block_len rows and one
// tile of 16 L channels, L = a.lanes a power of two <= 64: thread (j, r) = (tid % L, tid / L) holds 16 channels of the rows
// r, r + R, ... (R = 256 / L; the moments take them four at a time).  Where C % 16 == 0 a lane's channels are the 16
// consecutive ones at 16 j, one 16-byte load (or store) per row; where only C % 4 == 0 they are four dwords, dword q at
// 4 (q L + j); for every other C they are j, j + L, ..., 15 L + j, sixteen byte accesses -- in both the lanes of a row access
// side by side, and the bytes are assembled into the same four dwords.  Every offset into the filterbanks is 64-bit.
//
// bf_rfi_moments_kernel.  Four rows of a lane are 4 x 4 dwords.  udot4 of a dword with 0x01010101 is the lane's share of the
// row's zero-DM sum: the L lanes of the row add theirs across lanes, four rows at a time, and four of them add the totals to the
// words with one integer atomic, because a row wider than one tile is split over workgroups (the launcher zeroes the words with a memset).
// Transposed as 4 x 4 bytes (8 v_perm_b32, as bf_dedisperse.hip does) a dword holds four TIMES of one channel: udot4 with
// itself adds to s2, with 0x01010101 to s1 -- 32 accumulators per lane, about one vector operation per byte.  The R time
// slices of a workgroup add their accumulators in LDS with integer atomics, and the tile's 32 L words are stored once.
//
// bf_rfi_clean_kernel.  A lane turns the channel mask and the block's cell flags of its 16 channels into four select dwords,
// once; per row it loads the row's flag byte and its 16 bytes, selects with v_bfi_b32 and stores.  In place every byte is
// read and written by the same thread.  The bytes replaced are counted per thread, added over the wave, and one 64-bit atomic
// per wave adds them to the beam's counter.
//
// The flags (small): bf_rfi_cell_flags_kernel, one workgroup per (beam, block), finds the lower median of the C values m and
// of the C values q, and of their distances from it, by bisection on the value's bits -- two bits a pass, which counts the
// elements below three candidates with compares, ballots and popcounts -- so it needs no workspace and serves any C;
// bf_rfi_beam_kernel, one workgroup per beam, counts every channel's bad blocks, and does the same bisection on the zero-DM
// series of the whole window.  Both keep the values of a pass on chip where they fit (4096 channels in LDS, 16384 spectra in
// registers) and read them from global memory in every pass where they do not: the same counts either way.

#include "bf_host.h"

#include <hip/hip_runtime.h>

// The RFI flagger (include/dcs_rfi.h) on the filterbanks uint8 [B][in_spectra][C].  The
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

namespace {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256;          // four waves
constexpr uint32_t kLaneChannels = 16;      // channels a lane holds
constexpr uint32_t kMaxLanes = 64;          // lanes of one row in a workgroup
constexpr uint32_t kOnes = 0x01010101u;

// bytes b0 b1 b2 b3 of four dwords w0 .. w3 -> the four dwords (w0.bk, w1.bk, w2.bk, w3.bk), k = 0 .. 3
__device__ __forceinline__ void transpose4(const uint32_t w0, const uint32_t w1, const uint32_t w2, const uint32_t w3, uint32_t out[4])
{
    const uint32_t a = __builtin_amdgcn_perm(w1, w0, 0x05010400u); // w0.b0 w1.b0 w0.b1 w1.b1
    const uint32_t b = __builtin_amdgcn_perm(w1, w0, 0x07030602u); // w0.b2 w1.b2 w0.b3 w1.b3
    const uint32_t c = __builtin_amdgcn_perm(w3, w2, 0x05010400u);
    const uint32_t d = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
    out[0] = __builtin_amdgcn_perm(c, a, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(d, b, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(d, b, 0x07060302u);
}

// 0xff in every byte of f that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(const uint32_t f)
{
    const uint32_t top = (((f & 0x7f7f7f7fu) + 0x7f7f7f7fu) | f) & 0x80808080u;
    return (top >> 7) * 0xffu;
}

// Where the lane's channel i = 0 .. 15 lies in the tile, by the unit U of the row accesses: 16 (one 16-byte access at 16 j), 4
// (dword q = i / 4 at 4 (q L + j)) or 1 (byte i at i L + j).  The lanes of a row lie side by side in every form.
template <uint32_t U>
__device__ __forceinline__ uint32_t at_of(const uint32_t i, const uint32_t j, const uint32_t L)
{
    return U == 16u ? kLaneChannels * j + i : U == 4u ? 4u * ((i >> 2) * L + j) + (i & 3u) : i * L + j;
}

// The 16 bytes of a lane from p on as four dwords: byte e of dword q is the lane's channel 4 q + e, at p[at_of(4 q + e)].  Where
// `vec` says that p is aligned to U, units of U bytes are loaded, else single bytes; what lies at or past `end` (an index from
// p on, a multiple of U) reads as zero.
template <uint32_t U>
__device__ __forceinline__ void load16(const uint8_t *p, const uint32_t j, const uint32_t L, const uint32_t end, const bool vec, uint32_t w[4])
{
    if (U == 16u && vec) {
        const uintx4 v = *reinterpret_cast<const uintx4 *>(p + kLaneChannels * j);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return;
    }
    if (U == 4u && vec) {
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            const uint32_t at = at_of<U>(4u * q, j, L);
            w[q] = at < end ? *reinterpret_cast<const uint32_t *>(p + at) : 0u;
        }
        return;
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        uint32_t d = 0u;
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            const uint32_t at = at_of<U>(4u * q + e, j, L);
            const uint32_t byte = at < end ? p[at] : 0u;
            d |= byte << (8u * e);
        }
        w[q] = d;
    }
}

// the same 16 bytes stored, in units of U bytes; p is aligned to U, and with U = 16 the lane has all its channels
template <uint32_t U>
__device__ __forceinline__ void store16(uint8_t *p, const uint32_t j, const uint32_t L, const uint32_t end, const uint32_t w[4])
{
    if (U == 16u) {
        uintx4 v;
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        *reinterpret_cast<uintx4 *>(p + kLaneChannels * j) = v;
        return;
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        if (U == 4u) {
            const uint32_t at = at_of<U>(4u * q, j, L);
            if (at < end) *reinterpret_cast<uint32_t *>(p + at) = w[q];
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                const uint32_t at = at_of<U>(4u * q + e, j, L);
                if (at < end) p[at] = (uint8_t)(w[q] >> (8u * e));
            }
        }
    }
}

// what a workgroup of the two hot kernels owns, from its number: tiles fastest, so that the workgroups that run together read
// one row side by side
struct rfi_tile {
    uint32_t j, r, R, L, beam, k, c0, width; // width: the tile's channels that exist, 1 .. 16 L
};
__device__ __forceinline__ rfi_tile rfi_tile_of(const uint32_t lanes, const uint32_t tiles, const uint32_t nr_blocks, const uint32_t C)
{
    rfi_tile t;
    const uint32_t tid = threadIdx.x;
    t.L = lanes;
    t.j = tid & (lanes - 1u);
    t.r = tid >> __builtin_ctz(lanes);
    t.R = kThreads >> __builtin_ctz(lanes);
    uint32_t blk = blockIdx.x;
    t.c0 = (blk % tiles) * kLaneChannels * lanes;
    blk /= tiles;
    t.k = blk % nr_blocks;
    t.beam = blk / nr_blocks;
    t.width = C - t.c0 < kLaneChannels * lanes ? C - t.c0 : kLaneChannels * lanes;
    return t;
}

template <uint32_t U>
__global__ void __launch_bounds__(kThreads) bf_rfi_moments_kernel(const bf_rfi_moments_args a)
{
    __shared__ uint32_t s_acc[kMaxLanes * kLaneChannels * 2u]; // {s1, s2} of the tile's channels, in the tile's channel order

    const rfi_tile t = rfi_tile_of(a.lanes, a.tiles, a.nr_blocks, a.C);
    const uint32_t tid = threadIdx.x, n = a.block_len;
    const uint64_t window = (uint64_t)a.nr_blocks * n;
    // row 0 of the block, at the tile's first channel
    const uint8_t *in0 = a.in + ((size_t)t.beam * a.in_spectra + a.first + (size_t)t.k * n) * (size_t)a.C + t.c0;
    uint32_t *z0 = a.zero_dm ? a.zero_dm + (size_t)t.beam * window + (size_t)t.k * n : nullptr;
    // the lane has a channel at all; with U = 16 its 16 channels exist together or not at all
    const bool lane_on = at_of<U>(0u, t.j, t.L) < t.width;

    for (uint32_t i = tid; i < 2u * kLaneChannels * t.L; i += kThreads) s_acc[i] = 0u;

    uint32_t s1[kLaneChannels], s2[kLaneChannels];
#pragma unroll
    for (uint32_t i = 0; i < kLaneChannels; i++) s1[i] = s2[i] = 0u;

    const uint32_t groups = (n + 3u) / 4u; // of four rows
    // rows 4 g .. 4 g + 3 of the block; a row at or past n, and a lane without channels, reads as zeros
    auto load_group = [&](const uint32_t g, uint32_t w[4][4]) {
#pragma unroll
        for (uint32_t row = 0; row < 4u; row++) {
            const uint32_t tt = 4u * g + row;
            if (g < groups && tt < n && lane_on)
                load16<U>(in0 + (size_t)tt * a.C, t.j, t.L, t.width, true, w[row]);
            else
                w[row][0] = w[row][1] = w[row][2] = w[row][3] = 0u;
        }
    };
    auto use_group = [&](const uint32_t g, const uint32_t w[4][4]) {
        if (z0) {
            // the lane's share of the four rows' sums; the L lanes of a row are consecutive lanes of one wave and run the same trips
            uint32_t z[4];
#pragma unroll
            for (uint32_t row = 0; row < 4u; row++) {
                z[row] = 0u;
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) z[row] = __builtin_amdgcn_udot4(w[row][q], kOnes, z[row], false);
            }
            if (t.L >= 4u) {
                // four sums over L lanes in 2 + 1 + (log2 L - 2) exchanges instead of 4 log2 L: a lane keeps the two rows that its bit 0
                // names and hands the other two to its neighbour, then the one row that its bit 1 names; the rest are plain
                // halvings.  Lanes 0 .. 3 of the row end up with the totals of rows 0, 2, 1, 3 and add them with one atomic
                const bool b0 = (t.j & 1u) != 0u, b1 = (t.j & 2u) != 0u;
                const uint32_t a0 = (b0 ? z[2] : z[0]) + (uint32_t)__shfl_xor((int)(b0 ? z[0] : z[2]), 1);
                const uint32_t a1 = (b0 ? z[3] : z[1]) + (uint32_t)__shfl_xor((int)(b0 ? z[1] : z[3]), 1);
                uint32_t sum = (b1 ? a1 : a0) + (uint32_t)__shfl_xor((int)(b1 ? a0 : a1), 2);
                for (uint32_t x = 4u; x < t.L; x <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x);
                const uint32_t tt = 4u * g + 2u * (t.j & 1u) + ((t.j >> 1) & 1u);
                if (t.j < 4u && g < groups && tt < n) atomicAdd(z0 + tt, sum);
            } else {
#pragma unroll
                for (uint32_t row = 0; row < 4u; row++) {
                    uint32_t sum = z[row];
                    for (uint32_t x = 1u; x < t.L; x <<= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x);
                    const uint32_t tt = 4u * g + row;
                    if (t.j == 0u && g < groups && tt < n) atomicAdd(z0 + tt, sum);
                }
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            uint32_t o[4];
            transpose4(w[0][q], w[1][q], w[2][q], w[3][q], o);
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                s1[4u * q + e] = __builtin_amdgcn_udot4(o[e], kOnes, s1[4u * q + e], false);
                s2[4u * q + e] = __builtin_amdgcn_udot4(o[e], o[e], s2[4u * q + e], false);
            }
        }
    };
    // two groups of a lane in flight: eight 16-byte loads before the first use.  Every thread runs the same trips
    for (uint32_t g0 = 0; g0 < groups; g0 += 2u * t.R) {
        uint32_t wa[4][4], wb[4][4];
        load_group(g0 + t.r, wa);
        load_group(g0 + t.R + t.r, wb);
        use_group(g0 + t.r, wa);
        use_group(g0 + t.R + t.r, wb);
    }

    __syncthreads(); // s_acc is zero
    if (lane_on) {
#pragma unroll
        for (uint32_t i = 0; i < kLaneChannels; i++) {
            const uint32_t at = at_of<U>(i, t.j, t.L);
            atomicAdd(&s_acc[2u * at], s1[i]);
            atomicAdd(&s_acc[2u * at + 1u], s2[i]);
        }
    }
    __syncthreads();
    uint32_t *out = a.cell_sums + (((size_t)t.beam * a.nr_blocks + t.k) * a.C + t.c0) * 2u;
    for (uint32_t i = tid; i < 2u * t.width; i += kThreads) out[i] = s_acc[i];
}

template <uint32_t U>
__global__ void __launch_bounds__(kThreads) bf_rfi_clean_kernel(const bf_rfi_clean_args a)
{
    const rfi_tile t = rfi_tile_of(a.lanes, a.tiles, a.nr_blocks, a.C);
    const uint32_t n = a.block_len;
    const uint64_t window = (uint64_t)a.nr_blocks * n;
    const uint8_t *in0 = a.in + ((size_t)t.beam * a.in_spectra + a.first + (size_t)t.k * n) * (size_t)a.C + t.c0;
    uint8_t *out0 = a.out + ((size_t)t.beam * a.out_spectra + a.first_out + (size_t)t.k * n) * (size_t)a.C + t.c0;
    const uint8_t *rowflag0 = a.spectrum_flags ? a.spectrum_flags + (size_t)t.beam * window + (size_t)t.k * n : nullptr;
    const bool lane_on = at_of<U>(0u, t.j, t.L) < t.width;
    const uint32_t fill = (a.fill & 0xffu) * kOnes;

    // once per tile: 0xff where the lane's channel is replaced in every row of this block, and where the lane has a channel
    uint32_t sel[4] = {0u, 0u, 0u, 0u}, have[4] = {0u, 0u, 0u, 0u};
    if (lane_on) {
        uint32_t f[4];
        if (a.channel_mask) {
            const uint8_t *p = a.channel_mask + (size_t)t.beam * a.C + t.c0;
            load16<U>(p, t.j, t.L, t.width, (reinterpret_cast<uintptr_t>(p) & (U - 1u)) == 0u, f);
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) sel[q] = ~nonzero_bytes(f[q]);
        }
        if (a.cell_flags) {
            const uint8_t *p = a.cell_flags + ((size_t)t.beam * a.nr_blocks + t.k) * a.C + t.c0;
            load16<U>(p, t.j, t.L, t.width, (reinterpret_cast<uintptr_t>(p) & (U - 1u)) == 0u, f);
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) sel[q] |= nonzero_bytes(f[q]);
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
#pragma unroll
            for (uint32_t e = 0; e < 4u; e++) {
                const uint32_t at = at_of<U>(4u * q + e, t.j, t.L);
                if (at < t.width) have[q] |= 0xffu << (8u * e);
            }
            sel[q] &= have[q];
        }
    }

    uint32_t replaced = 0u; // bytes: at most 16 * 65536
    // four rows of a lane in flight
    for (uint32_t t0 = 0; t0 < n; t0 += 4u * t.R) {
        uint32_t w[4][4], flagged[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t tt = t0 + u * t.R + t.r;
            flagged[u] = 0u;
            if (tt < n && lane_on) {
                load16<U>(in0 + (size_t)tt * a.C, t.j, t.L, t.width, true, w[u]);
                if (rowflag0) flagged[u] = rowflag0[tt];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t tt = t0 + u * t.R + t.r;
            if (tt < n && lane_on) {
                uint32_t o[4];
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) {
                    const uint32_t s = flagged[u] ? have[q] : sel[q];
                    o[q] = (w[u][q] & ~s) | (fill & s);
                    replaced += (uint32_t)__popc(s) >> 3;
                }
                store16<U>(out0 + (size_t)tt * a.C, t.j, t.L, t.width, o);
            }
        }
    }
    if (a.replaced) { // the same in every thread
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) replaced += (uint32_t)__shfl_xor((int)replaced, x);
        if ((threadIdx.x & 63u) == 0u && replaced) atomicAdd(a.replaced + t.beam, (unsigned long long)replaced);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the flags

// The element of rank `rank` (0-based, ascending) of the `count` >= 1 values value(i) < 2^bits, the same in every thread of
// the workgroup of NT threads: from the top down, TWO bits a pass -- the rank-th element is at or above a candidate iff at
// most `rank` elements lie below it, so the pass counts the elements below each of the three candidates that the two bits
// allow and keeps the largest that passes.  Four values of a thread are fetched before the first is compared.  One
// __syncthreads per pass; s_part is the waves' counts, double-buffered by the parity of `pass`, which the caller keeps
// across calls.  Every thread of the workgroup calls it.
template <uint32_t NT, class F>
__device__ uint64_t select_rank(F value, const uint32_t count, const uint32_t rank, const int bits, uint32_t (*s_part)[NT / 64u][3],
                                uint32_t &pass)
{
    const uint32_t tid = threadIdx.x;
    uint64_t found = 0u;
    for (int bit = (bits - 1) & ~1; bit >= 0; bit -= 2) {
        const uint64_t cand[3] = {found | (1ull << bit), found | (2ull << bit), found | (3ull << bit)};
        uint32_t below[3] = {0u, 0u, 0u}; // of the wave: a ballot's popcount is the same in every lane
        for (uint64_t i0 = 0; i0 < count; i0 += 4u * NT) {
            uint64_t v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
                const uint64_t i = i0 + u * NT + tid;
                v[u] = i < count ? value((uint32_t)i) : ~0ull; // no value is at or above 2^63: never below a candidate
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
#pragma unroll
                for (uint32_t k = 0; k < 3u; k++) below[k] += (uint32_t)__popcll(__ballot(v[u] < cand[k]));
        }
        if ((tid & 63u) == 0u)
#pragma unroll
            for (uint32_t k = 0; k < 3u; k++) s_part[pass & 1u][tid >> 6][k] = below[k];
        __syncthreads();
        uint32_t total[3] = {0u, 0u, 0u};
#pragma unroll
        for (uint32_t w = 0; w < NT / 64u; w++)
#pragma unroll
            for (uint32_t k = 0; k < 3u; k++) total[k] += s_part[pass & 1u][w][k];
        pass++;
        found = total[2] <= rank ? cand[2] : total[1] <= rank ? cand[1] : total[0] <= rank ? cand[0] : found;
    }
    return found;
}

__device__ __forceinline__ uint64_t distance(const uint64_t v, const uint64_t med) { return v > med ? v - med : med - v; }

// limit = fmax(RN64(thr * (double)mad), floor): one multiply, rounded once (the build has -ffp-contract=off)
__device__ __forceinline__ double outlier_limit(const double thr, const uint64_t mad, const double floor)
{
    return fmax(thr * (double)mad, floor);
}

// the sum of v over the workgroup of NT threads, in every thread; s is free before the call and after it
template <uint32_t NT>
__device__ uint32_t block_sum(uint32_t v, uint32_t *s)
{
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) v += (uint32_t)__shfl_xor((int)v, x);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < NT / 64u; w++) total += s[w];
    return total;
}

constexpr uint32_t kCellCache = 4096;    // channels whose m and q a workgroup keeps in LDS: 48 KiB
constexpr uint32_t kBeamThreads = 1024;  // of the workgroup that owns a beam
constexpr uint32_t kBeamWords = 16;      // zero-DM words a thread of it keeps in registers: windows to 16384 spectra

// One workgroup per (beam, block): the flags of its C cells.  Up to kCellCache channels, m and q are worked out once into
// LDS and every pass reads them there; beyond that every pass makes them again from the cell sums in global memory.
__global__ void __launch_bounds__(kThreads) bf_rfi_cell_flags_kernel(const bf_rfi_flags_args a)
{
    __shared__ uint64_t s_q[kCellCache];
    __shared__ uint32_t s_m[kCellCache];
    __shared__ uint32_t s_part[2][kThreads / 64u][3];
    const uint32_t C = a.C, k = blockIdx.x % a.nr_blocks, beam = blockIdx.x / a.nr_blocks;
    const uint64_t n = a.block_len;
    const uint2 *cs = reinterpret_cast<const uint2 *>(a.cell_sums) + ((size_t)beam * a.nr_blocks + k) * C;
    const bool cached = C <= kCellCache; // the same in every thread
    auto q_of = [&](const uint2 s) -> uint64_t { return n * s.y - (uint64_t)s.x * s.x; };
    if (cached) {
        for (uint32_t c = threadIdx.x; c < C; c += kThreads) {
            const uint2 s = cs[c];
            s_m[c] = s.x;
            s_q[c] = q_of(s);
        }
        __syncthreads();
    }
    auto m = [&](const uint32_t c) -> uint64_t { return cached ? s_m[c] : cs[c].x; };
    auto q = [&](const uint32_t c) -> uint64_t { return cached ? s_q[c] : q_of(cs[c]); };
    const uint32_t rank = (C - 1u) >> 1;
    uint32_t pass = 0u;
    const uint64_t med_m = select_rank<kThreads>(m, C, rank, 24, s_part, pass);
    const uint64_t mad_m = select_rank<kThreads>([&](const uint32_t c) { return distance(m(c), med_m); }, C, rank, 24, s_part, pass);
    const uint64_t med_q = select_rank<kThreads>(q, C, rank, 49, s_part, pass);
    const uint64_t mad_q = select_rank<kThreads>([&](const uint32_t c) { return distance(q(c), med_q); }, C, rank, 49, s_part, pass);
    const double lim_m = outlier_limit(a.mean_thr, mad_m, a.mean_floor), lim_q = outlier_limit(a.var_thr, mad_q, a.var_floor);
    uint8_t *flags = a.cell_flags + ((size_t)beam * a.nr_blocks + k) * C;
    for (uint32_t c = threadIdx.x; c < C; c += kThreads) {
        const uint32_t f = ((double)distance(m(c), med_m) > lim_m ? 1u : 0u) | ((double)distance(q(c), med_q) > lim_q ? 2u : 0u);
        flags[c] = (uint8_t)f;
    }
}

// One workgroup of kBeamThreads per beam: the channel mask from the cell flags, the spectrum flags from the zero-DM series,
// the counts.  A window of up to kBeamThreads * kBeamWords spectra is read once into registers, word u kBeamThreads + tid
// in register u of thread tid, and every pass of the two bisections compares registers; a longer one is read from global
// memory in every pass.
__global__ void __launch_bounds__(kBeamThreads) bf_rfi_beam_kernel(const bf_rfi_flags_args a)
{
    __shared__ uint32_t s_part[2][kBeamThreads / 64u][3];
    __shared__ uint32_t s_sum[kBeamThreads / 64u];
    const uint32_t C = a.C, beam = blockIdx.x, tid = threadIdx.x;
    uint32_t cells = 0u, masked = 0u, spectra = 0u;
    for (uint32_t c = tid; c < C; c += kBeamThreads) {
        uint32_t bad = 0u;
        const uint8_t *f = a.cell_flags + (size_t)beam * a.nr_blocks * C + c;
        // eight loads before the first compare: few workgroups run, so nothing else hides the latency
        uint32_t k = 0;
        for (; k + 8u <= a.nr_blocks; k += 8u) {
            uint32_t v[8];
#pragma unroll
            for (uint32_t u = 0; u < 8u; u++) v[u] = f[(size_t)(k + u) * C];
#pragma unroll
            for (uint32_t u = 0; u < 8u; u++) bad += v[u] != 0u ? 1u : 0u;
        }
        for (; k < a.nr_blocks; k++) bad += f[(size_t)k * C] != 0u ? 1u : 0u;
        cells += bad;
        const uint32_t keep = bad > a.max_bad_blocks ? 0u : 1u;
        a.channel_mask[(size_t)beam * C + c] = (uint8_t)keep;
        masked += 1u - keep;
    }
    const uint64_t window = (uint64_t)a.nr_blocks * a.block_len; // <= 2^32 - 1
    if (a.zero_dm && window) {
        const uint32_t W = (uint32_t)window, rank = (W - 1u) >> 1;
        const uint32_t *z = a.zero_dm + (size_t)beam * window;
        uint8_t *flags = a.spectrum_flags + (size_t)beam * window;
        uint32_t pass = 0u;
        if (W <= kBeamThreads * kBeamWords) {
            uint32_t v[kBeamWords];
#pragma unroll
            for (uint32_t u = 0; u < kBeamWords; u++) v[u] = u * kBeamThreads + tid < W ? z[u * kBeamThreads + tid] : 0u;
            // select_rank's bisection on the registers, one bit a pass: word u of this thread, or its distance from med
            auto rank_of = [&](const bool from_med, const uint32_t med) -> uint32_t {
                uint32_t found = 0u;
                for (int bit = 31; bit >= 0; bit--) {
                    const uint32_t cand = found | (1u << bit);
                    uint32_t below = 0u;
#pragma unroll
                    for (uint32_t u = 0; u < kBeamWords; u++) {
                        const uint32_t x = from_med ? (v[u] > med ? v[u] - med : med - v[u]) : v[u];
                        below += (uint32_t)__popcll(__ballot(u * kBeamThreads + tid < W && x < cand));
                    }
                    if ((tid & 63u) == 0u) s_part[pass & 1u][tid >> 6][0] = below;
                    __syncthreads();
                    uint32_t total = 0u;
#pragma unroll
                    for (uint32_t w = 0; w < kBeamThreads / 64u; w++) total += s_part[pass & 1u][w][0];
                    pass++;
                    if (total <= rank) found = cand;
                }
                return found;
            };
            const uint32_t med = rank_of(false, 0u);
            const uint32_t mad = rank_of(true, med);
            const double lim = outlier_limit(a.zero_dm_thr, mad, a.zero_dm_floor);
#pragma unroll
            for (uint32_t u = 0; u < kBeamWords; u++) {
                const uint32_t i = u * kBeamThreads + tid;
                if (i < W) {
                    const uint32_t f = (double)distance(v[u], med) > lim ? 1u : 0u;
                    flags[i] = (uint8_t)f;
                    spectra += f;
                }
            }
        } else {
            const uint64_t med = select_rank<kBeamThreads>([&](const uint32_t i) -> uint64_t { return z[i]; }, W, rank, 32, s_part, pass);
            const uint64_t mad = select_rank<kBeamThreads>([&](const uint32_t i) { return distance(z[i], med); }, W, rank, 32, s_part, pass);
            const double lim = outlier_limit(a.zero_dm_thr, mad, a.zero_dm_floor);
            for (uint64_t i = tid; i < window; i += kBeamThreads) {
                const uint32_t f = (double)distance(z[i], med) > lim ? 1u : 0u;
                flags[i] = (uint8_t)f;
                spectra += f;
            }
        }
    }
    cells = block_sum<kBeamThreads>(cells, s_sum);
    masked = block_sum<kBeamThreads>(masked, s_sum);
    spectra = block_sum<kBeamThreads>(spectra, s_sum);
    if (tid == 0u) {
        a.counts[3u * (size_t)beam] = cells;
        a.counts[3u * (size_t)beam + 1u] = masked;
        a.counts[3u * (size_t)beam + 2u] = spectra;
    }
}

// lanes of 16 channels that a row of C channels needs, as a power of two <= kMaxLanes
uint32_t lanes_of(const uint32_t C)
{
    const uint32_t need = (C + kLaneChannels - 1u) / kLaneChannels;
    uint32_t lanes = 1u;
    while (lanes < need && lanes < kMaxLanes) lanes <<= 1;
    return lanes;
}

// the grid of the two hot kernels, 0 where it does not fit one
uint32_t hot_grid(const uint32_t C, const uint32_t B, const uint32_t nr_blocks, uint32_t &lanes, uint32_t &tiles)
{
    lanes = lanes_of(C);
    tiles = (C - 1u) / (kLaneChannels * lanes) + 1u;
    const unsigned __int128 blocks = (unsigned __int128)B * nr_blocks * tiles;
    return blocks > 0x7fffffffull ? 0u : (uint32_t)blocks;
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_rfi()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_rfi_beam_kernel));
}

static hipError_t bf_launch_rfi_moments(const bf_rfi_moments_args &args, hipStream_t stream)
{
    if (args.nr_blocks == 0u || args.B == 0u || args.C == 0u) return hipSuccess;
    bf_rfi_moments_args a = args;
    const uint32_t blocks = hot_grid(a.C, a.B, a.nr_blocks, a.lanes, a.tiles);
    if (blocks == 0u) return hipErrorInvalidValue;
    if (a.zero_dm) {
        const hipError_t e = hipMemsetAsync(a.zero_dm, 0, (size_t)a.B * a.nr_blocks * a.block_len * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    if (a.C % 16u == 0u)
        hipLaunchKernelGGL(bf_rfi_moments_kernel<16u>, dim3(blocks), dim3(kThreads), 0, stream, a);
    else if (a.C % 4u == 0u)
        hipLaunchKernelGGL(bf_rfi_moments_kernel<4u>, dim3(blocks), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(bf_rfi_moments_kernel<1u>, dim3(blocks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_rfi_flags(const bf_rfi_flags_args &a, hipStream_t stream)
{
    if (a.B == 0u || a.C == 0u) return hipSuccess;
    const uint64_t cells = (uint64_t)a.B * a.nr_blocks;
    if (cells > 0x7fffffffull) return hipErrorInvalidValue;
    if (cells) hipLaunchKernelGGL(bf_rfi_cell_flags_kernel, dim3((uint32_t)cells), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(bf_rfi_beam_kernel, dim3(a.B), dim3(kBeamThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_rfi_clean(const bf_rfi_clean_args &args, hipStream_t stream)
{
    if (args.nr_blocks == 0u || args.B == 0u || args.C == 0u) return hipSuccess;
    bf_rfi_clean_args a = args;
    const uint32_t blocks = hot_grid(a.C, a.B, a.nr_blocks, a.lanes, a.tiles);
    if (blocks == 0u) return hipErrorInvalidValue;
    if (a.C % 16u == 0u)
        hipLaunchKernelGGL(bf_rfi_clean_kernel<16u>, dim3(blocks), dim3(kThreads), 0, stream, a);
    else if (a.C % 4u == 0u)
        hipLaunchKernelGGL(bf_rfi_clean_kernel<4u>, dim3(blocks), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(bf_rfi_clean_kernel<1u>, dim3(blocks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

// The host side of include/dcs_rfi.h, behind the table as in bf_integrate.hip.  Nothing allocated; of the context the channel
// count and the device are used.  The sizes that need C are checked here; the thresholds are host memory and travel by value
// in the kernels' arguments.
namespace bf_host {

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
