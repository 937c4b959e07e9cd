// bf_correlator.hip -- the int8 correlator on the matrix cores (include/dcs_correlator.h), gfx950
// only: the exact visibilities V[a][b] = sum_t x_a[t] conj(x_b[t]), b <= a, of the antenna tensor
// int8 [C][nt / 16][A][16][{re, im}], summed over n = blocks_per_vis blocks of 16 samples, as int32 [C][nr_vis][NB][{re, im}].
// Every term is an integer and no sum leaves int32 (n <= 4095), so any order of summation gives the same bits.
//
// The contraction is v_mfma_i32_16x16x64_i8 on 16-antenna tiles.  Both operands of a product take their K index from the
// same sample bytes, so ANY assignment of a lane's 16 operand bytes to K is right as long as both operands use the same one;
// and here they do by construction, because a tile has ONE pair of operands that serves as the row operand of the tile
// pairs it is the a side of and as the column operand of those it is the b side of:
//
//  * lane (lm = lane & 15, lg = lane >> 4) of a tile loads, per pair of blocks, the 16 bytes -- 8 samples -- of half
//    (lg & 1) of antenna 16 tile + lm in block (lg >> 1) of the pair: one global_load_dwordx4, no LDS, no transpose.  A step
//    is four blocks: two such loads per tile;
//  * eight v_perm_b32 de-interleave the two loads into a re-only and an im-only operand of K = 64 (16 samples of each of
//    four blocks between the four lane groups), no K wasted on zeros;
//  * a tile pair takes four MFMAs per step into three accumulators: Re Re^T and Im Im^T into re, Im_a Re_b^T into p and
//    Re_a Im_b^T into q; the epilogue stores (re, p - q).  No byte is negated anywhere: -(-128) is no int8;
//  * blocks past n in the last step (n % 4 != 0) are zero operands: the load reads a block that exists and is masked;
//  * a load's address is a wave-uniform 64-bit base (scalar registers) plus a 32-bit lane offset.
//
// A wave owns a unit of one (channel, visibility).  On the diagonal it is a square of kS x kS tiles (64 x 64 antennas), of
// which it computes the pairs with b_tile <= a_tile from one set of tiles for both sides: A <= 64 is one such unit, ten tile
// pairs from four tiles' loads.  Off the diagonal it is kS a tiles against kSB b tiles, eight tile pairs from six tiles'
// loads: a square of the strict lower triangle is kS / kSB units.  A = 256 has 4 + 6 * 2 = 16 units per (channel, visibility).
// The a tiles that exist are a template parameter (1 .. kS, chosen by a wave-uniform switch), so a ragged or small A costs
// what it needs and a step is straight-line code.  The work item is (channel, visibility, unit), so a small C * nr_vis still
// spreads; where there are several units, the workgroups of one XCD take consecutive items, and the units of a (channel,
// visibility) re-read its samples through that L2.
// A step builds its operands, issues the next step's loads into the registers that this has freed, and then its MFMAs (two
// scheduling fences hold that order); the last step, the only one that can hold blocks past n, is peeled and masks.  The
// launch bound asks for two waves per SIMD (the register report is in DESIGN.md).
//
// Result: register r of lane (lm, lg) of a tile pair is row a = 16 a_tile + 4 lg + r, column b = 16 b_tile + lm.  Row a of
// the triangle begins at word pair a (a + 1) / 2, which is aligned to 8 bytes and no more, so the store is one (re, im)
// dwordx2 per lane and register: the 16 lanes of a group write 128 contiguous bytes of one row.  A diagonal tile stores its
// b <= a half; rows and columns past A are not stored (their loads are clamped to antenna A - 1).  Every word is written
// once, by a plain store.  Byte offsets are 64-bit.  No LDS, no barrier, no scratch (the register report is in DESIGN.md).

#include "bf_host.h"

#include <hip/hip_runtime.h>

#include <type_traits>

// The correlator (include/dcs_correlator.h): the sample tensor
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

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kS = 4;     // tiles along an edge of a wave's unit: 64 antennas (correlate_unit is instantiated for 1 .. 4)
constexpr uint32_t kSB = 2;    // b tiles of a unit off the diagonal: kS x kSB tile pairs (4 x 4 needs 368 registers: one wave per SIMD)
static_assert(kSB >= 1u && kS % kSB == 0u, "a square of tiles off the diagonal is whole units");
constexpr uint32_t kWaves = 4; // waves per workgroup, one unit each
constexpr uint32_t kGrid = 1u << 20; // workgroups at most; the waves walk the items beyond

constexpr uint32_t kSelRe = 0x06040200u; // bytes 0, 2 of the low dword and 0, 2 of the high one: four real parts
constexpr uint32_t kSelIm = 0x07050301u; // bytes 1, 3 of each: four imaginary parts

struct tile_ops {
    intx4 re, im; // K = 64 between the four lane groups: 16 samples of one antenna from each of four blocks
};

// the two loads of one tile and step
struct tile_raw {
    intx4 p[2];
};

__device__ __forceinline__ uint32_t perm(const int hi, const int lo, const uint32_t sel)
{
    return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, sel);
}

// MASKED (the last step only: every block of a step that another follows exists): keep0, keep1 are all ones, or zero where
// the lane's block of that load lies past the visibility: a zero operand.  The mask is applied here, at the use, so that
// nothing waits for a load where it is issued
template <bool MASKED>
__device__ __forceinline__ tile_ops deinterleave(const tile_raw &x, const int keep0, const int keep1)
{
    tile_ops o;
    if (!MASKED) {
        o.re = intx4{(int)perm(x.p[0].y, x.p[0].x, kSelRe), (int)perm(x.p[0].w, x.p[0].z, kSelRe), (int)perm(x.p[1].y, x.p[1].x, kSelRe),
                     (int)perm(x.p[1].w, x.p[1].z, kSelRe)};
        o.im = intx4{(int)perm(x.p[0].y, x.p[0].x, kSelIm), (int)perm(x.p[0].w, x.p[0].z, kSelIm), (int)perm(x.p[1].y, x.p[1].x, kSelIm),
                     (int)perm(x.p[1].w, x.p[1].z, kSelIm)};
        return o;
    }
    o.re = intx4{(int)perm(x.p[0].y, x.p[0].x, kSelRe) & keep0, (int)perm(x.p[0].w, x.p[0].z, kSelRe) & keep0,
                 (int)perm(x.p[1].y, x.p[1].x, kSelRe) & keep1, (int)perm(x.p[1].w, x.p[1].z, kSelRe) & keep1};
    o.im = intx4{(int)perm(x.p[0].y, x.p[0].x, kSelIm) & keep0, (int)perm(x.p[0].w, x.p[0].z, kSelIm) & keep0,
                 (int)perm(x.p[1].y, x.p[1].x, kSelIm) & keep1, (int)perm(x.p[1].w, x.p[1].z, kSelIm) & keep1};
    return o;
}

// What a wave needs to load a step: the visibility's first block (wave-uniform) and, per lane, its block inside a pair
struct wave_src {
    const char *vis0;   // block 0 of the visibility
    uint64_t blk_bytes; // A * 32
    uint32_t lb;        // lg >> 1
    uint32_t n;         // blocks of the visibility
};

// The loads of step s: lane group lg reads half (lg & 1) of block 4 s + 2 p + lb, p = 0, 1.  The address is a wave-uniform
// 64-bit base -- block min(4 s + 2 p, n - 1) -- plus a 32-bit lane offset: add[p] here, the same for every tile (the step
// to block + 1 for the lanes with lb = 1 where that block exists), and the tile's own off (antenna and half).  A block
// past n - 1 is so read as one that exists, and masked at its use
struct step_src {
    const char *base[2];
    uint32_t add[2];
};

__device__ __forceinline__ step_src step_of(const wave_src &src, const uint32_t s)
{
    step_src st;
#pragma unroll
    for (uint32_t p = 0; p < 2u; p++) {
        const uint32_t blk = 4u * s + 2u * p < src.n ? 4u * s + 2u * p : src.n - 1u;
        st.base[p] = src.vis0 + (uint64_t)blk * src.blk_bytes;
        st.add[p] = blk + src.lb < src.n ? src.lb * (uint32_t)src.blk_bytes : 0u;
    }
    return st;
}

__device__ __forceinline__ tile_raw load_tile(const step_src &st, const uint32_t off)
{
    tile_raw x;
#pragma unroll
    for (uint32_t p = 0; p < 2u; p++) x.p[p] = *reinterpret_cast<const intx4 *>(st.base[p] + (st.add[p] + off));
    return x;
}

// One unit of (channel, visibility) cv: the a tiles sa kS .. against the b tiles bt0 .. .  DIAG: bt0 == sa kS, the pairs with
// b <= a; else kSB b tiles below the a tiles, which all exist.  NA: the a tiles that exist (a template parameter, so that the
// steps are straight-line code on registers known at compile time)
template <bool DIAG, uint32_t NA>
__device__ __forceinline__ void correlate_unit(const bf_corr_args &a, const uint64_t cv, const uint32_t sa, const uint32_t bt0)
{
    const uint32_t lane = threadIdx.x & 63u, lm = lane & 15u, lg = lane >> 4;
    const uint32_t steps = (a.n + 3u) / 4u;
    {
        const uint64_t c = cv / a.nr_vis, vis = cv % a.nr_vis;
        wave_src src;
        src.blk_bytes = (uint64_t)a.A * 32u;
        src.vis0 = reinterpret_cast<const char *>(a.ant) + (c * a.nT16 + vis * a.n) * src.blk_bytes;
        src.lb = lg >> 1;
        src.n = a.n;
        // the lane's antenna of every tile, clamped in bounds, and its half of the antenna's row
        uint32_t offa[kS], offb[kSB];
#pragma unroll
        for (uint32_t i = 0; i < kS; i++) {
            const uint32_t ra = (sa * kS + i) * 16u + lm;
            offa[i] = (ra < a.A ? ra : a.A - 1u) * 32u + (lg & 1u) * 16u;
        }
#pragma unroll
        for (uint32_t j = 0; j < kSB; j++) {
            const uint32_t rb = (bt0 + j) * 16u + lm;
            offb[j] = (rb < a.A ? rb : a.A - 1u) * 32u + (lg & 1u) * 16u;
        }
        constexpr uint32_t NBT = DIAG ? NA : kSB;
        intx4 acc_re[NA][NBT], acc_p[NA][NBT], acc_q[NA][NBT];
#pragma unroll
        for (uint32_t i = 0; i < NA; i++)
#pragma unroll
            for (uint32_t j = 0; j < NBT; j++) acc_re[i][j] = acc_p[i][j] = acc_q[i][j] = intx4{0, 0, 0, 0};

        tile_raw rawa[kS], rawb[kSB];
        {
            const step_src first = step_of(src, 0u);
#pragma unroll
            for (uint32_t i = 0; i < NA; i++) rawa[i] = load_tile(first, offa[i]);
            if (!DIAG) {
#pragma unroll
                for (uint32_t j = 0; j < kSB; j++) rawb[j] = load_tile(first, offb[j]);
            }
        }
        // one step: s, and whether another follows it (a constant at each of the two calls: the body is one basic block)
        auto step = [&](const uint32_t s, auto more_t) __attribute__((always_inline)) {
            constexpr bool more = decltype(more_t)::value;
            tile_ops opa[kS], opb[kSB];
            const int keep0 = 4u * s + src.lb < a.n ? -1 : 0, keep1 = 4u * s + 2u + src.lb < a.n ? -1 : 0;
#pragma unroll
            for (uint32_t i = 0; i < NA; i++) opa[i] = deinterleave<!more>(rawa[i], keep0, keep1);
            if (!DIAG) {
#pragma unroll
                for (uint32_t j = 0; j < kSB; j++) opb[j] = deinterleave<!more>(rawb[j], keep0, keep1);
            }
            // the operands first, then the next loads into the registers they have freed: without the fence the compiler
            // issues the loads first and keeps a second set of load registers, which costs a wave per SIMD
            __builtin_amdgcn_sched_barrier(0);
            if (more) {
                const step_src next = step_of(src, s + 1u);
#pragma unroll
                for (uint32_t i = 0; i < NA; i++) rawa[i] = load_tile(next, offa[i]);
                if (!DIAG) {
#pragma unroll
                    for (uint32_t j = 0; j < kSB; j++) rawb[j] = load_tile(next, offb[j]);
                }
                __builtin_amdgcn_sched_barrier(0); // and every load before the first MFMA: they fly while the MFMAs issue
            }
#pragma unroll
            for (uint32_t i = 0; i < NA; i++) {
#pragma unroll
                for (uint32_t j = 0; j < NBT; j++) {
                    if (DIAG && j > i) continue;
                    const tile_ops &x = opa[i];
                    const tile_ops &y = DIAG ? opa[j] : opb[j];
                    acc_re[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x.re, y.re, acc_re[i][j], 0, 0, 0);
                    acc_re[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x.im, y.im, acc_re[i][j], 0, 0, 0);
                    acc_p[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x.im, y.re, acc_p[i][j], 0, 0, 0);
                    acc_q[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x.re, y.im, acc_q[i][j], 0, 0, 0);
                }
            }
        };
        for (uint32_t s = 0; s + 1u < steps; s++) step(s, std::true_type{});
        step(steps - 1u, std::false_type{});
        // register r: row 16 a_tile + 4 lg + r, column 16 b_tile + lm
        char *out = reinterpret_cast<char *>(a.vis) + cv * a.NB * 8u;
#pragma unroll
        for (uint32_t i = 0; i < NA; i++) {
#pragma unroll
            for (uint32_t j = 0; j < NBT; j++) {
                if (DIAG && j > i) continue;
                const uint32_t col = (bt0 + j) * 16u + lm;
#pragma unroll
                for (uint32_t r = 0; r < 4u; r++) {
                    const uint32_t row = (sa * kS + i) * 16u + 4u * lg + r;
                    if (row < a.A && col <= row) // col <= row < A
                        *reinterpret_cast<intx2 *>(out + ((uint64_t)(row * (row + 1u) / 2u + col) * 8u)) =
                            intx2{acc_re[i][j][r], acc_p[i][j][r] - acc_q[i][j][r]};
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kWaves * 64, 2) bf_correlate_kernel(const bf_corr_args a)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    // The workgroups that share blockIdx.x % 8 -- observed: one XCD, one L2 -- take consecutive items, so the units of a
    // (channel, visibility) re-read its samples through one L2.  For speed only: gridDim.x % 8 == 0 (the launcher) makes the
    // renumbering a bijection wherever the workgroups run.  With one unit there is nothing to share, and neighbouring
    // workgroups on neighbouring samples read faster
    const uint32_t wg = a.units > 1u ? (blockIdx.x % 8u) * (gridDim.x / 8u) + blockIdx.x / 8u : blockIdx.x;
    for (uint64_t item = (uint64_t)wg * kWaves + wave; item < a.items; item += nwaves) {
        // unit u of a (channel, visibility): the a.st squares of kS x kS tiles on the diagonal first, then the squares (sa, sb),
        // sb < sa, of the strict lower triangle, kS / kSB units each
        const uint32_t u = (uint32_t)(item % a.units);
        const uint64_t cv = item / a.units; // c * nr_vis + visibility
        if (u < a.st) {
            switch (a.tiles - u * kS) { // the a tiles of the unit that exist, kS at most
            case 1: correlate_unit<true, 1>(a, cv, u, u * kS); break;
            case 2: correlate_unit<true, 2>(a, cv, u, u * kS); break;
            case 3: correlate_unit<true, 3>(a, cv, u, u * kS); break;
            default: correlate_unit<true, 4>(a, cv, u, u * kS); break;
            }
        } else {
            const uint32_t v = u - a.st, w = v / (kS / kSB);
            uint32_t sa = 1;
            while (sa * (sa + 1u) / 2u <= w) sa++;
            const uint32_t bt0 = (w - sa * (sa - 1u) / 2u) * kS + v % (kS / kSB) * kSB;
            switch (a.tiles - sa * kS) {
            case 1: correlate_unit<false, 1>(a, cv, sa, bt0); break;
            case 2: correlate_unit<false, 2>(a, cv, sa, bt0); break;
            case 3: correlate_unit<false, 3>(a, cv, sa, bt0); break;
            default: correlate_unit<false, 4>(a, cv, sa, bt0); break;
            }
        }
    }
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_correlator()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_correlate_kernel));
}

static hipError_t bf_launch_correlate(const bf_corr_args &args, hipStream_t stream)
{
    if (args.C == 0u || args.nr_vis == 0u) return hipSuccess;
    if (args.A == 0u || args.A > 256u || args.n == 0u) return hipErrorInvalidValue;
    bf_corr_args a = args;
    a.tiles = (a.A + 15u) / 16u;
    a.NB = (uint64_t)a.A * (a.A + 1u) / 2u;
    a.st = (a.tiles + kS - 1u) / kS;
    a.units = a.st + a.st * (a.st - 1u) / 2u * (kS / kSB);
    a.items = (uint64_t)a.C * a.nr_vis * a.units;
    const uint64_t blocks = (a.items + kWaves - 1u) / kWaves;
    const uint32_t grid = ((uint32_t)(blocks < kGrid ? blocks : kGrid) + 7u) & ~7u; // a multiple of 8: the kernel's renumbering
    hipLaunchKernelGGL(bf_correlate_kernel, dim3(grid), dim3(kWaves * 64u), 0, stream, a);
    return hipGetLastError();
}

// The host side of include/dcs_correlator.h, behind the table as in bf_integrate.hip.  No coefficients, nothing allocated, and
// math_mode plays no part.
namespace bf_host {

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

} // namespace bf_host
