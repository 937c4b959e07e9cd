// bf_beamform_mfma.hip -- beamformer with coefficient REUSE on the gfx950 matrix cores
// ("a general version is a contraction over antennas").
//
// The reference regenerates every steering coefficient for every time sample
// (calculate_beamweights_and_beamform_single_channel, BeamformerKernels.cu:192-367) and only MODELS
// what a deployed beamformer does: new coefficients every ACCUMULATIONS_BEFORE_NEW_COEFFS time units
// (BeamformerParameters.h:17; BeamformerCoefficientTest.cu:426-448).  Here the coefficients of ONE time
// are generated once per (channel, antenna, beam) -- into registers or LDS, never HBM -- and applied to a
// block of samples:
//   beams[c][t/16][b][t%16] = ( sum_a cos(rot[a][b][c]) * re[c][t][a] ,  sum_a sin(rot[a][b][c]) * im[c][t][a] )
// (the reference's element-wise product, BeamformerKernels.cu:315-316; table indexed [b*A + a]; layouts
// BeamformerKernels.cuh:137-143).  Per channel that is two real contractions over antennas,
//   Re[beam][t] = Wre[beam][ant] x Sre[ant][t]      Im likewise.
// Roofline: int8 samples in (2 B per antenna and sample) + fp32 beams out (8 B per beam and sample) against HBM.
//
// Two forms (bf_bacc_args.fp32_chain):
//
// 1. bf_beamform_i8_kernel (default; second half of this file): the contraction in EXACT integer arithmetic on
//    v_mfma_i32_16x16x64_i8 -- 24-bit fixed-point coefficients as three signed digits -- which takes the matrix
//    work out of the picture (32 x the fp32 pipe's rate) and leaves a kernel bound by the memory system:
//    at 16 beams (as many bytes in as out) 5.0-5.7 TB/s, 80-90 % of what the leanest device copy kernel moves on
//    the same box (6.3 TB/s) and more than hipMemcpyDtoD (5.0); at >= 64 beams (output-dominated) 4.7-4.9 TB/s, the
//    rate this chip gives long-lived waves that each stream 64 stores (profiles/r01_store_patterns.md: 5.4-5.5).
//
// 2. bf_beamform_acc_kernel (first half): v_mfma_f32_16x16x4_f32, exact-fp32 products accumulated as an fp32 fma
//    chain IN ANTENNA ORDER (the instruction is, bit for bit, a k-ordered fmaf chain), so the result differs from
//    the verifier's "sum += coeff * sample" (separate multiply and add) by the roundings of the chain only.
//    Workgroup = 4 waves = one channel x NBT beam tiles of 16 x a range of 16-sample blocks:
//      wave w: beam tile w % NBT, sample-block slot w / NBT of each round (4 / NBT blocks per round).
//    A lane reads the (re, im) int8 pair of its own B operand straight from global memory (one 2-byte load per
//    k-step), one stage ahead of the matrix pipe, and converts it on the VALU.  W (all antennas x 16*NBT beams,
//    re and im planes) is generated once per workgroup into LDS from the terms table bf_bform_terms_kernel
//    writes ([a][b]; L2-resident) -- the kernel's only barrier -- and read from there, one ds_read_b32 per A
//    operand.  0.38-0.53 of the fp32 matrix peak across six structures (profiles/r02_fused.md); kept as the form
//    whose rounding is the verifier's loop with fused multiply-adds.
//      A operand, lane l: W[beam l & 15][antenna 4j + (l >> 4)]   B operand: S[antenna 4j + (l >> 4)][sample l & 15]
//    C/D: lane l, register r = beam (l >> 4) * 4 + r, sample l & 15.

#include "bf_kernels.h"

#include <hip/hip_runtime.h>

#include <tuple>
#include <type_traits>

#include "bf_device.h"

namespace {

// Workgroup numbering, XCD-aware.  The hardware hands workgroup w to XCD w % 8, and every XCD has its own L2.  The
// logical order below is beam group fastest, then sample-block group, then channel: the n_bgroups workgroups that
// read the SAME samples (one channel's blocks) are neighbours in it.  Numbered as dispatched, those neighbours land on
// different XCDs and each L2 fetches the samples again (FETCH_SIZE 4.0 x the algorithmic input at 64 x 256 beams,
// profiles/r02_fused.md -- served by the 256 MiB Infinity Cache behind the L2s, not by HBM, as it turned out).  With
// G = a.xcd_group > 1 the dispatch number w (XCD x = w % 8, that XCD's q-th workgroup, q = w / 8) becomes the logical
// number of member q % G of sharer group (q / G) * 8 + x: the G sharers follow each other on ONE XCD -- all but the
// first hit its L2 (FETCH_SIZE 1.04 x) -- while the eight XCDs still work on eight NEIGHBOURING groups at any moment.
// (Giving every XCD one contiguous eighth of the order instead keeps the sharers together just as well, but sends the
// XCDs to eight far-apart address windows: 6 % slower where there is nothing to share.)  A bijection: on the whole
// multiples of 8 G by construction, identity on the tail; identity altogether for G = 1.  The launcher decides G from
// measurements (profiles/r03_fused.md): the sharers' count for the forms of more than 64 antennas (each workgroup reads
// 4 x what it writes: -18 % time), and for the staged form from 16 sharers on (+3.5 %; at 2 - 8 sharers the grouped
// order measured 1.5 - 7 % SLOWER -- four workgroups missing on the same lines of one L2 at the same moment -- so those
// stay as dispatched).
// (the function itself: bf_kernels.h, bf_xcd_grouped -- host-callable too, so that tests/test_host_abi.py can check the
// bijection on the CPU through probes/libdcs_probes.so)
__device__ __forceinline__ uint32_t xcd_grouped(uint32_t w, uint32_t total, uint32_t G) { return bf_xcd_grouped(w, total, G); }
#ifdef DCS_PROBES
// A/B of the numbering (dcs_probe_knobs.bacc_order): 0 = the launcher's choice, 1 = as dispatched (round 2), 2 = one
// contiguous eighth of the order per XCD, 3 = sharers grouped whatever their number
__device__ __forceinline__ uint32_t probe_order(uint32_t order, uint32_t w, uint32_t total, uint32_t G, uint32_t n_sharers)
{
    if (order == 1u) return w;
    if (order >= 16u && order < 24u) return (w + (order - 16u)) % total; // 16 + r: as dispatched, rotated by r (XCD <-> channel affinity probe)
    if (order == 2u) {
        const uint32_t per = total >> 3, rem = total & 7u, x = w & 7u, q = w >> 3;
        return x * per + min(x, rem) + q;
    }
    return xcd_grouped(w, total, order == 3u ? n_sharers : G);
}
#define BACC_LOGICAL_ID(a) probe_order((a).order, blockIdx.x, gridDim.x, (a).xcd_group, (a).n_bgroups)
#else
#define BACC_LOGICAL_ID(a) xcd_grouped(blockIdx.x, gridDim.x, (a).xcd_group)
#endif

constexpr uint32_t kKC = 64; // antennas per staged chunk (16 k-steps of 4)

template <int NBT>
__global__ void __launch_bounds__(kBlock) bf_beamform_acc_kernel(const bf_bacc_args a)
{
    constexpr int TPR = 4 / NBT;                                  // 16-sample blocks per round
    constexpr uint32_t WS = 16u * NBT + (NBT > 1 ? 16u : 0u);     // W row stride in floats (padded: no bank conflict)
    constexpr uint32_t NJ = kKC / 4u;                             // k-steps per chunk
    extern __shared__ __attribute__((aligned(16))) float lds[];   // Wre[A_pad][WS] | Wim[A_pad][WS]
    const uint32_t A_pad = (a.A + 3u) & ~3u;

    uint32_t bid = BACC_LOGICAL_ID(a);
    const uint32_t bg = bid % a.n_bgroups;
    bid /= a.n_bgroups;
    const uint32_t tg = bid % a.n_tgroups;
    const uint32_t c = bid / a.n_tgroups;
    const uint32_t b0 = bg * 16u * NBT;            // first beam of this workgroup
    const uint32_t tt0 = tg * a.tiles_per_wg;      // first 16-sample block
    const uint32_t tt1 = min(tt0 + a.tiles_per_wg, a.nT16);

    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t bt = wave % NBT, slot = wave / NBT;
    const uint32_t lm = lane & 15u, lg = lane >> 4;

    const uint32_t fw = a.flags[0]; // (epoch << 2) | highest pair class of the table (bf_bform_terms_kernel)
    const uint32_t cls = (fw >> 2) == a.epoch ? (fw & 3u) : DCS_CLASS_FAST_LOW;
    const float fChan = (float)c;
    const float D = a.k.fDenominator, y = a.k.fRcpDenominator;
    // one coefficient through the class's path (slow: IEEE divide + fp64 sincos; rare, workgroup-uniform)
    auto with_generator = [&](auto &&body) {
        if (cls == DCS_CLASS_SLOW) {
            body([&](float kx, float ky, float &re, float &im) { coeff_slow(kx, ky, fChan, D, re, im); });
        } else {
            dispatch_fast(a.k.uDiv3Exact != 0u, cls == DCS_CLASS_FAST_LOW, [&](auto div3, auto lowdeg) {
                body([&](float kx, float ky, float &re, float &im) {
                    coeff_fast<decltype(div3)::value, decltype(lowdeg)::value>(kx, ky, fChan, D, y, re, im);
                });
            });
        }
    };

    // ---- W for (channel c, beams [b0, b0 + 16 NBT), all antennas) into LDS: once per workgroup, a rolled loop
    //      (a lane computing its own 16 fragments unrolled cost 178 registers and 36 000 lines of code);
    //      batches of 8 terms loads in flight together, unconditional on clamped indices and masked afterwards
    //      (a load under an exec mask makes hipcc wait for it on the spot: one memory latency per load)
    {
        float *Wre = lds, *Wim = lds + (size_t)A_pad * WS;
        const uint32_t nb = 16u * NBT;
        with_generator([&](auto gen) {
            constexpr uint32_t kBatch = 8;
            for (uint32_t i0 = threadIdx.x; i0 < A_pad * nb; i0 += kBlock * kBatch) {
                floatx2 kp[kBatch];
#pragma unroll
                for (uint32_t q = 0; q < kBatch; q++) {
                    const uint32_t i = min(i0 + q * kBlock, A_pad * nb - 1u), ant = i / nb, b = b0 + (i - ant * nb);
                    kp[q] = *reinterpret_cast<const floatx2 *>(a.terms + 2u * ((uint64_t)min(ant, a.A - 1u) * a.B + min(b, a.B - 1u)));
                }
#pragma unroll 1
                for (uint32_t q = 0; q < kBatch; q++) {
                    const uint32_t i = i0 + q * kBlock, ant = i / nb, bl = i - ant * nb;
                    floatx2 t = kp[0];
#pragma unroll
                    for (uint32_t z = 1; z < kBatch; z++) t = (z == q) ? kp[z] : t; // kp[q] without indexing registers
                    float re, im;
                    gen(t.x, t.y, re, im);
                    if (i < A_pad * nb) {
                        const bool live = ant < a.A && b0 + bl < a.B;
                        Wre[ant * WS + bl] = live ? re : 0.0f;
                        Wim[ant * WS + bl] = live ? im : 0.0f;
                    }
                }
            }
        });
        __syncthreads(); // the only barrier of the kernel
    }
    // A "stage" of this wave = (one of its 16-sample blocks, chunk of kKC antennas), block-major.  The (re, im)
    // int8 pairs of stage s + 1 are requested one stage ahead.  Whole chunks (64 antennas) take a path without any
    // per-operand mask or clamp: the vector ALU issues at most ~12 instructions per MFMA on a SIMD, across all its
    // waves, and a version that masked every operand (3-4 VALU instructions each) ran at 45-55 % of the matrix rate
    // with or without its loads and stores.
    const uint32_t n_chunks = (a.A + kKC - 1u) / kKC;
    const uint32_t n_blocks = tt1 > tt0 + slot ? (tt1 - tt0 - slot + TPR - 1u) / TPR : 0u; // this wave's sample blocks
    const uint32_t n_stages = n_blocks * n_chunks;
    const uint16_t *ant16 = reinterpret_cast<const uint16_t *>(a.ant);
    uint32_t cur[NJ], nxt[NJ];
    auto fetch = [&](uint32_t s, uint32_t (&dst)[NJ]) {
        const uint32_t tt = tt0 + (s / n_chunks) * TPR + slot, a0 = (s % n_chunks) * kKC; // tt < tt1 by construction
        const uint16_t *p0 = ant16 + ((uint64_t)c * a.nT16 + tt) * a.A * 16u + lm; // [c][tt][antenna 0][sample] of (re, im)
        if (a0 + kKC <= a.A) { // wave-uniform
            const uint16_t *p = p0 + (size_t)(a0 + lg) * 16u;
#pragma unroll
            for (uint32_t j = 0; j < NJ; j++) dst[j] = p[(size_t)j * 64u]; // one base address, immediate offsets
        } else {
            // the last, partial chunk: raw, from a clamped (always valid) antenna index, masked where it is consumed.
            // (A select(cond, load, 0) here becomes a load under an exec mask that hipcc waits for on the spot.)
#pragma unroll
            for (uint32_t j = 0; j < NJ; j++) dst[j] = p0[(size_t)min(a0 + lg + 4u * j, a.A - 1u) * 16u];
        }
    };
    floatx4 acc_re = {0.0f, 0.0f, 0.0f, 0.0f}, acc_im = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n_stages) fetch(0, cur);
    for (uint32_t s = 0; s < n_stages; s++) {
        const uint32_t blk = s / n_chunks, chunk = s - blk * n_chunks, a0 = chunk * kKC;
        if (s + 1 < n_stages) fetch(s + 1, nxt);
        // ---- k-steps of 4 antennas: two fma chains (re, im) in antenna order
        const float *wr = lds + (size_t)(a0 + lg) * WS + bt * 16u + lm;
        const float *wi = wr + (size_t)A_pad * WS;
        if (a0 + kKC <= a.A) {
#pragma unroll
            for (uint32_t j = 0; j < NJ; j++) {
                acc_re = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[(size_t)j * 4u * WS], (float)(int8_t)(cur[j] & 0xffu), acc_re, 0, 0, 0);
                acc_im = __builtin_amdgcn_mfma_f32_16x16x4f32(wi[(size_t)j * 4u * WS], (float)(int8_t)(cur[j] >> 8), acc_im, 0, 0, 0);
            }
        } else { // antennas past A: W = 0 (rows up to A_pad) and S masked to 0
            const uint32_t nj = (a.A - a0 + 3u) >> 2;
            for (uint32_t j = 0; j < nj; j++) {
                uint32_t v = cur[0];
#pragma unroll
                for (uint32_t z = 1; z < NJ; z++) v = (z == j) ? cur[z] : v; // cur[j] without indexing registers
                v &= 0u - (uint32_t)(a0 + lg + 4u * j < a.A);
                acc_re = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[(size_t)j * 4u * WS], (float)(int8_t)(v & 0xffu), acc_re, 0, 0, 0);
                acc_im = __builtin_amdgcn_mfma_f32_16x16x4f32(wi[(size_t)j * 4u * WS], (float)(int8_t)(v >> 8), acc_im, 0, 0, 0);
            }
        }
        if (chunk + 1 == n_chunks) { // the block's last chunk: store, start the next block's sums
            // lane l, register r: beam b0 + 16 bt + 4 (l >> 4) + r, sample l & 15
            floatx2 *dst = reinterpret_cast<floatx2 *>(a.beams) + ((uint64_t)c * a.nT16 + tt0 + blk * TPR + slot) * a.B * 16u + lm;
            const uint32_t bb = b0 + bt * 16u + lg * 4u;
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (bb + r < a.B) dst[(uint64_t)(bb + r) * 16u] = floatx2{acc_re[r], acc_im[r]};
            acc_re = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
            acc_im = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (uint32_t j = 0; j < NJ; j++) cur[j] = nxt[j];
    }
}


// ---------------------------------------------------------------------------------------------------------------
// The same contraction on the int8 matrix pipe (v_mfma_i32_16x16x64_i8, 32x the fp32 pipe's rate), EXACTLY:
// the samples ARE int8, and a coefficient w in [-1, 1] is taken as the 24-bit fixed-point number
//   F = rint(w * 8355711) = d1 * 65536 + d2 * 256 + d3,   d1, d2, d3 in [-128, 127]   (8355711 = 0x7F7F7F),
// so that  sum_a w_a x_a  ~=  (65536 * sum d1 x  +  256 * sum d2 x  +  sum d3 x) / 8355711:  three integer
// contractions per plane and 64 antennas whose sums are exact (|sum| <= 128 * 128 * 64 = 2^20) -- no rounding
// depends on the order of the antennas; the two low sums are combined in integers, and that and the high sum (and
// the chunks of more than 64 antennas) are scaled by exact powers of two and added in fp32.  What differs from the
// verifier's fp32 "sum += coeff * sample" is the quantisation of each coefficient (|F / 8355711 - w| <=
// 0.75 / 8355711 = 9e-8: the size of the fp32 coefficient's own last place) and the verifier's OWN accumulation
// roundings; against an exact-arithmetic sum of the fp32 coefficients the result is within 9e-8 * sum_a |x_a| +
// 1.8e-7 * |sum| (three roundings of 2^-24 relative each -- the low part's conversion apart, which is far below:
// tests/test_beamformer_model.py derives it term by term; tests/test_gpu_beamformer_exact.py holds the kernels to
// this arithmetic bit for bit, tests/test_gpu_parity.py to a bound over the oracle's coefficients).
//
// A wave owns one 16-beam tile of one channel and some of the workgroup's 16-sample blocks.  Its coefficients
// (64 antennas = 6 operands of 4 registers: 3 digits x {re, im}) are made once, in registers (waves that own the
// same tile make a share each and exchange them through LDS).  Up to 64 antennas the workgroup's sample blocks
// (at most 16 = 32 KiB) travel to LDS by LDS-DMA while the coefficients are being made; beyond (kChain, round 3), the
// workgroup's waves make the coefficients of 64 antennas each, put them in LDS, and every wave walks all the antenna
// chunks of its own sample blocks with the matrix instruction's accumulator.  Per pair of blocks and 64 antennas: 16 four-byte operand reads per
// lane, a 4 x 4 byte transpose into four K = 64 operands (slot (lane >> 4, byte p) of BOTH operands is antenna
// 64 ch + 4 p + (lane >> 4): the contraction index may be permuted freely as long as both sides agree), 12 MFMAs,
// ~130 vector instructions to recombine, 4 sixteen-byte stores.  The arithmetic is hidden entirely: with its stores
// alone, no loads and no coefficients, the kernel is as fast (profiles/r02_fused.md).
typedef int intx4 __attribute__((ext_vector_type(4)));
constexpr float kFixScale = 8355711.0f;

// The three signed digits of rint(w * 8355711), one per byte (byte 0 = d3 ... byte 2 = d1; byte 3 unused): with every
// digit biased by 128 the number F + 0x808080 is a plain 24-bit unsigned whose bytes are d + 128, and (d + 128) ^ 0x80
// is d as a signed byte -- no borrows to chase.
__device__ __forceinline__ uint32_t fixed_word(float w)
{
    // a coefficient one ulp above 1 must not carry into a fourth digit
    const float f = __builtin_amdgcn_fmed3f(w * kFixScale, -kFixScale, kFixScale);
    return ((uint32_t)(int)rintf(f) + 0x808080u) ^ 0x808080u;
}

// Three forms of one kernel (FORM):
//   kStaged (nr_stations <= 64): the workgroup's sample blocks (at most 16: 32 KiB) travel to LDS by LDS-DMA, all at
//       once and while the coefficients are being made, and the waves read their operands from there -- every wave of
//       the workgroup needs the same blocks when it owns several beam tiles, and no wave ever waits for a global load
//       inside its loop (a wave that loads its own operands pays one memory latency per trip; with loads and stores
//       but no arithmetic that form ran exactly as fast as with the arithmetic).  Wave w: beam tile w % nbt, blocks
//       w / nbt, w / nbt + 4 / nbt, ...
//   kDirect (nr_stations <= 64; probes and A/B only): the same, every wave loading its own operands.
//   kSplit  (64 < nr_stations <= 256): the CONTRACTION INDEX is split over the waves -- wave w holds the coefficients
//       of antennas [64 w, 64 w + 64) of the workgroup's ONE beam tile (24 registers, as in the other forms, instead of
//       96 in one wave), loads that chunk's operands itself, and the four partial sums of a pair of blocks meet in
//       LDS: each wave adds up, scales and stores the four beams of one result register (wave w: beams w, w + 4 ... of
//       the tile).  Two barriers per trip of two pairs.
//   kChain  (64 < nr_stations <= 256; the product's form there since round 3): the workgroup owns ONE beam tile and its
//       coefficients -- wave w makes those of antennas [64 w, 64 w + 64), as in kSplit -- go to LDS (4 chunks x 6 operands x
//       1 KiB = 24 KiB), from where EVERY wave reads them (one ds_read_b128 per operand and chunk).  Wave w then takes the
//       sample blocks w, w + 4, ... by itself and walks ALL the antenna chunks of a pair of blocks with the matrix
//       instruction's own accumulator: the twelve integer sums (3 digits x 4 planes) run through the chunks in int32,
//       exactly (|sum| <= 128 * 128 * 256 = 2^22), and are recombined ONCE per pair.  Against kSplit: no partial sums in
//       LDS, no barrier inside the loop (kSplit: two per trip, every wave waiting for the slowest), a quarter of the
//       recombination arithmetic, and a result that is one fp32 rounding closer to the exact sum.
// FULL: nr_stations is a multiple of 64 (no antenna masks, immediate load offsets).
enum { kStaged = 0, kDirect = 1, kSplit = 2, kChain = 3 };
// kChain is allocated for 4 waves per SIMD (127 VGPRs, no scratch: the coefficient digits go straight to LDS as they are made,
// and the results are recombined and stored one register at a time) and walks with TWO sample buffers.  It measures the same at 3
// waves (the kernel is issue-bound: profiles/r03_fused.md); tried and not kept: a third sample buffer (168 registers, 2 spills), the
// next step's loads issued before this step's wait (1-4 % slower).
constexpr int kChainWaves = 4;

// NW: waves per workgroup -- 4; 8 (kStaged, eight beam tiles per workgroup) is instantiated in the probes build only: an A/B
// that measured no gain over four tiles (profiles/r03_fused.md)
// quant: the quantised kChain kernels take 3 -- their epilogue (four packed results held for the quad transpose, the gains, the
// clip counts) wants 144 registers and spills 16 of them at 128, and scratch is not an option (the first launch of a
// process would pay for it); kChain measured the same at 3 waves as at 4
// wide: the weighted complex product's kernels with antenna masks (include/dcs_beam_complex.h; nine coefficient operands, the
// weights' loads and the masks together) take 3 as well, kStaged too: at 128 registers kStaged spilled 2 and kChain 6
// the quantised complex product (include/dcs_beam_complex_quant.h) falls under the same two rules, and they give each of its eight
// kernels the most waves it takes without spilling (DESIGN.md section 5.14 has the table): kStaged 4 (126 - 128 registers) but for the
// weighted one with antenna masks (8 spilled at 128; 138 at 3), kChain 3 (144; 16 - 20 spilled at 128)
constexpr int i8_waves_per_eu(int form, bool full, bool quant = false, bool wide = false)
{
    return form == kSplit ? (full ? 3 : 2)
                          : (form == kChain ? kChainWaves - (quant || wide ? 1 : 0) : (wide ? 3 : (full || form == kStaged ? 4 : 3)));
}

// ---- the quantised epilogue (include/dcs_beam_quant.h): what bf_beamform_i8_kernel's QUANT
// instantiations do with a result register instead of storing its four floats.
// o = {re even, im even, re odd, im odd} of one beam and one pair of samples, exactly the floats the unquantised kernel
// stores; k the beam's gain.  Per component y = RN(o * k) (one multiply of its own), NaN -> -128, otherwise
// clamp(rint(y), -127, 127); the four bytes are, in this order, four consecutive bytes of the int8 tensor.  Counting
// (count: wave-uniform; live: this lane's register is stored at all) costs a compare per component and one wave-uniform
// branch: the lanes' counts of register r pile up in byte r of n_clip -- at most 4 per pair of blocks, and the launcher
// gives a wave fewer than 64 pairs.
__device__ __forceinline__ uint32_t q8_pack(const floatx4 o, float k, bool count, bool live, int r, uint32_t &n_clip)
{
    uint32_t word = 0u, n = 0u;
    bool any = false;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const float y = o[v] * k;
        const float ry = rintf(y);
        const bool clip = !(fabsf(ry) <= 127.0f); // NaN included
        const float q = y != y ? -128.0f : __builtin_amdgcn_fmed3f(ry, -127.0f, 127.0f);
        word |= ((uint32_t)(int)q & 0xffu) << (8 * v);
        any |= clip;
        n += clip ? 1u : 0u;
    }
    if (count && __builtin_amdgcn_ballot_w64(any && live) != 0ull) n_clip += live ? n << (8 * r) : 0u;
    return word;
}

// 4 x 4 dword transpose inside every quad of lanes (lanes 4 j .. 4 j + 3), on the DPP quad permutes -- no LDS: afterwards
// register j of lane i is what register i of lane j was.  Two exchanges of 2 x 2 blocks (lane ^ 1, then lane ^ 2); every
// lane of the wave must be active.
__device__ __forceinline__ void q8_quad_transpose(uint32_t (&d)[4], uint32_t lane)
{
    const bool b0 = (lane & 1u) != 0u, b1 = (lane & 2u) != 0u;
#pragma unroll
    for (int p = 0; p < 4; p += 2) { // registers (p, p + 1) with lane ^ 1: quad_perm [1, 0, 3, 2]
        const uint32_t recv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(b0 ? d[p] : d[p + 1]), 0xB1, 0xf, 0xf, false);
        d[p] = b0 ? recv : d[p];
        d[p + 1] = b0 ? d[p + 1] : recv;
    }
#pragma unroll
    for (int p = 0; p < 2; p++) { // registers (p, p + 2) with lane ^ 2: quad_perm [2, 3, 0, 1]
        const uint32_t recv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(b1 ? d[p] : d[p + 2]), 0x4E, 0xf, 0xf, false);
        d[p] = b1 ? recv : d[p];
        d[p + 2] = b1 ? d[p + 2] : recv;
    }
}

// The wave's clip counts to the caller's counters: n_clip's byte r is this lane's count for beam bb + 4 r, and the sixteen
// lanes of a row (same lane >> 4) hold the same four beams.  Only a wave that clipped gets past the first line; it adds
// up each row and issues at most sixteen atomics.
__device__ __forceinline__ void q8_tally(unsigned long long *clips, uint32_t n_clip, uint32_t bb, uint32_t lm, uint32_t B)
{
    if (__builtin_amdgcn_ballot_w64(n_clip != 0u) == 0ull) return;
    uint32_t even = n_clip & 0x00ff00ffu, odd = (n_clip >> 8) & 0x00ff00ffu; // registers (0, 2) and (1, 3) in 16-bit fields: <= 16 x 255
    for (int s = 1; s < 16; s <<= 1) even += (uint32_t)__shfl_xor((int)even, s), odd += (uint32_t)__shfl_xor((int)odd, s);
    if (lm < 4u) { // lane lm of the row: register r = lm
        const uint32_t n = (((lm & 1u) ? odd : even) >> (16u * (lm >> 1))) & 0xffffu, beam = bb + 4u * lm;
        if (n != 0u && beam < B) atomicAdd(clips + beam, (unsigned long long)n);
    }
}

// ---- the detecting epilogue (include/dcs_beam_power.h): what bf_beamform_i8_kernel's POWER
// instantiations do with a result register instead of storing its four floats.
// o = {re even, im even, re odd, im odd} of one beam and samples 2 m, 2 m + 1 (m = lane & 7), exactly the floats the float
// kernel stores.  p_t = RN(RN(re re) + RN(im im)) per sample (no fma: -ffp-contract=off), level 1 of the block's pairwise sum
// in the lane, levels 2 - 4 with lane ^ 1, lane ^ 2 (the DPP quad permutes of q8_quad_transpose) and the other quad of the
// 8-lane group (row_half_mirror: lane 7 - i of the group, whose quad holds one value by then).  fp32 addition commutes, so
// all 8 lanes end with the same bits; every lane of the wave must be active.
__device__ __forceinline__ float power_block_sum(const floatx4 o)
{
    const float p_even = o[0] * o[0] + o[1] * o[1], p_odd = o[2] * o[2] + o[3] * o[3];
    float s = p_even + p_odd;
    s = s + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0xB1, 0xf, 0xf, false));  // quad_perm [1, 0, 3, 2]
    s = s + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x4E, 0xf, 0xf, false));  // quad_perm [2, 3, 0, 1]
    s = s + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), 0x141, 0xf, 0xf, false)); // row_half_mirror
    return s;
}

#include "bf_beamform_i8_kernel.inc"

} // namespace

// LDS bytes of one workgroup for NBT beam tiles and A antennas.
static size_t bacc_lds_bytes(int nbt, uint32_t A)
{
    const uint32_t A_pad = (A + 3u) & ~3u;
    const uint32_t ws = 16u * (uint32_t)nbt + (nbt > 1 ? 16u : 0u);
    return (size_t)A_pad * ws * 2u * sizeof(float);
}

// This translation unit is a code object of its own: load it when the context is created, not in the first (timed) call.
hipError_t bf_warm_module_mfma()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_beamform_i8_kernel<kStaged, true>));
}

namespace {
// f(one std::bool_constant per flag): the runtime flags as template arguments
template <class F>
void dispatch_flags(F f)
{
    f();
}
template <class F, class... Rest>
void dispatch_flags(F f, bool flag, Rest... rest)
{
    if (flag)
        dispatch_flags([&](auto... t) { f(std::true_type{}, t...); }, rest...);
    else
        dispatch_flags([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

// a kernel parameter that exists only where its switch is on
template <bool ON, class T>
auto i8_arg(const T *p)
{
    if constexpr (ON)
        return std::tuple<T>(*p);
    else
        return std::tuple<>();
}

// One launch for every instantiation of bf_beamform_i8_kernel.  w, q, power, cx: nullptr / false = not asked for; the switches
// exist for the product's forms (kStaged, kChain; four waves) only, every other instantiation is the plain kernel's.
template <int FORM, bool FULL, int NW>
void launch_i8(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const bf_bacc_args &a, const bf_weights_args *w,
               const bf_quant_args *q, bool power, const bf_complex_args *cx)
{
    if constexpr (NW == 4 && (FORM == kStaged || FORM == kChain)) {
        dispatch_flags([&](auto weighted, auto quant, auto detect, auto complex) {
            constexpr bool W = decltype(weighted)::value, Q = decltype(quant)::value, P = decltype(detect)::value, C = decltype(complex)::value;
            if constexpr (!(Q && P)) // (the launcher has refused that)
                std::apply([&](const auto &...extra) {
                    hipLaunchKernelGGL((bf_beamform_i8_kernel<FORM, FULL, NW, W, Q, P, C, std::decay_t<decltype(extra)>...>), grid, block, lds,
                                       stream, a, extra...);
                }, std::tuple_cat(i8_arg<W>(w), i8_arg<Q>(q), i8_arg<C>(cx)));
        }, w != nullptr, q != nullptr, power, cx != nullptr);
    } else {
        hipLaunchKernelGGL((bf_beamform_i8_kernel<FORM, FULL, NW>), grid, block, lds, stream, a);
    }
}

template <int FORM, int NW = 4>
void launch_i8_form(bool full, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const bf_bacc_args &a,
                    const bf_weights_args *w, const bf_quant_args *q, bool power, const bf_complex_args *cx)
{
    if (full)
        launch_i8<FORM, true, NW>(grid, block, lds, stream, a, w, q, power, cx);
    else
        launch_i8<FORM, false, NW>(grid, block, lds, stream, a, w, q, power, cx);
}
} // namespace

hipError_t bf_launch_beamform_acc(const bf_bacc_args &a_in, const bf_weights_args *w, const bf_quant_args *q, bool power,
                                  const bf_complex_args *cx, hipStream_t stream)
{
    bf_bacc_args a = a_in;
    if (a.A == 0 || a.B == 0 || a.C == 0 || a.nT16 == 0) return hipSuccess;
    if (a.A > 256u) return hipErrorInvalidValue; // not built
    const bool chain = a.fp32_chain != 0u;
    if ((w || q || power || cx) && chain) return hipErrorInvalidValue;
    if (q && power) return hipErrorInvalidValue;
    // beam tiles per workgroup: as many as the beams need; the fp32 form keeps its coefficient planes in LDS and
    // takes as many as still admit 6 workgroups per CU (26 KiB each), one tile whatever it takes beyond
    // more than 64 antennas, int8 form: one beam tile per workgroup; kChain (the product's form) or, probes build only, kSplit
    const bool wide = !chain && a.A > 64u;
    const bool split = wide && BACC_KNOB(a, unstaged) != 0u; // kSplit (round 2): every wave takes every block, partial sums meet in LDS
    const bool staged_form = !chain && a.A <= 64u && !BACC_KNOB(a, unstaged); // at most 16 blocks (32 KiB of LDS) per workgroup
    int nbt = wide ? 1 : (a.B > 32u ? 4 : (a.B > 16u ? 2 : 1));
#ifdef DCS_PROBES
    // A/B: beam tiles per workgroup.  1 / 2 / 4 / 8 (eight-wave workgroups) at 64 x 256 x 4096 x 256: 552 / 502 / 396 / 399 us --
    // four is where the samples' re-staging stops mattering (profiles/r03_fused.md); eight exists in the probes build only
    if (staged_form && (a.nbt_force == 1u || a.nbt_force == 2u || a.nbt_force == 4u || a.nbt_force == 8u)) nbt = (int)a.nbt_force;
#endif
    uint32_t nw = nbt == 8 ? 8u : 4u; // waves per workgroup
#ifdef DCS_PROBES
    if (staged_form && (a.nw_force == 8u || a.nw_force == 16u) && a.nw_force >= (uint32_t)nbt) nw = a.nw_force; // A/B: waves per workgroup
#endif
    while (chain && nbt > 1 && bacc_lds_bytes(nbt, a.A) > 26u * 1024u) nbt >>= 1;
    const size_t lds = chain ? bacc_lds_bytes(nbt, a.A) : 0u;
    a.nbt_log2 = nbt == 8 ? 3u : (nbt == 4 ? 2u : (nbt == 2 ? 1u : 0u));
    a.n_bgroups = (a.B + 16u * (uint32_t)nbt - 1u) / (16u * (uint32_t)nbt);
    // 16-sample blocks per workgroup: whole rounds of 4 / nbt blocks, at most max_rounds (the coefficients are
    // generated once per workgroup; but a launch of only a few thousand long-lived workgroups ends with most of the
    // chip idle behind the last ones), fewer while that leaves the chip under 4096 workgroups
    const uint32_t tpr = split ? 1u : nw / (uint32_t)nbt; // (K-split: every wave takes every block)
    // (64 beams exactly fill one four-tile workgroup per channel: there EIGHT blocks per workgroup measured 3-5 % faster than
    // sixteen on four shapes, while from 128 beams on eight or twelve blocks cost 3-7 %: profiles/r03_fused.md)
    const uint32_t blocks_cap = staged_form && nbt == 4 && a.n_bgroups == 1u ? 8u : 16u;
    const uint32_t max_rounds = BACC_KNOB(a, max_rounds) ? BACC_KNOB(a, max_rounds) : (chain ? 16u : (staged_form || wide ? blocks_cap / tpr : 32u));
    uint32_t tiles = (a.nT16 + tpr - 1u) / tpr * tpr;
    if (tiles > max_rounds * tpr) { // several workgroups per (channel, beam group): equal shares (17 blocks are 9 + 8, not 16 + 1)
        const uint32_t parts = (a.nT16 + max_rounds * tpr - 1u) / (max_rounds * tpr);
        tiles = ((a.nT16 + parts - 1u) / parts + tpr - 1u) / tpr * tpr;
    }
    // (the int8 form makes its coefficients once per wave -- half its arithmetic at 16 blocks -- so it only splits
    // further while the chip, which holds 1280 of its workgroups, would not even be filled once)
    const uint64_t enough = chain ? 4096u : 5120u / nw;
    while (tiles > tpr && (uint64_t)a.C * a.n_bgroups * ((a.nT16 + tiles - 1u) / tiles) < enough) tiles = ((tiles / tpr + 1u) / 2u) * tpr;
    a.tiles_per_wg = tiles;
    a.n_tgroups = (a.nT16 + tiles - 1u) / tiles;
    // the workgroups that share a channel's samples on one XCD? (xcd_grouped above; measured)
    a.xcd_group = wide ? a.n_bgroups : (!chain && a.n_bgroups >= 16u ? a.n_bgroups : 1u);
    const uint64_t blocks = (uint64_t)a.C * a.n_bgroups * a.n_tgroups;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks), block(64u * nw);
    if (chain) {
        if (nbt == 4)
            hipLaunchKernelGGL(bf_beamform_acc_kernel<4>, grid, block, lds, stream, a);
        else if (nbt == 2)
            hipLaunchKernelGGL(bf_beamform_acc_kernel<2>, grid, block, lds, stream, a);
        else
            hipLaunchKernelGGL(bf_beamform_acc_kernel<1>, grid, block, lds, stream, a);
        return hipGetLastError();
    }
    const bool plain = !w && !q && !power && !cx;
    if (!plain && (nw != 4u || (!staged_form && (!wide || split)))) return hipErrorInvalidValue; // the product's forms only
    if (q && a.tiles_per_wg / tpr > 126u) return hipErrorInvalidValue; // a lane counts its clips in bytes, 4 per pair of blocks
    const bool full = a.A % 64u == 0u; // (kStaged, kDirect: 64 antennas exactly)
    if (staged_form) {
        size_t stage_bytes = ((size_t)a.tiles_per_wg * a.A * 32u + 1023u) / 1024u * 1024u;
        if (tpr > 1u && !BACC_KNOB(a, no_share)) { // waves that own the same tile share the making of its coefficients
            a.share_off = (uint32_t)stage_bytes;
            stage_bytes += (size_t)nbt * 4u * (cx ? 9u : 6u) * 64u * sizeof(uint32_t); // the complex product: nine operands
        }
#ifdef DCS_PROBES
        if (plain && a.wg_per_cu >= 1u && a.wg_per_cu <= 5u && stage_bytes < 160u * 1024u / a.wg_per_cu) // residency cap: unused LDS
            stage_bytes = (160u * 1024u / a.wg_per_cu) & ~1023u;
        if (nw == 8u)
            launch_i8_form<kStaged, 8>(full, grid, block, stage_bytes, stream, a, w, q, power, cx);
        else if (nw == 16u)
            launch_i8_form<kStaged, 16>(full, grid, block, stage_bytes, stream, a, w, q, power, cx);
        else
#endif
        launch_i8_form<kStaged>(full, grid, block, stage_bytes, stream, a, w, q, power, cx);
#ifdef DCS_PROBES
    } else if (a.A <= 64u) { // kDirect: the probes build's A/B form only
        launch_i8_form<kDirect>(full, grid, block, 0, stream, a, w, q, power, cx);
    } else if (split) { // 2 pairs x 4 registers x 4 chunks x 64 lanes x 16 bytes of partial sums
        launch_i8_form<kSplit>(full, grid, block, 2u * 4u * 4u * 64u * 16u, stream, a, w, q, power, cx);
#endif
    } else { // kChain: 4 chunks x 6 operands x 64 lanes x 16 bytes of coefficients + the chunks' NaN-row words, then the 16
             // beams' scale factors (weighted) and behind them their 16 gains (quantised, weighted or not)
             // (the complex product: 9 operands, 36 KiB)
        const size_t coef_bytes = 4u * (cx ? 9u : 6u) * 64u * 16u + 8u * sizeof(uint32_t) + (q ? 32u : (w ? 16u : 0u)) * sizeof(float);
        launch_i8_form<kChain>(full, grid, block, coef_bytes, stream, a, w, q, power, cx);
    }
    return hipGetLastError();
}
