// bf_ddc.hip -- the narrowband digital down-converter on the matrix cores (include/dcs_ddc.h), gfx950
// only: real int8 [nr_inputs][in_stride] mixed with an oscillator, filtered by T <= 256 taps and decimated by 16 into
// float [band][input][out_stride][{re, im}].  The mixer is folded into the filter, so the filter is an exact integer
// contraction of fixed complex taps g with the raw bytes, S[m] = sum_j g[j] x[16 m + j], and the oscillator one rotation per
// output by a 32-bit phase word.
//
// The contraction is v_mfma_i32_16x16x64_i8 with the taps as the row operand and the samples as the column operand:
//
//  * the 16 rows are 4 quantities {band 0 re, band 0 im, band 1 re, band 1 im} x (the three balanced base-256 digits of the
//    tap + one zero row): row = 4 quantity + digit.  Register r of lane (lm = lane & 15, lg = lane >> 4) of the result is row
//    4 lg + r, column lm: a lane's four accumulator registers are the three digit sums of quantity lg of output lm (and a
//    zero), which it combines as s0 + (s1 << 8) + (s2 << 16) without any other lane;
//  * with decimation 16 the Hankel operand costs no data movement.  A lane's K slice is 16 consecutive bytes; for output
//    column lm of the tile at output m0 and K step s, lane group lg takes taps 16 (4 s + lg) .. + 15, which multiply the ALIGNED
//    16-byte chunk m0 + lm + 4 s + lg of the row: one ds_read_b128 from the staged span.  Both operands take a lane's byte k
//    of group lg for the same K index, whatever the hardware's order of K;
//  * the tap operand, the table of bf_ddc_tap_digits_kernel, is [K step][lane][16 bytes]: T / 64 b128 loads per lane, made once
//    per wave and kept (16 registers at T = 256).
//
// A workgroup of kWaves waves stages the chunks of a span of kSpanOut outputs of one row in LDS -- kSpanOut + T / 16 - 1 of
// them, b128 loads, zero where the row is not to be read: past chunk nr_out + T / 16 - 2 -- and its waves take runs of
// kTilesPerWave tiles of 16 outputs, two tiles at a time.  One exchange with the lane 16 away (the other component of the
// band) gives the lanes of the re rows (S_re, S_im) of the first tile of the pair and those of the im rows that of the second,
// so every lane of a band that exists finishes one output: F = (float)S, the oscillator's (c, s) by dcs_sincos_turn32, the
// rotation and the gain, each a single fp32 operation (-ffp-contract=off), and ONE dwordx2 store: the 16 lanes of a group write
// 128 contiguous bytes.  Every word is written once, by a plain store.  Byte offsets are 64-bit.

#include "bf_host.h"
#include "bf_math.h"

#include <hip/hip_runtime.h>

// The digital down-converter (include/dcs_ddc.h): real int8 [nr_inputs][in_stride] ->
// float [band][input][out_stride][{re, im}], nr_out outputs per row, output m from samples 16 m .. 16 m + T - 1
struct bf_ddc_digits_args {
    const int32_t *taps; // [band][T][{re, im}]
    int8_t *digits;      // 16 T bytes, 16-byte aligned
    uint32_t T;          // 64, 128, 192, 256
    uint32_t nr_bands;   // 1, 2
};
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

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kWaves = 4;                                     // waves per workgroup
constexpr uint32_t kTilesPerWave = 8;                              // tiles of 16 outputs a wave takes, in pairs
constexpr uint32_t kSpanOut = kWaves * kTilesPerWave * 16u;        // outputs per workgroup: 512
constexpr uint32_t kMaxSteps = 4;                                  // K steps of 64 taps: T <= 256
constexpr uint32_t kChunks = kSpanOut + 16u * kMaxSteps;           // staged chunks: kSpanOut + 15 are used at most
constexpr uint32_t kGrid = 1u << 20;                               // workgroups at most; they walk the items beyond
static_assert(kTilesPerWave % 2u == 0u, "a wave takes its tiles in pairs");

// The operand table: byte k of lane (lm, lg) of K step s is digit (lm & 3) of component (lm >> 2) & 1 of band lm >> 3 of tap
// 16 (4 s + lg) + k; digit 3 and the bands that do not exist are zero rows.  A thread makes one lane's 16 bytes.
__global__ void __launch_bounds__(64) bf_ddc_tap_digits_kernel(const bf_ddc_digits_args a)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x, lm = lane & 15u, lg = lane >> 4;
    const uint32_t digit = lm & 3u, comp = (lm >> 2) & 1u, band = lm >> 3;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (digit < 3u && band < a.nr_bands) {
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t j = 16u * (4u * s + lg) + k;
            const int32_t v = a.taps[((uint64_t)band * a.T + j) * 2u + comp];
            // balanced digits: d0 the low byte taken as signed, then the same of (v - d0) / 256, and once more (it wraps)
            // (the differences in unsigned arithmetic: v - d0 of a v near 2^31 wraps, which the top digit's wrap absorbs)
            const int32_t d0 = (int32_t)(int8_t)(uint8_t)v, v1 = (int32_t)((uint32_t)v - (uint32_t)d0) >> 8;
            const int32_t d1 = (int32_t)(int8_t)(uint8_t)v1, v2 = (int32_t)((uint32_t)v1 - (uint32_t)d1) >> 8;
            const int32_t d = digit == 0u ? d0 : digit == 1u ? d1 : (int32_t)(int8_t)(uint8_t)v2;
            w[k >> 2] |= ((uint32_t)d & 0xffu) << (8u * (k & 3u));
        }
    }
    reinterpret_cast<intx4 *>(a.digits)[s * 64u + lane] = intx4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
}

__global__ void __launch_bounds__(kWaves * 64) bf_ddc_kernel(const bf_ddc_args a)
{
    __shared__ intx4 span[kChunks];
    const uint32_t lane = threadIdx.x & 63u, lm = lane & 15u, lg = lane >> 4;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t steps = a.T / 64u, halo = a.T / 16u - 1u;
    const uint32_t comp = lg & 1u, band = lg >> 1;

    intx4 tap[kMaxSteps];
#pragma unroll
    for (uint32_t s = 0; s < kMaxSteps; s++)
        tap[s] = s < steps ? reinterpret_cast<const intx4 *>(a.digits)[s * 64u + lane] : intx4{0, 0, 0, 0};
    const uint32_t u0 = band ? a.u0[1] : a.u0[0], step16 = band ? a.step16[1] : a.step16[0];
    const float gain = band ? a.gain[1] : a.gain[0];

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint64_t input = item / a.spans;
        const uint32_t o0 = (uint32_t)(item % a.spans) * kSpanOut; // first output of the span
        const uint32_t n_out = a.nr_out - o0 < kSpanOut ? a.nr_out - o0 : kSpanOut;
        const uint32_t n_chunks = n_out + halo; // the chunks of the span that the row holds: none is read past them
        const intx4 *row = reinterpret_cast<const intx4 *>(a.x + input * a.in_stride) + (uint64_t)o0;
        __syncthreads(); // the previous item's reads of the span are done
        for (uint32_t i = threadIdx.x; i < kChunks; i += kWaves * 64u) span[i] = i < n_chunks ? row[i] : intx4{0, 0, 0, 0};
        __syncthreads();

#pragma unroll 1
        for (uint32_t p = 0; p < kTilesPerWave; p += 2u) {
            const uint32_t tA = wave * kTilesPerWave + p; // tile tA and tile tA + 1
            if (tA * 16u >= n_out) break;                 // wave-uniform
            intx4 accA = {0, 0, 0, 0}, accB = {0, 0, 0, 0};
            const uint32_t c0 = tA * 16u + lm + lg; // < kSpanOut + 18; + 4 s + 16 < kChunks
#pragma unroll
            for (uint32_t s = 0; s < kMaxSteps; s++) {
                if (s < steps) {
                    accA = __builtin_amdgcn_mfma_i32_16x16x64_i8(tap[s], span[c0 + 4u * s], accA, 0, 0, 0);
                    accB = __builtin_amdgcn_mfma_i32_16x16x64_i8(tap[s], span[c0 + 16u + 4u * s], accB, 0, 0, 0);
                }
            }
            // the word of this lane's quantity in both tiles, modulo 2^32
            const uint32_t SA = (uint32_t)accA[0] + ((uint32_t)accA[1] << 8) + ((uint32_t)accA[2] << 16);
            const uint32_t SB = (uint32_t)accB[0] + ((uint32_t)accB[1] << 8) + ((uint32_t)accB[2] << 16);
            // re lanes finish tile A, im lanes tile B: each sends the other its word of the tile that the other finishes
            const uint32_t mine = comp ? SB : SA;
            const uint32_t theirs = (uint32_t)__shfl_xor((int)(comp ? SA : SB), 16, 64);
            const float Fre = (float)(int32_t)(comp ? theirs : mine), Fim = (float)(int32_t)(comp ? mine : theirs);
            const uint32_t ml = (tA + comp) * 16u + lm; // output of the span
            if (band < a.nr_bands && ml < n_out) {
                const uint32_t m = o0 + ml;
                float sn, cs;
                dcs_sincos_turn32(u0 + m * step16, &sn, &cs);
                const float re = (Fre * cs + Fim * sn) * gain;
                const float im = (Fim * cs - Fre * sn) * gain;
                float *out = a.out + (((uint64_t)band * a.nr_inputs + input) * a.out_stride + m) * 2u;
                *reinterpret_cast<floatx2 *>(out) = floatx2{re, im};
            }
        }
    }
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_ddc()
{
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_ddc_tap_digits_kernel));
    if (e != hipSuccess) return e;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_ddc_kernel));
}

static hipError_t bf_launch_ddc_tap_digits(const bf_ddc_digits_args &a, hipStream_t stream)
{
    if (a.T % 64u != 0u || a.T < 64u || a.T > 64u * kMaxSteps || a.nr_bands < 1u || a.nr_bands > 2u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_ddc_tap_digits_kernel, dim3(a.T / 64u), dim3(64), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_ddc(const bf_ddc_args &args, hipStream_t stream)
{
    if (args.nr_out == 0u || args.nr_inputs == 0u) return hipSuccess;
    if (args.T % 64u != 0u || args.T < 64u || args.T > 64u * kMaxSteps || args.nr_bands < 1u || args.nr_bands > 2u)
        return hipErrorInvalidValue;
    bf_ddc_args a = args;
    a.spans = (uint32_t)(((uint64_t)a.nr_out + kSpanOut - 1u) / kSpanOut);
    a.items = (uint64_t)a.nr_inputs * a.spans;
    hipLaunchKernelGGL(bf_ddc_kernel, dim3((uint32_t)(a.items < kGrid ? a.items : kGrid)), dim3(kWaves * 64u), 0, stream, a);
    return hipGetLastError();
}

// The host side of include/dcs_ddc.h, behind the table as in bf_integrate.hip.  Of the context these use the device alone:
// every size is an argument, and the device-free checks are all the checks there are.
namespace bf_host {

int ddc_tap_digits_impl(dcs_bf_context *c, const int32_t *d_taps, uint32_t nr_taps, uint32_t nr_bands, void *d_digits,
                        size_t digits_bytes, void *stream)
{
    if (int e = ddc_tap_digits_args(c, d_taps, nr_taps, nr_bands, d_digits, digits_bytes)) return e;
    DCS_CHECK_DEVICE(c);
    bf_ddc_digits_args a;
    std::memset(&a, 0, sizeof(a));
    a.taps = d_taps;
    a.digits = static_cast<int8_t *>(d_digits);
    a.T = nr_taps;
    a.nr_bands = nr_bands;
    return (int)bf_launch_ddc_tap_digits(a, as_stream(stream));
}

// the oscillator of output m of the call is phase0 + 16 (first_output + m) phase_step mod 2^32: the part that does not depend on
// m is made here, in wrapping 32-bit arithmetic
int ddc_impl(dcs_bf_context *c, uint32_t nr_inputs, uint32_t nr_out, const int8_t *d_samples, size_t samples_bytes, uint64_t in_stride,
             const void *d_digits, size_t digits_bytes, uint32_t nr_taps, uint32_t nr_bands, const dcs_ddc_band *bands,
             uint64_t first_output, float *d_out, size_t out_bytes, uint64_t out_stride, void *stream)
{
    if (int e = ddc_args(c, nr_inputs, nr_out, d_samples, samples_bytes, in_stride, d_digits, digits_bytes, nr_taps, nr_bands, bands,
                         d_out, out_bytes, out_stride))
        return e;
    DCS_CHECK_DEVICE(c);
    if (nr_out == 0u || nr_inputs == 0u) return DCS_OK;
    bf_ddc_args a;
    std::memset(&a, 0, sizeof(a));
    a.x = d_samples;
    a.digits = static_cast<const int8_t *>(d_digits);
    a.out = d_out;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.nr_inputs = nr_inputs;
    a.nr_out = nr_out;
    a.T = nr_taps;
    a.nr_bands = nr_bands;
    for (uint32_t b = 0; b < nr_bands; b++) {
        a.step16[b] = 16u * bands[b].phase_step;
        a.u0[b] = bands[b].phase0 + (uint32_t)first_output * a.step16[b];
        a.gain[b] = bands[b].gain;
    }
    return (int)bf_launch_ddc(a, as_stream(stream));
}

} // namespace bf_host
