// bf_filterbank.hip -- 8-bit search filterbanks (include/dcs_filterbank.h), gfx950 only: running
// sums per (channel, beam) of float spectra [time][channel][beam], the scales {mu, k} from those sums, and the hot path:
// every spectrum normalised, quantised to a byte and transposed into uint8 [beam][time][channel].
//
// The quantiser reads 4 bytes and writes 1 byte per element; its one difficulty is the transposition from beam-fastest
// floats to channel-fastest bytes.  A workgroup of four waves owns a tile of kTileC = 128 channels x kTileB = 32 beams and
// walks a run of time slices:
//
//  * once, in front of the loop, a lane reads the {mu, k} of its 4 channels x 4 beams into registers (the scales have
//    the layout of one time slice);
//  * per slice a lane loads 4 channels x 4 consecutive beams: lane l of the workgroup has beam quad l & 7 and channel
//    quad l >> 3, so eight consecutive lanes read the 128 bytes of a channel's 32 beams.  The fast form loads 16 bytes
//    at a time, the general form dwords, each guarded;
//  * it quantises in registers, one dword of four beams per channel, and transposes the 4 x 4 bytes with four
//    v_perm_b32 so that a dword holds four consecutive channels of one beam;
//  * the four dwords go to an LDS image uint8 [32 beams][128 channels] (4 KiB, two of them in turn so that one barrier
//    per slice is enough), whose 16-byte chunks are XOR-swizzled by the beam quad; the lane then reads back 16 bytes of
//    ONE beam -- lane l has chunk l & 7 of beam l >> 3 -- so eight consecutive lanes store the 128 bytes of a beam's 128
//    channels.  The fast form stores 16 bytes at a time, the general form bytes, each guarded;
//  * the loads of the next slice are issued before the current one is quantised.
//
// LDS banking (ds_write_b32: bank = dword address mod 32, per 32-lane half; ds_read_b128: 16-byte slot = (address / 16)
// mod 16, per the instruction's four 16-lane groups).  A 32-lane half writes beam quads 0 .. 7 of four consecutive channel
// quads q0 .. q0 + 3 (q0 a multiple of 4): row r = 4 bq + i, dword column cq ^ (4 bq), bank (cq & 3) | 4 ((cq >> 2) ^ bq)
// mod 32 -- 32 different banks.  Unswizzled it would be 8-way.  (The compiler pairs the four stores into two ds_write2_b32,
// each half of which is such an access.)  A 16-lane read group {0-3, 12-15, 20-27} holds chunks 0 .. 3 of rows r and
// r + 3 and chunks 4 .. 7 of rows r + 1 and r + 2, r a multiple of 4 (the group {4-11, 16-19, 28-31} the other chunks):
// its slots 8 (row & 1) + (chunk ^ (row >> 2)) are 16 different ones.  Both accesses are conflict-free: 0 extra cycles.
//
// The time axis is gridDim.y: the launcher gives a workgroup at least kMinSlices slices (so that the scales, 8 bytes per
// element, cost at most a quarter of what the slices do) and more once kGrid workgroups are reached.  Clipped elements
// are counted per lane over its whole run and added to the per-beam counters with integer atomics at the end, so the
// counts are exact; a null counter pointer skips that.  Byte offsets are 64-bit.
//
// The sums kernel is bf_integrate_kernel's layout: one lane per (channel, beam), beam fastest, walking time in
// order with eight loads in flight.  The order of the additions is the contract's, so the result cannot depend on the
// launch geometry.  The scales kernel is one lane per (channel, beam) of fp64 arithmetic; -ffp-contract=off keeps every
// operation rounded once.

#include "bf_host.h"

#include <hip/hip_runtime.h>

// 8-bit search filterbanks (include/dcs_filterbank.h).  Spectra are float
// [T][C][B], beam fastest; cb = C * B.
// Running sums {s1, s2} per (channel, beam) over the T spectra, in order, in fp64
struct bf_fbsums_args {
    const float *spectra;
    double *sums;        // [C][B][2]
    uint64_t cb;
    uint32_t T;
    uint32_t accumulate; // non-zero: the sums start from what sums holds
};
// Sums -> scales {mu, k} float [C][B][2], in fp64 rounded once per operation
struct bf_fbscales_args {
    const double *sums;
    float *scales;
    uint64_t cb;
    uint64_t count; // spectra behind the sums: 1 .. 2^53 - 1
    float target_std;
};
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

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kTileC = 128;   // channels of a tile
constexpr uint32_t kTileB = 32;    // beams of a tile
constexpr uint32_t kMinSlices = 8; // slices a workgroup walks at least (where the call has that many)
constexpr uint32_t kGrid = 4096;   // workgroups from which on a workgroup walks more than kMinSlices: 256 CUs x 8 x 2

__global__ void __launch_bounds__(256) bf_spectra_sums_kernel(const bf_fbsums_args a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // c * B + b
    if (g >= a.cb) return;
    double s1 = 0.0, s2 = 0.0;
    if (a.accumulate) {
        s1 = a.sums[2u * g];
        s2 = a.sums[2u * g + 1u];
    }
    const float *p = a.spectra + g;
    uint32_t t = 0;
    for (; t + 8u <= a.T; t += 8u) {
        float x[8];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) x[j] = p[(uint64_t)(t + j) * a.cb];
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            const double d = (double)x[j];
            s1 = s1 + d;
            s2 = s2 + d * d; // the product of two floats is exact in a double
        }
    }
    for (; t < a.T; t++) {
        const double d = (double)p[(uint64_t)t * a.cb];
        s1 = s1 + d;
        s2 = s2 + d * d;
    }
    a.sums[2u * g] = s1;
    a.sums[2u * g + 1u] = s2;
}

__global__ void __launch_bounds__(256) bf_filterbank_scales_kernel(const bf_fbscales_args a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // c * B + b
    if (g >= a.cb) return;
    const double N = (double)a.count; // exact: count < 2^53
    const double m = a.sums[2u * g] / N;
    const double var = a.sums[2u * g + 1u] / N - m * m;
    const double sd = var > 0.0 ? sqrt(var) : 0.0; // a NaN var gives 0
    a.scales[2u * g] = (float)m;
    a.scales[2u * g + 1u] = sd > 0.0 ? (float)((double)a.target_std / sd) : 0.0f;
}

// q = clamp(rint((x - mu) * k + level), 0, 255), each operation rounded once; NaN gives 0.  clipped: NaN or outside 0 .. 255
__device__ __forceinline__ uint32_t quantise(float x, float mu, float k, float level, uint32_t &clipped)
{
    const float d = x - mu;
    const float y = d * k + level; // -ffp-contract=off: no fma
    const float r = rintf(y);
    const bool lo = !(r >= 0.0f); // NaN, or below 0 (-0 is 0)
    const bool hi = r > 255.0f;
    clipped += (lo || hi) ? 1u : 0u;
    return lo ? 0u : hi ? 255u : (uint32_t)r;
}

template <bool FAST> // FAST: B % 4 == 0, C % 16 == 0, spectra 16-byte aligned (the launcher decides)
__global__ void __launch_bounds__(256) bf_filterbank_q8_kernel(const bf_fbq8_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t image[2][kTileB * kTileC / 4u];
    const uint32_t tid = threadIdx.x;
    const uint32_t tiles_b = (a.B + kTileB - 1u) / kTileB;
    const uint32_t c0 = (blockIdx.x / tiles_b) * kTileC, b0 = (blockIdx.x % tiles_b) * kTileB;
    // loading role: channels cl .. cl + 3, beams bl .. bl + 3
    const uint32_t bq = tid & 7u, cq = tid >> 3;
    const uint32_t cl = c0 + cq * 4u, bl = b0 + bq * 4u;
    // storing role: beam bs, channels cs .. cs + 15
    const uint32_t chunk = tid & 7u, row = tid >> 3;
    const uint32_t bs = b0 + row, cs = c0 + chunk * 16u;
    const uint32_t t_begin = blockIdx.y * a.slices; // below T: the launcher makes no empty run
    const uint32_t t_end = a.T - t_begin > a.slices ? t_begin + a.slices : a.T;

    bool ok[4][4]; // [channel j][beam i] inside the tensor; FAST: whole quads are in or out
    float mu[4][4], k[4][4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++)
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            ok[j][i] = FAST ? (cl < a.C && bl < a.B) : (cl + j < a.C && bl + i < a.B);
            mu[j][i] = k[j][i] = 0.0f;
            if (ok[j][i]) {
                const float *s = a.scales + 2u * ((uint64_t)(cl + j) * a.B + bl + i);
                mu[j][i] = s[0];
                k[j][i] = s[1];
            }
        }
    const uint64_t slice = (uint64_t)a.C * a.B; // elements
    uint32_t clips[4] = {0u, 0u, 0u, 0u};       // per beam i

    floatx4 cur[4], nxt[4];
    auto load = [&](floatx4 (&v)[4], uint32_t t) {
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            const float *p = a.spectra + ((uint64_t)t * slice + (uint64_t)(cl + j) * a.B + bl);
            if constexpr (FAST) {
                v[j] = ok[j][0] ? *reinterpret_cast<const floatx4 *>(p) : floatx4{0.0f, 0.0f, 0.0f, 0.0f};
            } else {
                v[j].x = ok[j][0] ? p[0] : 0.0f;
                v[j].y = ok[j][1] ? p[1] : 0.0f;
                v[j].z = ok[j][2] ? p[2] : 0.0f;
                v[j].w = ok[j][3] ? p[3] : 0.0f;
            }
        }
    };
    if (t_begin < t_end) load(cur, t_begin);
    for (uint32_t t = t_begin; t < t_end; t++) {
        if (t + 1u < t_end) load(nxt, t + 1u);
        // quantise: w[j] = the four beams of channel j, beam i in byte i
        uint32_t w[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            uint32_t n[4] = {0u, 0u, 0u, 0u};
            const uint32_t q0 = quantise(cur[j].x, mu[j][0], k[j][0], a.level, n[0]);
            const uint32_t q1 = quantise(cur[j].y, mu[j][1], k[j][1], a.level, n[1]);
            const uint32_t q2 = quantise(cur[j].z, mu[j][2], k[j][2], a.level, n[2]);
            const uint32_t q3 = quantise(cur[j].w, mu[j][3], k[j][3], a.level, n[3]);
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) clips[i] += ok[j][i] ? n[i] : 0u;
            w[j] = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
        }
        // 4 x 4 byte transpose: v[i] = the four channels of beam i, channel j in byte j.  v_perm_b32 selects from the
        // eight bytes {first operand: 7 .. 4, second operand: 3 .. 0}
        const uint32_t lo01 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u); // c0b0 c1b0 c0b1 c1b1
        const uint32_t hi01 = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u); // c0b2 c1b2 c0b3 c1b3
        const uint32_t lo23 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);
        const uint32_t hi23 = __builtin_amdgcn_perm(w[3], w[2], 0x07030602u);
        uint32_t v[4];
        v[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
        v[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
        v[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
        v[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
        uint32_t *img = image[(t - t_begin) & 1u];
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) img[(bq * 4u + i) * (kTileC / 4u) + (cq ^ (bq * 4u))] = v[i];
        __syncthreads();
        uintx4 o = *reinterpret_cast<const uintx4 *>(img + row * (kTileC / 4u) + ((chunk ^ (row >> 2)) * 4u));
        if (bs < a.B && cs < a.C) {
            const uint64_t line = ((uint64_t)bs * a.out_spectra + a.first + t) * a.C; // the output row's first byte
            if constexpr (FAST) {
                if (a.descending) {
                    o = uintx4{__builtin_bswap32(o.w), __builtin_bswap32(o.z), __builtin_bswap32(o.y), __builtin_bswap32(o.x)};
                    *reinterpret_cast<uintx4 *>(a.out + line + (a.C - 16u - cs)) = o;
                } else {
                    *reinterpret_cast<uintx4 *>(a.out + line + cs) = o;
                }
            } else {
                const uint32_t d[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (uint32_t e = 0; e < 16u; e++) {
                    const uint32_t c = cs + e;
                    if (c < a.C) a.out[line + (a.descending ? a.C - 1u - c : c)] = (uint8_t)(d[e >> 2] >> (8u * (e & 3u)));
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) cur[j] = nxt[j];
    }
    if (a.clip_count) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++)
            if (clips[i]) atomicAdd(a.clip_count + bl + i, (unsigned long long)clips[i]);
    }
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_filterbank()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_filterbank_scales_kernel));
}

static hipError_t bf_launch_spectra_sums(const bf_fbsums_args &a, hipStream_t stream)
{
    if (a.T == 0u || a.cb == 0u) return hipSuccess;
    const uint64_t blocks = (a.cb + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_spectra_sums_kernel, dim3((uint32_t)blocks), dim3(256u), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_filterbank_scales(const bf_fbscales_args &a, hipStream_t stream)
{
    if (a.cb == 0u) return hipSuccess;
    const uint64_t blocks = (a.cb + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_filterbank_scales_kernel, dim3((uint32_t)blocks), dim3(256u), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_filterbank_q8(const bf_fbq8_args &args, hipStream_t stream)
{
    bf_fbq8_args a = args;
    if (a.T == 0u || a.C == 0u || a.B == 0u) return hipSuccess;
    const uint64_t tiles = (uint64_t)((a.C + kTileC - 1u) / kTileC) * ((a.B + kTileB - 1u) / kTileB);
    if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
    // slices per workgroup: kMinSlices while that leaves the grid below kGrid workgroups, else what keeps it at kGrid; the
    // second grid dimension holds at most 65535 runs
    uint64_t slices = a.T < kMinSlices ? a.T : kMinSlices;
    const uint64_t full = ((uint64_t)a.T * tiles + kGrid - 1u) / kGrid;
    if (full > slices) slices = full;
    if (slices > a.T) slices = a.T;
    if ((a.T + slices - 1u) / slices > 65535u) slices = (a.T + 65534u) / 65535u;
    a.slices = (uint32_t)slices;
    const uint32_t runs = (uint32_t)((a.T + slices - 1u) / slices);
    const bool fast = a.B % 4u == 0u && a.C % 16u == 0u && !(reinterpret_cast<uintptr_t>(a.spectra) & 15u);
    if (fast)
        hipLaunchKernelGGL(bf_filterbank_q8_kernel<true>, dim3((uint32_t)tiles, runs), dim3(256u), 0, stream, a);
    else
        hipLaunchKernelGGL(bf_filterbank_q8_kernel<false>, dim3((uint32_t)tiles, runs), dim3(256u), 0, stream, a);
    return hipGetLastError();
}

// The host side of include/dcs_filterbank.h, behind the table as in bf_integrate.hip.  No coefficients and nothing allocated;
// nr_beams is the caller's, so the one set of calls serves detected (the context's beams) and incoherent (1) spectra.
namespace bf_host {

int spectra_sums_impl(dcs_bf_context *c, const float *d_spectra, size_t spectra_bytes, uint32_t nr_spectra, uint32_t nr_beams,
                      uint32_t accumulate, double *d_sums, size_t sums_bytes, void *stream)
{
    if (int e = spectra_sums_args(c, d_spectra, nr_beams, d_sums)) return e;
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
    if (int e = filterbank_scales_args(c, d_sums, count, nr_beams, d_scales)) return e;
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
    if (int e = filterbank_q8_args(c, d_spectra, nr_spectra, nr_beams, d_scales, flags, d_filterbank, out_spectra, first_spectrum,
                                   d_clip_count))
        return e;
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
    a.descending = flags & DCS_FB_DESCENDING;
    a.level = level;
    return (int)bf_launch_filterbank_q8(a, as_stream(stream));
}

} // namespace bf_host
