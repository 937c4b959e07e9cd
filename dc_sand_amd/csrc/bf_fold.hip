// bf_fold.hip -- the pulsar folder (include/dcs_fold.h), gfx950 only: the 8-bit filterbanks folded
// at an integer phase model into profiles per sub-integration, channel and phase bin, the hits of every bin, and the profiles
// summed over frequency.  Every term is a byte, every sum an exact integer and the phase is 64-bit integer arithmetic, so
// nothing here depends on an order of summation.
//
// bf_fold_kernel.  A workgroup of kThreads = 1024 owns one beam, one sub-integration and a tile of W consecutive channels,
// W = 256 >> form a power of two, and keeps the tile's nbin x W words in kTileWords = 16384 words (64 KiB) of static LDS:
//
//  * W falls as nbin grows (fold_form: 256 channels up to 64 bins, 16 from 513 bins on) and is no wider than the channels
//    need (C <= 128 takes the narrowest W >= C, at least 16), so that a short band still spreads a sub-integration over lanes;
//  * the workgroup's threads are T = 1024 / W time slices of W lanes: lane (slice ts, column cl) walks the spectra k of
//    [ts * chunk, (ts + 1) * chunk), chunk = ceil(subint_len / T), of channel c0 + cl, reading the byte at k + delay[c] --
//    lanes across channels read a row's neighbouring bytes, each at its own delay.  kRows = 8 loads are in flight per lane;
//  * phi(k) is computed once per slice, at the chunk's first k, and stepped from there: phi += inc, inc += accel.  With W >= 64 a
//    wave is one slice (kUniform): the slice goes through v_readfirstlane, so the phase, the bin and the bin-change test are
//    scalar work.  With W < 64 a wave holds 64 / W slices and every lane steps its own phase;
//  * a lane adds bytes in a register while bin(k) stays the same and flushes into its LDS word on a bin change.  Several slices
//    share a word, so the flush is an integer ds_add_u32 -- the only atomics of this unit are integer adds in LDS, whose order
//    cannot show in the result.  Word (bin j, column cl) lies at j * W + (cl ^ (j & (W - 1))): a flush (one j, consecutive cl)
//    and the transposed read-out (consecutive j, one cl) are both free of bank conflicts (2-way at W = 16);
//  * the tile's words [c0 .. c0 + width)[nbin] are CONTIGUOUS in d_profiles (bin fastest, then channel), so the read-out is
//    one coalesced run of width * nbin dwords, written or added (each word by exactly one thread: no atomic in global memory).
//
// bf_fold_hits_kernel: one workgroup per (model row, sub-integration) counts the bins the same way, without the bytes.
// bf_fold_scrunch_kernel: one workgroup per (beam, sub-integration, 256 bins) sums the profile words over the channels in 64 bits.
//
// Reads stay inside the rows [first, first + nr_subints * subint_len + max_delay) of a beam whatever the tables hold: a column
// takes part only with 0 <= delay <= max_delay, and k < subint_len.  Every offset into the three tensors is 64-bit.

#include "bf_host.h"

#include <hip/hip_runtime.h>

namespace {

struct bf_fold_args {
    const uint8_t *in;               // [B][in_spectra][C], 16-byte aligned
    const dcs_bf_fold_model *models; // [P][nr_subints]; read when the work runs
    const int32_t *delays;           // nullptr (all 0), or [P][C]; an entry outside [0, max_delay] folds its column to zero
    const uint8_t *mask;             // nullptr (every column), or [C]: a zero byte folds the column to zero
    uint32_t *profiles;              // [B][out_subints][C][nbin]
    uint32_t *hits;                  // nullptr, or [P][out_subints][nbin]
    uint64_t in_spectra, first, out_subints, first_subint;
    uint32_t C, B, beams_per_model, L, nr_subints, nbin, max_delay, accumulate;
    uint32_t form, tiles; // filled by the launcher: W = 256 >> form, and the tiles of W channels
};
struct bf_scrunch_args {
    const uint32_t *profiles; // [B][out_subints][C][nbin]
    uint64_t *out;            // [B][out_subints][nbin]
    uint64_t out_subints, first_subint;
    uint32_t C, B, nr_subints, nbin, accumulate;
};

constexpr uint32_t kThreads = 1024;      // sixteen waves: two workgroups fill a CU's 32 wave slots
constexpr uint32_t kTileWords = 16384;   // 64 KiB of static LDS: nbin * W words at the most
constexpr uint32_t kMaxWidth = 256;      // channels of the widest tile
constexpr uint32_t kMinWidth = 16;       // of the narrowest: nbin = 1024
constexpr uint32_t kRows = 8;            // spectra whose loads a lane has in flight
constexpr uint32_t kHitsThreads = 256;
constexpr uint32_t kMaxBins = 1024;
constexpr uint32_t kScrunchThreads = 256;

static_assert(kMinWidth * kMaxBins == kTileWords && kMaxWidth * 64u == kTileWords, "the tile's words at both ends of nbin");

// phi(k) of a model, modulo 2^64; k (k - 1) / 2 is exact
__device__ __forceinline__ uint64_t phase_at(const dcs_bf_fold_model &m, uint64_t k)
{
    return m.phase0 + k * m.step + (k * (k - 1u) / 2u) * m.accel;
}
__device__ __forceinline__ uint32_t bin_of(uint64_t phi, uint32_t nbin) { return __umulhi((uint32_t)(phi >> 32), nbin); }

template <bool kUniform>
__global__ void __launch_bounds__(kThreads) bf_fold_kernel(const bf_fold_args a)
{
    __shared__ uint32_t s_tile[kTileWords];

    const uint32_t tid = threadIdx.x;
    const uint32_t W = kMaxWidth >> a.form, wmask = W - 1u, T = kThreads / W;
    // tiles fastest: the workgroups that run together read neighbouring bytes of the same rows
    uint32_t blk = blockIdx.x;
    const uint32_t c0 = (blk % a.tiles) * W;
    blk /= a.tiles;
    const uint32_t beam = blk % a.B, s = blk / a.B;
    const uint32_t p = beam / a.beams_per_model;
    const uint32_t width = a.C - c0 < W ? a.C - c0 : W; // the tile's channels that exist
    const uint32_t cl = tid & wmask, c = c0 + cl;
    uint32_t ts = tid >> (8u - a.form);
    if (kUniform) ts = (uint32_t)__builtin_amdgcn_readfirstlane((int)ts); // a wave is one slice

    for (uint32_t i = tid; i < a.nbin * W; i += kThreads) s_tile[i] = 0u;

    // whether this lane's column takes part, and where it reads
    int32_t d = 0;
    bool on = c < a.C && (!a.mask || a.mask[c] != 0u);
    if (on && a.delays) {
        d = a.delays[(size_t)p * a.C + c];
        on = d >= 0 && (uint32_t)d <= a.max_delay;
    }
    const dcs_bf_fold_model m = a.models[(size_t)p * a.nr_subints + s];
    const uint32_t chunk = (a.L + T - 1u) / T;
    const uint32_t k0 = ts * chunk < a.L ? ts * chunk : a.L; // chunk <= 2^24 and ts < 64: no overflow
    const uint32_t k1 = a.L - k0 < chunk ? a.L : k0 + chunk;
    __syncthreads();

    if (k0 < k1) { // the same in every lane of a slice
        // row k0 of this lane's column: inside [first, first + nr_subints * L + max_delay) where the lane is on
        const uint8_t *src = a.in + ((size_t)beam * a.in_spectra + a.first + (size_t)s * a.L + k0 + (on ? (uint32_t)d : 0u)) * (size_t)a.C + c;
        uint64_t phi = phase_at(m, k0);
        uint64_t inc = m.step + (uint64_t)k0 * m.accel; // phi(k + 1) - phi(k) = step + k accel
        uint32_t cur = bin_of(phi, a.nbin), acc = 0u;
        for (uint32_t k = k0; k < k1; k += kRows) {
            uint32_t v[kRows];
#pragma unroll
            for (uint32_t i = 0; i < kRows; i++) v[i] = on && k + i < k1 ? (uint32_t)src[(size_t)i * a.C] : 0u;
            src += (size_t)kRows * a.C;
#pragma unroll
            for (uint32_t i = 0; i < kRows; i++) {
                // past k1 the bytes are zeros: a flush there adds nothing
                const uint32_t bin = bin_of(phi, a.nbin);
                if (bin != cur) {
                    if (acc) atomicAdd(&s_tile[cur * W + (cl ^ (cur & wmask))], acc);
                    acc = 0u;
                    cur = bin;
                }
                acc += v[i];
                phi += inc;
                inc += m.accel;
            }
        }
        if (acc) atomicAdd(&s_tile[cur * W + (cl ^ (cur & wmask))], acc);
    }
    __syncthreads();

    // the tile's words of d_profiles are one run of width * nbin dwords
    uint32_t *out = a.profiles + (((size_t)beam * a.out_subints + a.first_subint + s) * a.C + c0) * (size_t)a.nbin;
    const uint32_t words = width * a.nbin;
    for (uint32_t i = tid; i < words; i += kThreads) {
        const uint32_t ch = i / a.nbin, j = i - ch * a.nbin;
        const uint32_t v = s_tile[j * W + (ch ^ (j & wmask))];
        out[i] = a.accumulate ? out[i] + v : v;
    }
}

// One workgroup per (model row, sub-integration): the bins' counts.  Every thread walks a chunk of the spectra, counts while
// the bin stays the same and adds the count into LDS on a change (integer ds_add_u32).
__global__ void __launch_bounds__(kHitsThreads) bf_fold_hits_kernel(const bf_fold_args a)
{
    __shared__ uint32_t s_hits[kMaxBins];
    const uint32_t tid = threadIdx.x;
    const uint32_t s = blockIdx.x % a.nr_subints, p = blockIdx.x / a.nr_subints;
    for (uint32_t i = tid; i < a.nbin; i += kHitsThreads) s_hits[i] = 0u;
    const dcs_bf_fold_model m = a.models[(size_t)p * a.nr_subints + s];
    const uint32_t chunk = (a.L + kHitsThreads - 1u) / kHitsThreads;
    const uint32_t k0 = tid * chunk < a.L ? tid * chunk : a.L; // chunk <= 2^16 and tid < 256: no overflow
    const uint32_t k1 = a.L - k0 < chunk ? a.L : k0 + chunk;
    __syncthreads();
    if (k0 < k1) {
        uint64_t phi = phase_at(m, k0);
        uint64_t inc = m.step + (uint64_t)k0 * m.accel;
        uint32_t cur = bin_of(phi, a.nbin), n = 0u;
        for (uint32_t k = k0; k < k1; k++) {
            const uint32_t bin = bin_of(phi, a.nbin);
            if (bin != cur) {
                atomicAdd(&s_hits[cur], n);
                n = 0u;
                cur = bin;
            }
            n++;
            phi += inc;
            inc += m.accel;
        }
        atomicAdd(&s_hits[cur], n);
    }
    __syncthreads();
    uint32_t *out = a.hits + ((size_t)p * a.out_subints + a.first_subint + s) * (size_t)a.nbin;
    for (uint32_t i = tid; i < a.nbin; i += kHitsThreads) out[i] = a.accumulate ? out[i] + s_hits[i] : s_hits[i];
}

// One workgroup per (beam, sub-integration, tile of up to 256 bins): jw = the tile's bins rounded up to a power of two lanes
// along the bins, 256 / jw groups of lanes along the channels; a lane sums its channels in 64 bits, the groups meet in LDS
// (integer ds_add_u64).
__global__ void __launch_bounds__(kScrunchThreads) bf_fold_scrunch_kernel(const bf_scrunch_args a, uint32_t jw, uint32_t bin_tiles)
{
    __shared__ unsigned long long s_sum[kScrunchThreads];
    const uint32_t tid = threadIdx.x;
    uint32_t blk = blockIdx.x;
    const uint32_t j0 = (blk % bin_tiles) * jw;
    blk /= bin_tiles;
    const uint32_t s = blk % a.nr_subints, beam = blk / a.nr_subints;
    const uint32_t jl = tid & (jw - 1u), j = j0 + jl, group = tid / jw, groups = kScrunchThreads / jw;
    s_sum[tid] = 0ull;
    __syncthreads();
    if (j < a.nbin) {
        const uint32_t *in = a.profiles + (((size_t)beam * a.out_subints + a.first_subint + s) * a.C) * (size_t)a.nbin + j;
        unsigned long long sum = 0ull;
        for (uint32_t c = group; c < a.C; c += groups) sum += in[(size_t)c * a.nbin];
        atomicAdd(&s_sum[jl], sum);
    }
    __syncthreads();
    if (group == 0u && j < a.nbin) {
        uint64_t *out = a.out + ((size_t)beam * a.out_subints + a.first_subint + s) * (size_t)a.nbin + j;
        *out = a.accumulate ? *out + (uint64_t)s_sum[jl] : (uint64_t)s_sum[jl];
    }
}

// The form of a fold: the tile is W = 256 >> form channels.  As many as nbin leaves room for in kTileWords, and no more than
// the band needs, down to kMinWidth
uint32_t fold_form(uint32_t nbin, uint32_t C)
{
    uint32_t form = 0u;
    while ((kMaxWidth >> form) * nbin > kTileWords) form++;
    while ((kMaxWidth >> form) > kMinWidth && (kMaxWidth >> (form + 1u)) >= C) form++;
    return form;
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_fold()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_fold_kernel<true>));
}

static hipError_t bf_launch_fold(const bf_fold_args &args, hipStream_t stream)
{
    if (args.nr_subints == 0u) return hipSuccess;
    bf_fold_args a = args;
    a.form = fold_form(a.nbin, a.C);
    const uint32_t W = kMaxWidth >> a.form;
    a.tiles = (a.C - 1u) / W + 1u;
    const uint64_t blocks = (uint64_t)a.tiles * a.B * a.nr_subints;
    const uint64_t hits_blocks = (uint64_t)(a.B / a.beams_per_model) * a.nr_subints;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (W >= 64u)
        hipLaunchKernelGGL(bf_fold_kernel<true>, dim3((uint32_t)blocks), dim3(kThreads), 0, stream, a);
    else
        hipLaunchKernelGGL(bf_fold_kernel<false>, dim3((uint32_t)blocks), dim3(kThreads), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.hits) return e;
    hipLaunchKernelGGL(bf_fold_hits_kernel, dim3((uint32_t)hits_blocks), dim3(kHitsThreads), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_fold_scrunch(const bf_scrunch_args &a, hipStream_t stream)
{
    if (a.nr_subints == 0u) return hipSuccess;
    uint32_t jw = 1u;
    while (jw < a.nbin && jw < kScrunchThreads) jw <<= 1;
    const uint32_t bin_tiles = (a.nbin - 1u) / jw + 1u;
    const uint64_t blocks = (uint64_t)bin_tiles * a.nr_subints * a.B;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_fold_scrunch_kernel, dim3((uint32_t)blocks), dim3(kScrunchThreads), 0, stream, a, jw, bin_tiles);
    return hipGetLastError();
}

// The host side of include/dcs_fold.h, behind the table as in bf_dedisperse.hip.  No coefficients, nothing allocated, and
// math_mode plays no part.
namespace bf_host {

int fold_q8_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra, uint64_t first_spectrum,
                 uint32_t subint_len, uint32_t nr_subints, uint32_t nr_beams, uint32_t beams_per_model,
                 const dcs_bf_fold_model *d_models, size_t models_bytes, const int32_t *d_delays, size_t delays_bytes, uint32_t max_delay,
                 const uint8_t *d_channel_mask, uint32_t nbin, uint32_t *d_profiles, size_t profiles_bytes, uint32_t *d_hits,
                 size_t hits_bytes, uint64_t out_subints, uint64_t first_subint, uint32_t accumulate, void *stream)
{
    if (int e = fold_q8_args(c, d_filterbank, in_spectra, first_spectrum, subint_len, nr_subints, nr_beams, beams_per_model, d_models,
                             d_delays, max_delay, nbin, d_profiles, d_hits, out_subints, first_subint, accumulate))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels, P = nr_beams / beams_per_model;
    if (!holds(filterbank_bytes, nr_beams, in_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(models_bytes, P, nr_subints, sizeof(dcs_bf_fold_model), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (d_delays && !holds(delays_bytes, P, C, sizeof(int32_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(profiles_bytes, nr_beams, out_subints, (uint64_t)C * nbin, sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    if (d_hits && !holds(hits_bytes, P, out_subints, nbin, sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_fold_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_filterbank;
    a.models = d_models;
    a.delays = d_delays;
    a.mask = d_channel_mask;
    a.profiles = d_profiles;
    a.hits = d_hits;
    a.in_spectra = in_spectra;
    a.first = first_spectrum;
    a.out_subints = out_subints;
    a.first_subint = first_subint;
    a.C = C;
    a.B = nr_beams;
    a.beams_per_model = beams_per_model;
    a.L = subint_len;
    a.nr_subints = nr_subints;
    a.nbin = nbin;
    a.max_delay = max_delay;
    a.accumulate = accumulate;
    return (int)bf_launch_fold(a, as_stream(stream));
}

int fold_scrunch_impl(dcs_bf_context *c, const uint32_t *d_profiles, size_t profiles_bytes, uint32_t nr_beams, uint64_t out_subints,
                      uint64_t first_subint, uint32_t nr_subints, uint32_t nbin, uint64_t *d_scrunched, size_t scrunched_bytes,
                      uint32_t accumulate, void *stream)
{
    if (int e = fold_scrunch_args(c, d_profiles, nr_beams, out_subints, first_subint, nr_subints, nbin, d_scrunched, accumulate)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(profiles_bytes, nr_beams, out_subints, (uint64_t)C * nbin, sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(scrunched_bytes, nr_beams, out_subints, nbin, sizeof(uint64_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_scrunch_args a;
    std::memset(&a, 0, sizeof(a));
    a.profiles = d_profiles;
    a.out = d_scrunched;
    a.out_subints = out_subints;
    a.first_subint = first_subint;
    a.C = C;
    a.B = nr_beams;
    a.nr_subints = nr_subints;
    a.nbin = nbin;
    a.accumulate = accumulate;
    return (int)bf_launch_fold_scrunch(a, as_stream(stream));
}

} // namespace bf_host
