// bf_channeliser.hip -- the polyphase channeliser (include/dcs_channeliser.h), gfx950 only: float
// [nr_inputs][in_stride][{re, im}] -> a FIR over P rows of N pairs, an N-point FFT, and the spectra in the sample tensor's
// order [N][out_blocks][out_inputs][16][{re, im}], as floats or quantised to int8 with a gain per (input, channel).
//
// The arithmetic is a radix-2 butterfly network with a caller's twiddle table, every operation one fp32 operation
// (-ffp-contract=off): whatever groups the butterflies gives the same bits.  One kernel template per log2 N and per epilogue.
//
// A workgroup takes items of F = 2^LT / N transforms -- 16 spectra of up to 4 adjacent inputs where N <= 128, of 2 at N = 256,
// of one at N = 512, 8 spectra of one input at N = 1024 and at N = 2048 (LT = 14) -- in three steps on one LDS array of 2^LT
// pairs, transform f's element i at index I = f N + i:
//
//  1. FIR.  A thread owns a column r of an input: it loads the SP + P - 1 pairs z[(n + q) N + r] of the item once (adjacent
//     lanes adjacent r: the loads coalesce), forms the SP spectra's y[r] in registers, taps in order, and writes them to
//     i = bitrev(r): the permutation costs an address.
//  2. The log2 N stages in groups of 3 or 4: a task holds the 8 or 16 elements that differ in the group's index bits in
//     registers, does the group's butterflies on them as the network states them, and writes them back in place.  The twiddle
//     of a butterfly is read from the table where it is not entry 0 or N / 4; those two are no arithmetic.
//  3. The epilogue reads the spectra in output order: a thread makes 16 bytes of one run -- two pairs of floats, or eight
//     quantised pairs -- and stores them with one 16-byte store.
//
// LDS pitch.  Index I is kept at slot I + (I >> 5) + (I >> 10) of 8 bytes: one slot of padding per 256-byte bank row, one more
// per 32 rows.  The bank of a slot (ds_read_b64: 32 slots) is then the sum over the index bits of bit_p 2^(p mod 5), modulo
// 32: 32 lanes that differ in five index bits of distinct p mod 5 hit 32 banks.  Every step numbers its tasks so that the five
// low lane bits go to such index bits (lane_map below, made when compiling), so every read and write of steps 2 and 3 is
// conflict-free; the writes of step 1 (bit-reversed columns) are at most two to a bank.  Offsets into the tensors are size_t.

#include "bf_host.h"

#include <hip/hip_runtime.h>

// The polyphase channeliser (include/dcs_channeliser.h): float [nr_inputs][in_stride][2]
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

namespace {

typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kGrid = 1u << 16; // workgroups at most (64 to 256 per CU); they walk the items beyond
constexpr int kMaxTaps = 16;

constexpr int total_bits(int L) { return L == 6 ? 12 : L == 11 ? 14 : 13; }   // LT: the LDS array holds 2^LT pairs
constexpr int threads_of(int L) { return L >= 10 ? 512 : 256; } // 512 where the registers leave four waves a SIMD
constexpr int spectra_bits(int L) { return total_bits(L) - L < 4 ? total_bits(L) - L : 4; } // log2 SP: spectra per item
constexpr int radix_bits(int L, int g)                                                      // stages of group g
{
    constexpr int r[6][3] = {{3, 3, 0}, {4, 3, 0}, {4, 4, 0}, {3, 3, 3}, {4, 3, 3}, {4, 4, 3}};
    return r[L - 6][g];
}
constexpr uint32_t slot(uint32_t I) { return I + (I >> 5) + (I >> 10); }
constexpr uint32_t slots(int LT) { return slot((1u << LT) - 1u) + 1u; }

// Which index bit each bit of a task number goes to.  The index bits of `excluded` are the task's own (it walks them); of
// the others the `forced_n` from `forced_lo` up come first, in order (the epilogue: the lanes of one run are adjacent); then
// the lowest bits whose p mod 5 is still free, until five are placed; then the rest, ascending.  Without forced bits the
// first five are ordered by p mod 5, so that lane bit j moves the bank by 2^j: 16 adjacent lanes also differ modulo 16
// slots, the banks of a ds_write_b64
struct lane_map {
    int pos[16];
    int n;
};
constexpr lane_map make_map(int total, uint32_t excluded, int forced_lo, int forced_n)
{
    lane_map m{};
    bool taken[16] = {}, residue[5] = {};
    int n = 0;
    for (int i = 0; i < forced_n; i++) {
        m.pos[n++] = forced_lo + i;
        taken[forced_lo + i] = true;
        residue[(forced_lo + i) % 5] = true;
    }
    for (int p = 0; p < total && n < 5; p++)
        if (!((excluded >> p) & 1u) && !taken[p] && !residue[p % 5]) {
            m.pos[n++] = p;
            taken[p] = true;
            residue[p % 5] = true;
        }
    if (forced_n == 0)
        for (int i = 0; i < n; i++)
            for (int j = i + 1; j < n; j++)
                if (m.pos[j] % 5 < m.pos[i] % 5) {
                    const int t = m.pos[i];
                    m.pos[i] = m.pos[j];
                    m.pos[j] = t;
                }
    for (int p = 0; p < total; p++)
        if (!((excluded >> p) & 1u) && !taken[p]) m.pos[n++] = p;
    m.n = n;
    return m;
}

template <int L, int B, int R>
__device__ __forceinline__ void fft_group(floatx2 *v, const floatx2 *__restrict__ W, uint32_t f_limit)
{
    constexpr int LT = total_bits(L), NT = threads_of(L);
    constexpr lane_map M = make_map(LT, ((1u << R) - 1u) << B, 0, 0);
    static_assert(M.n == LT - R, "every other index bit is a task bit");
    for (uint32_t T = threadIdx.x; T < (1u << (LT - R)); T += NT) {
        uint32_t I = 0u;
#pragma unroll
        for (int j = 0; j < M.n; j++) I |= ((T >> j) & 1u) << M.pos[j];
        if ((I >> L) >= f_limit) continue; // a transform of an input that the call does not have
        const uint32_t jb = I & ((1u << B) - 1u);
        floatx2 x[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); k++) x[k] = v[slot(I + ((uint32_t)k << B))];
#pragma unroll
        for (int u = 0; u < R; u++) {
#pragma unroll
            for (int k = 0; k < (1 << R); k++) {
                if ((k >> u) & 1) continue;
                const int kl = k & ((1 << u) - 1);
                // j = jb + kl 2^B of m = 2^(B + u); q = j N / (2 m)
                const bool one = kl == 0 && jb == 0u;
                const bool quarter = u >= 1 ? (kl == (1 << (u - 1)) && jb == 0u) : (B >= 1 && jb == (1u << (B >= 1 ? B - 1 : 0)));
                const floatx2 a = x[k], b = x[k | (1 << u)];
                floatx2 t;
                if (one) {
                    t = b;
                } else if (quarter) {
                    t = floatx2{b.y, -b.x};
                } else {
                    // (w.re b.re - w.im b.im, w.re b.im + w.im b.re) as two products of pairs and one sum of pairs: the
                    // sign of w.im moves into the factor, which rounds the same
                    const floatx2 w = W[(jb + ((uint32_t)kl << B)) << (L - 1 - B - u)];
                    t = floatx2{w.x, w.x} * b + floatx2{-w.y, w.y} * floatx2{b.y, b.x};
                }
                x[k] = a + t;
                x[k | (1 << u)] = a - t;
            }
        }
#pragma unroll
        for (int k = 0; k < (1 << R); k++) v[slot(I + ((uint32_t)k << B))] = x[k];
    }
}

// include/dcs_beam_quant.h's quantiser: y = RN(x k); NaN -> -128; otherwise clamp(rint(y), -127, 127); the byte, and the count
__device__ __forceinline__ uint32_t q8(float x, float k, uint32_t &n_clip)
{
    const float y = x * k;
    const float ry = rintf(y);
    n_clip += !(fabsf(ry) <= 127.0f) ? 1u : 0u; // NaN included
    const float q = y != y ? -128.0f : __builtin_amdgcn_fmed3f(ry, -127.0f, 127.0f);
    return (uint32_t)(int)q & 0xffu;
}

template <int L, bool Q8>
__global__ void __launch_bounds__(threads_of(L)) bf_channelise_kernel(const bf_chan_args a)
{
    constexpr int LT = total_bits(L), NT = threads_of(L), LS = spectra_bits(L);
    constexpr uint32_t N = 1u << L, SP = 1u << LS, IG = 1u << (LT - L - LS); // spectra per item; inputs per item
    constexpr uint32_t PASSES = 16u / SP;
    __shared__ floatx2 v[slots(LT)];
    __shared__ uint32_t clip[4];
    static_assert(IG <= 4u, "a counter per input of the item");
    const uint32_t P = a.P;
    const floatx2 *__restrict__ W = reinterpret_cast<const floatx2 *>(a.twiddles);

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint32_t pass = (uint32_t)(item % PASSES);
        const uint64_t rest = item / PASSES;
        const uint32_t i0 = (uint32_t)(rest % a.groups) * IG; // the item's first input, of the call's
        const uint64_t blk = rest / a.groups;                 // the item's block of 16 spectra, of the call's
        const uint32_t n_in = a.nr_inputs - i0 < IG ? a.nr_inputs - i0 : IG;
        const uint32_t s0 = pass * SP; // the item's first spectrum of the block
        __syncthreads();               // the previous item's reads of v and clip are done
        if (Q8 && threadIdx.x < 4u) clip[threadIdx.x] = 0u;

        // 1. the FIR: column r of input i0 + il
        for (uint32_t col = threadIdx.x; col < n_in * N; col += NT) {
            const uint32_t il = col >> L, r = col & (N - 1u);
            const floatx2 *z = reinterpret_cast<const floatx2 *>(a.in) + (size_t)(i0 + il) * (size_t)a.in_stride +
                               ((size_t)blk * 16u + s0) * (size_t)N + r;
            floatx2 w[SP + kMaxTaps - 1];
#pragma unroll
            for (uint32_t q = 0; q < SP + kMaxTaps - 1; q++) w[q] = q < SP + P - 1u ? z[(size_t)q * N] : floatx2{0.0f, 0.0f};
            floatx2 y[SP];
#pragma unroll
            for (uint32_t p = 0; p < (uint32_t)kMaxTaps; p++) {
                if (p < P) {
                    const float h = a.taps[p * N + r];
#pragma unroll
                    for (uint32_t s = 0; s < SP; s++) {
                        const floatx2 term = floatx2{h, h} * w[s + p];
                        y[s] = p == 0u ? term : y[s] + term;
                    }
                }
            }
            const uint32_t i = __brev(r) >> (32 - L);
#pragma unroll
            for (uint32_t s = 0; s < SP; s++) v[slot((((il << LS) + s) << L) + i)] = y[s];
        }
        __syncthreads();

        // 2. the stages
        const uint32_t f_limit = n_in << LS;
        fft_group<L, 0, radix_bits(L, 0)>(v, W, f_limit);
        __syncthreads();
        fft_group<L, radix_bits(L, 0), radix_bits(L, 1)>(v, W, f_limit);
        __syncthreads();
        if constexpr (radix_bits(L, 2) != 0) {
            fft_group<L, radix_bits(L, 0) + radix_bits(L, 1), radix_bits(L, 2)>(v, W, f_limit);
            __syncthreads();
        }

        // 3. the epilogue: a task is E consecutive spectra of one (channel, input): 16 bytes
        constexpr int LE = Q8 ? 3 : 1;
        static_assert(LE <= LS, "a task's spectra are of one item");
        constexpr lane_map M = make_map(LT, ((1u << LE) - 1u) << L, L + LE, LT - L - LE);
        static_assert(M.n == LT - LE, "every other index bit is a task bit");
        for (uint32_t T = threadIdx.x; T < (1u << (LT - LE)); T += NT) {
            uint32_t I = 0u;
#pragma unroll
            for (int j = 0; j < M.n; j++) I |= ((T >> j) & 1u) << M.pos[j];
            const uint32_t k = I & (N - 1u), f = I >> L, il = f >> LS, s = f & (SP - 1u);
            if (il >= n_in) continue;
            const uint32_t c = a.order ? (k + N / 2u) & (N - 1u) : k;
            const size_t pair = ((((size_t)c * (size_t)a.out_blocks + (size_t)a.first_block + (size_t)blk) * (size_t)a.out_inputs +
                                  (size_t)a.first_input + i0 + il) << 4) + s0 + s;
            if constexpr (Q8) {
                const float gain = a.gains[(size_t)(i0 + il) * N + c];
                uint32_t n_clip = 0u, word[4];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const floatx2 x0 = v[slot(I + ((uint32_t)(2 * e) << L))], x1 = v[slot(I + ((uint32_t)(2 * e + 1) << L))];
                    word[e] = q8(x0.x, gain, n_clip) | q8(x0.y, gain, n_clip) << 8 | q8(x1.x, gain, n_clip) << 16 |
                              q8(x1.y, gain, n_clip) << 24;
                }
                *reinterpret_cast<intx4 *>(a.out_q8 + pair * 2u) = intx4{(int)word[0], (int)word[1], (int)word[2], (int)word[3]};
                if (a.clip_count && n_clip) atomicAdd(&clip[il], n_clip);
            } else {
                const floatx2 x0 = v[slot(I)], x1 = v[slot(I + N)];
                *reinterpret_cast<floatx4 *>(a.out + pair * 2u) = floatx4{x0.x, x0.y, x1.x, x1.y};
            }
        }
        if constexpr (Q8) {
            if (a.clip_count) { // uniform
                __syncthreads();
                if (threadIdx.x < n_in && clip[threadIdx.x]) atomicAdd(a.clip_count + i0 + threadIdx.x, (unsigned long long)clip[threadIdx.x]);
            }
        }
    }
}

template <int L, bool Q8>
hipError_t launch(const bf_chan_args &args, hipStream_t stream)
{
    constexpr int LT = total_bits(L), LS = spectra_bits(L);
    constexpr uint32_t IG = 1u << (LT - L - LS);
    bf_chan_args a = args;
    a.groups = (a.nr_inputs + IG - 1u) / IG;
    a.items = (uint64_t)(a.nr_spectra / 16u) * a.groups * (16u >> LS);
    hipLaunchKernelGGL((bf_channelise_kernel<L, Q8>), dim3((uint32_t)(a.items < kGrid ? a.items : kGrid)), dim3(threads_of(L)), 0, stream, a);
    return hipGetLastError();
}

template <int L>
hipError_t warm()
{
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_channelise_kernel<L, false>));
    if (e != hipSuccess) return e;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_channelise_kernel<L, true>));
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_channeliser()
{
    hipError_t e = warm<6>();
    if (e == hipSuccess) e = warm<7>();
    if (e == hipSuccess) e = warm<8>();
    if (e == hipSuccess) e = warm<9>();
    if (e == hipSuccess) e = warm<10>();
    if (e == hipSuccess) e = warm<11>();
    return e;
}

static hipError_t bf_launch_channelise(const bf_chan_args &a, hipStream_t stream)
{
    if (a.nr_spectra == 0u || a.nr_inputs == 0u) return hipSuccess;
    if (a.nr_spectra % 16u != 0u || a.P < 1u || a.P > (uint32_t)kMaxTaps || a.order > 1u || (a.out != nullptr) == (a.out_q8 != nullptr))
        return hipErrorInvalidValue;
    const bool q = a.out_q8 != nullptr;
    switch (a.N) {
    case 64u: return q ? launch<6, true>(a, stream) : launch<6, false>(a, stream);
    case 128u: return q ? launch<7, true>(a, stream) : launch<7, false>(a, stream);
    case 256u: return q ? launch<8, true>(a, stream) : launch<8, false>(a, stream);
    case 512u: return q ? launch<9, true>(a, stream) : launch<9, false>(a, stream);
    case 1024u: return q ? launch<10, true>(a, stream) : launch<10, false>(a, stream);
    case 2048u: return q ? launch<11, true>(a, stream) : launch<11, false>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

// The host side of include/dcs_channeliser.h, behind the table as in bf_integrate.hip.  Of the context these use the device
// alone: every size is an argument, and the device-free checks are all the checks there are.  Nothing allocated: one launch each.
namespace bf_host {

static int channelise_launch(dcs_bf_context *c, uint32_t N, uint32_t P, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                             uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order, const float *d_gains,
                             float *d_out, int8_t *d_out_q8, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs,
                             uint32_t first_input, unsigned long long *d_clip_count, void *stream)
{
    DCS_CHECK_DEVICE(c);
    if (nr_spectra == 0u || nr_inputs == 0u) return DCS_OK;
    bf_chan_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_in;
    a.taps = d_taps;
    a.twiddles = d_twiddles;
    a.gains = d_gains;
    a.out = d_out;
    a.out_q8 = d_out_q8;
    a.clip_count = d_clip_count;
    a.in_stride = in_stride;
    a.out_blocks = out_blocks;
    a.first_block = first_block;
    a.N = N;
    a.P = P;
    a.nr_inputs = nr_inputs;
    a.nr_spectra = nr_spectra;
    a.order = order;
    a.out_inputs = out_inputs;
    a.first_input = first_input;
    return (int)bf_launch_channelise(a, as_stream(stream));
}

int channelise_impl(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra, const float *d_in,
                    size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order, float *d_out,
                    size_t out_bytes, uint64_t out_blocks, uint64_t first_block, uint32_t out_inputs, uint32_t first_input, void *stream)
{
    if (int e = channelise_args(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles, order,
                                d_out, 4u, out_bytes, out_blocks, first_block, out_inputs, first_input))
        return e;
    return channelise_launch(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_stride, d_taps, d_twiddles, order, nullptr, d_out,
                             nullptr, out_blocks, first_block, out_inputs, first_input, nullptr, stream);
}

int channelise_q8_impl(dcs_bf_context *c, uint32_t nr_channels, uint32_t nr_taps, uint32_t nr_inputs, uint32_t nr_spectra,
                       const float *d_in, size_t in_bytes, uint64_t in_stride, const float *d_taps, const float *d_twiddles, uint32_t order,
                       const float *d_gains, int8_t *d_out_q8, size_t out_bytes, uint64_t out_blocks, uint64_t first_block,
                       uint32_t out_inputs, uint32_t first_input, unsigned long long *d_clip_count, void *stream)
{
    if (int e = channelise_q8_args(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_bytes, in_stride, d_taps, d_twiddles, order,
                                   d_gains, d_out_q8, out_bytes, out_blocks, first_block, out_inputs, first_input, d_clip_count))
        return e;
    return channelise_launch(c, nr_channels, nr_taps, nr_inputs, nr_spectra, d_in, in_stride, d_taps, d_twiddles, order, d_gains, nullptr,
                             d_out_q8, out_blocks, first_block, out_inputs, first_input, d_clip_count, stream);
}

} // namespace bf_host
