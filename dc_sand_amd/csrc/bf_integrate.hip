// bf_integrate.hip -- the integrator of every post-detection output, gfx950 only: n consecutive
// blocks of a [C][nr_blocks][bs] tensor reduced to one row of spectra [nr_blocks / n][C][bs].  One kernel for detected power
// (float, bs = B), the incoherent beam (uint32, bs = 1), the Stokes parameters (int32, bs = B * nr_stokes) and the
// visibilities (int32, bs = A (A + 1)); the element type selects the reduction rule and nothing else.
//
// One lane per output element, innermost index fastest: a wave reads and writes runs of consecutive elements (and, where
// bs < 64, of consecutive channels' runs), and a lane walks its n blocks bs words apart.  No atomics and no cross-lane step,
// so the result does not depend on the launch geometry.  Offsets are 64-bit.  Where bs is 1 a lane's n words are consecutive
// and the stride is worth knowing when compiling: the loads merge four to an instruction, and 128 MiB of block powers
// integrate in 32 us instead of 193.  A unit of its own, so that an edit here recompiles 20 lines and
// not the matrix-core beamformer.

#include "bf_host.h"

#include <hip/hip_runtime.h>

#include <type_traits>

// The integrator of every post-detection output: blocks [C][nr_blocks][bs] summed n at a time into
// out [nr_blocks / n][C][bs].  The element type (bf_integrate_type, bf_host.h) selects the rule: float words are added in
// order, one rounded add each; 32-bit integer words exactly, in 64 bits, and the sum converted once
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

namespace {

// float: the ordered sum, one rounded add per block (no fma: -ffp-contract=off); accumulating starts it from what the
// output holds.  int32 / uint32: the exact 64-bit running sum -- signed or unsigned as the words are, since n <= 2^32 - 1
// words of up to 2^32 - 1 fit an unsigned 64-bit sum and no signed one -- then one conversion, RN((float)S); accumulating
// adds that, rounded once more, to what the output holds.
template <class T, bool UNIT = false> // UNIT: bs == 1, known when compiling
__global__ void __launch_bounds__(256) bf_integrate_kernel(const bf_integrate_args a)
{
    const uint32_t bs = UNIT ? 1u : a.bs;
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // (i * C + c) * bs + e
    if (g >= a.total) return;
    const uint32_t e = (uint32_t)(g % bs);
    const uint64_t ic = g / bs;
    const uint32_t c = (uint32_t)(ic % a.C);
    const uint64_t i = ic / a.C;
    const T *p = static_cast<const T *>(a.blocks) + (((uint64_t)c * a.nr_blocks + i * a.n) * bs + e);
    if constexpr (std::is_same_v<T, float>) {
        float acc = a.accumulate ? a.out[g] : p[0];
#pragma unroll 4
        for (uint32_t j = a.accumulate ? 0u : 1u; j < a.n; j++) acc = acc + p[(uint64_t)j * bs];
        a.out[g] = acc;
    } else {
        std::conditional_t<std::is_signed_v<T>, long long, unsigned long long> sum = 0;
#pragma unroll 8
        for (uint32_t j = 0; j < a.n; j++) sum += p[(uint64_t)j * bs];
        const float s = (float)sum;
        a.out[g] = a.accumulate ? a.out[g] + s : s;
    }
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_integrate()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_integrate_kernel<float>));
}

static hipError_t bf_launch_integrate(bf_integrate_type type, const bf_integrate_args &a, hipStream_t stream)
{
    if (a.total == 0u) return hipSuccess;
    const uint64_t blocks = (a.total + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks), block(256u);
    switch (type) {
    case BF_INTEGRATE_F32: hipLaunchKernelGGL(bf_integrate_kernel<float>, grid, block, 0, stream, a); break;
    case BF_INTEGRATE_U32: // a lane's n words are consecutive, and the unit-stride form reads them four to a load (section 5.22)
        if (a.bs != 1u) return hipErrorInvalidValue; // not built: no call has unsigned words more than one to a block
        hipLaunchKernelGGL((bf_integrate_kernel<uint32_t, true>), grid, block, 0, stream, a);
        break;
    case BF_INTEGRATE_I32: hipLaunchKernelGGL(bf_integrate_kernel<int32_t>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The host side, behind the table at the head of every context (bf_ctx_ext.h).  Of the context these calls use its parameters
// and its device, nothing else.  Each begins with the device-free checks of its table entry (bf_arg_checks.h), the ones its
// companion has made already; what follows needs the device or the context's sizes, or is a condition that only this side makes.
namespace bf_host {

// The one integration behind integrate_block_power, integrate_incoherent_power, integrate_stokes and integrate_visibilities:
// blocks [C][nr_blocks][bs] of 4-byte words of the named type, n at a time, into out [nr_blocks / n][C][bs].
// The caller has made its own device-free checks: n >= 1 divides nr_blocks.
int integrate_blocks(dcs_bf_context *c, bf_integrate_type type, const void *d_blocks, size_t blocks_bytes, uint64_t bs,
                     uint32_t nr_blocks, uint32_t n, uint32_t accumulate, float *d_out, size_t out_bytes, void *stream)
{
    DCS_CHECK_DEVICE(c);
    const uint64_t C = (uint32_t)c->p.nr_channels, n_out = nr_blocks / n;
    if (bs > 0xffffffffull) return DCS_ERR_UNSUPPORTED;
    if (!holds(blocks_bytes, C, nr_blocks, bs, 4u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(out_bytes, n_out, C, bs, sizeof(float))) return DCS_ERR_INVALID_ARGUMENT;
    bf_integrate_args a;
    std::memset(&a, 0, sizeof(a));
    a.blocks = d_blocks;
    a.out = d_out;
    a.total = n_out * C * bs;
    a.bs = (uint32_t)bs;
    a.C = (uint32_t)C;
    a.nr_blocks = nr_blocks;
    a.n = n;
    a.accumulate = accumulate ? 1u : 0u;
    return (int)bf_launch_integrate(type, a, as_stream(stream));
}

int integrate_block_power_impl(dcs_bf_context *c, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                               uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes, void *stream)
{
    if (int e = integrate_block_power_args(c, d_block_power, nr_blocks, blocks_per_spectrum, d_spectra)) return e;
    return integrate_blocks(c, BF_INTEGRATE_F32, d_block_power, power_bytes, (uint32_t)c->p.nr_beams, nr_blocks, blocks_per_spectrum,
                            accumulate, d_spectra, spectra_bytes, stream);
}

} // namespace bf_host
