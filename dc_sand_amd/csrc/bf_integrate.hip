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

#include "bf_kernels.h"

#include <hip/hip_runtime.h>

#include <type_traits>

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

hipError_t bf_launch_integrate(bf_integrate_type type, const bf_integrate_args &a, hipStream_t stream)
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
