// bf_incoherent.hip -- the incoherent beam (include/dcs_incoherent_beam.h), gfx950 only: the
// antennas' own power summed over each 16-sample block, exactly (bf_integrate.hip integrates those block powers).
//
// The sample tensor int8 [C][nt / 16][A][16][{re, im}] is R = C * nt / 16 contiguous rows of A * 32 bytes, and a row
// reduces to one dword.  The kernel is a stream of 16-byte loads bound by the HBM read rate (2 A bytes in per sample and
// channel, 0.25 bytes out per A * 32 read):
//
//  * a lane loads 16 bytes -- eight samples of one antenna, half of its block -- and squares and sums them with four
//    v_dot4c_i32_i8 (the same register as both operands).  A wave-wide load is 1 KiB: 32 antennas of one row, and a row
//    is NC = ceil(A / 32) of them.  Lane l of load k holds 16-byte unit u = 64 k + l of its row, antenna u / 2;
//  * a wave takes RPW = max(1, 8 / NC) consecutive rows at a time and issues all their RPW * NC (5 to 8) loads before
//    the first use: 5 to 8 KiB in flight per wave, and eight waves per SIMD fit (the register report is in DESIGN.md);
//  * an antenna's flag (its weight != 0; lanes behind a ragged row's end count as flagged off) is a select on the
//    lane's partial sum.  The flags are read once per wave, in front of its loop over the rows;
//  * the partial sums of a row's loads accumulate in the lane; then one integer wave reduction per row: four DPP adds
//    give every lane its 16-lane row's sum, four v_readlane and three scalar adds the wave's.  No LDS.  Integer
//    addition is exact in any order, so this is the cheapest one, not a contractual one;
//  * lane r keeps row r's sum and lanes 0 .. RPW - 1 write RPW consecutive dwords with one vector store.
//
// Where A is a multiple of 32 every lane of every load is busy.  A ragged A clamps the address of a lane behind the
// row's end to the row's first unit (in bounds, and a line the wave fetches anyway) and flags it off; a group of rows
// that runs over the last row repeats that row and does not store the repeats.  A < 32 leaves lanes idle instead of
// packing several rows into one load: correct, and no production shape.
// Byte offsets are 64-bit.  Nothing here rounds: -ffp-contract and the float flags of the build play no part.

#include "bf_host.h"

#include <hip/hip_runtime.h>

// The incoherent beam (include/dcs_incoherent_beam.h): the sample tensor as
// rows = C * nT16 rows of A * 32 bytes, each summed to one exact dword of block_power [C][nT16]
struct bf_incoh_args {
    const int8_t *ant;     // [rows][A][16][2], 16-byte aligned
    const float *weights;  // nullptr (every antenna), or [A] flags: antenna a takes part iff weights[a] != 0
    uint32_t *block_power; // [rows]
    uint64_t rows;
    uint64_t n_groups;     // filled by the launcher: groups of rows that a wave carries at once
    uint32_t A;            // 1 .. 256
};

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kLoads = 8;  // 16-byte loads a lane has in flight, at most
constexpr uint32_t kWaves = 4;  // waves per workgroup
constexpr uint32_t kGrid = 2048; // workgroups at most: 256 CUs x 8 workgroups = 8 waves per SIMD, each walking its share of the rows

template <int CTRL>
__device__ __forceinline__ int add_dpp(int v)
{
    return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

// The sum of v over the 64 lanes (all active), wave-uniform
__device__ __forceinline__ int wave_sum(int v)
{
    v = add_dpp<0xB1>(v);  // quad_perm [1, 0, 3, 2]
    v = add_dpp<0x4E>(v);  // quad_perm [2, 3, 0, 1]
    v = add_dpp<0x141>(v); // row_half_mirror
    v = add_dpp<0x140>(v); // row_mirror: every lane has the sum of its row of 16
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ int sum_of_squares(const intx4 v)
{
    int s = __builtin_amdgcn_sdot4(v.x, v.x, 0, false);
    s = __builtin_amdgcn_sdot4(v.y, v.y, s, false);
    s = __builtin_amdgcn_sdot4(v.z, v.z, s, false);
    return __builtin_amdgcn_sdot4(v.w, v.w, s, false);
}

template <uint32_t NC> // wave-wide loads per row: ceil(A / 32), 1 .. 8
__global__ void __launch_bounds__(kWaves * 64) bf_incoherent_power_kernel(const bf_incoh_args a)
{
    constexpr uint32_t RPW = kLoads / NC; // rows a wave carries at once: 8, 4, 2, 2, 1, 1, 1, 1
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t units = a.A * 2u; // 16-byte units per row
    // this lane's units of a row: byte offsets, and whether their antenna takes part
    uint32_t off[NC];
    bool on[NC];
#pragma unroll
    for (uint32_t k = 0; k < NC; k++) {
        const uint32_t u = k * 64u + lane;
        const bool in_row = u < units;
        off[k] = in_row ? u * 16u : 0u;
        on[k] = in_row && (!a.weights || a.weights[u >> 1] != 0.0f); // -0 == 0; NaN != 0
    }
    const uint64_t row_bytes = (uint64_t)units * 16u;
    const char *ant = reinterpret_cast<const char *>(a.ant);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    // the wave's number as a scalar: the row addresses below are then scalar arithmetic, and a load is base + lane offset
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < a.n_groups; g += nwaves) {
        const uint64_t r0 = g * RPW;
        intx4 v[RPW][NC];
#pragma unroll
        for (uint32_t r = 0; r < RPW; r++) {
            const uint64_t row = r0 + r < a.rows ? r0 + r : a.rows - 1u;
#pragma unroll
            for (uint32_t k = 0; k < NC; k++) v[r][k] = *reinterpret_cast<const intx4 *>(ant + row * row_bytes + off[k]);
        }
        int mine = 0;
#pragma unroll
        for (uint32_t r = 0; r < RPW; r++) {
            int acc = 0;
#pragma unroll
            for (uint32_t k = 0; k < NC; k++) {
                const int s = sum_of_squares(v[r][k]);
                acc += on[k] ? s : 0;
            }
            const int total = wave_sum(acc);
            mine = lane == r ? total : mine;
        }
        if (lane < RPW && r0 + lane < a.rows) a.block_power[r0 + lane] = (uint32_t)mine;
    }
}

template <uint32_t NC>
void launch_power(const bf_incoh_args &args, hipStream_t stream)
{
    bf_incoh_args a = args;
    a.n_groups = (a.rows + kLoads / NC - 1u) / (kLoads / NC);
    const uint64_t blocks = (a.n_groups + kWaves - 1u) / kWaves;
    hipLaunchKernelGGL(bf_incoherent_power_kernel<NC>, dim3((uint32_t)(blocks < kGrid ? blocks : kGrid)), dim3(kWaves * 64u), 0,
                       stream, a);
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_incoherent()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_incoherent_power_kernel<1>));
}

static hipError_t bf_launch_incoherent_power(const bf_incoh_args &a, hipStream_t stream)
{
    if (a.rows == 0u) return hipSuccess;
    if (a.A == 0u || a.A > 256u) return hipErrorInvalidValue;
    switch ((a.A + 31u) / 32u) {
    case 1: launch_power<1>(a, stream); break;
    case 2: launch_power<2>(a, stream); break;
    case 3: launch_power<3>(a, stream); break;
    case 4: launch_power<4>(a, stream); break;
    case 5: launch_power<5>(a, stream); break;
    case 6: launch_power<6>(a, stream); break;
    case 7: launch_power<7>(a, stream); break;
    default: launch_power<8>(a, stream); break;
    }
    return hipGetLastError();
}

// The host side of include/dcs_incoherent_beam.h, behind the table as in bf_integrate.hip.  No coefficients: no delay table,
// no terms, nothing allocated, and math_mode plays no part.
namespace bf_host {

int incoherent_block_power_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                uint32_t *d_block_power, size_t power_bytes, void *stream)
{
    if (int e = incoherent_block_power_args(c, nt, d_weights, d_block_power)) return e;
    if (nt && !d_antenna) return DCS_ERR_INVALID_ARGUMENT;
    DCS_CHECK_DEVICE(c);
    const uint32_t A = (uint32_t)c->p.nr_stations, C = (uint32_t)c->p.nr_channels;
    if (A > 256u) return DCS_ERR_UNSUPPORTED; // as the float call
    if (antenna_bytes < (size_t)A * C * nt * 2u) return DCS_ERR_INVALID_ARGUMENT;
    if (power_bytes < (size_t)C * (nt / 16u) * sizeof(uint32_t)) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_antenna, 16u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_incoh_args a;
    std::memset(&a, 0, sizeof(a));
    a.ant = d_antenna;
    a.weights = d_weights;
    a.block_power = d_block_power;
    a.rows = (uint64_t)C * (nt / 16u);
    a.A = A;
    return (int)bf_launch_incoherent_power(a, as_stream(stream));
}

int integrate_incoherent_power_impl(dcs_bf_context *c, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                    uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                    void *stream)
{
    if (int e = integrate_incoherent_power_args(c, d_block_power, nr_blocks, blocks_per_spectrum, d_spectra)) return e;
    return integrate_blocks(c, BF_INTEGRATE_U32, d_block_power, power_bytes, 1u, nr_blocks, blocks_per_spectrum, accumulate, d_spectra,
                            spectra_bytes, stream);
}

} // namespace bf_host
