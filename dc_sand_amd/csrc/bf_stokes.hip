// bf_stokes.hip -- full-Stokes detection of dual-polarisation 8-bit voltage beams (include/dcs_stokes.h; DESIGN.md section
// 5.15), gfx950 only: the exact block Stokes parameters of two int8 beam tensors (bf_integrate.hip integrates them).
// The sibling of bf_incoherent.hip: the same kind of arithmetic -- every term an integer -- on two streams instead of one.
//
// The two tensors int8 [C][nt / 16][B][16][{re, im}] are the same flat sequence of N = C * (nt / 16) * B rows of 32 bytes,
// and a row pair reduces to NS = nr_stokes dwords.  Nothing depends on the antennas and no inner dimension is ragged; only
// the tail of N is.  The kernel is a stream of 16-byte loads bound by the HBM read rate (4 bytes in per beam and sample,
// 1 (IQUV) or 0.25 (I) out):
//
//  * a lane takes whole rows: two 16-byte loads from x and two from y per row, kRows = 2 rows at a time 64 rows apart, so
//    a wave's loads of one kind cover 2 KiB contiguous bytes between them and a lane has eight loads -- 128 bytes -- in
//    flight before the first use.  A wave carries 128 consecutive rows per trip, and eight waves per SIMD fit (the register
//    report is in DESIGN.md);
//  * a dword holds two samples (re, im, re', im').  v_dot4_i32_i8 of (x, x), (y, y) and (x, y) gives Pxx, Pyy and
//    Cr = sum xr yr + xi yi directly.  For Ci = sum xi yr - xr yi the bytes of x are permuted into (xi, 0, xi', 0) and
//    (0, xr, 0, xr') with v_perm_b32 (selector byte 0x0c gives a zero byte); two more dot4 against y give sum xi yr and
//    sum xr yi, and the two int32 sums are subtracted.  No byte is negated anywhere: -(-128) is no int8;
//  * no cross-lane step and no LDS: a row's NS sums end in the lane that loaded it.  IQUV is one 16-byte store per row, I
//    one dword per row with consecutive rows in consecutive lanes.  The kernel is a template on NS, so the I-only one has
//    neither the cross terms nor their stores.
//
// A trip that runs over the last row clamps the row to N - 1 for its loads (in bounds, a line the wave fetches anyway) and
// does not store it.  Byte offsets are 64-bit.  Nothing here rounds: -ffp-contract and the float flags of the build play
// no part.

#include "bf_host.h"

#include <hip/hip_runtime.h>

// Full-Stokes detection (include/dcs_stokes.h): two int8 beam tensors as
// rows = C * nT16 * B rows of 32 bytes each, every row pair reduced to nr_stokes exact dwords of block_stokes [C][nT16][B][nr_stokes]
struct bf_stokes_args {
    const int8_t *beams_x; // [rows][16][2], 16-byte aligned; polarisation x
    const int8_t *beams_y; // the same of polarisation y; may be beams_x
    int32_t *block_stokes; // [rows][nr_stokes], aligned to 4 * nr_stokes bytes
    uint64_t rows;
    uint64_t n_groups;     // filled by the launcher: groups of rows that a wave carries at once
    uint32_t nr_stokes;    // 1 (I) or 4 (I, Q, U, V)
};

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kRows = 2;    // rows a lane carries at once: 4 kRows 16-byte loads in flight
constexpr uint32_t kWaves = 4;   // waves per workgroup
constexpr uint32_t kGrid = 2048; // workgroups at most: 256 CUs x 8 workgroups = 8 waves per SIMD, each walking its share of the rows
constexpr uint32_t kWaveRows = kRows * 64u; // rows a wave carries per trip

constexpr uint32_t kSelImag = 0x0c030c01u; // (b1, 0, b3, 0) of a dword's bytes b0 .. b3: the imaginary parts, over y's real parts
constexpr uint32_t kSelReal = 0x020c000cu; // (0, b0, 0, b2): the real parts, over y's imaginary parts

struct row_sums {
    int pxx, pyy, cr, xiyr, xryi;
};

template <uint32_t NS>
__device__ __forceinline__ void dot_dword(row_sums &s, const int x, const int y)
{
    s.pxx = __builtin_amdgcn_sdot4(x, x, s.pxx, false);
    s.pyy = __builtin_amdgcn_sdot4(y, y, s.pyy, false);
    if (NS == 4u) {
        s.cr = __builtin_amdgcn_sdot4(x, y, s.cr, false);
        s.xiyr = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm((uint32_t)x, (uint32_t)x, kSelImag), y, s.xiyr, false);
        s.xryi = __builtin_amdgcn_sdot4((int)__builtin_amdgcn_perm((uint32_t)x, (uint32_t)x, kSelReal), y, s.xryi, false);
    }
}

template <uint32_t NS>
__device__ __forceinline__ void dot_unit(row_sums &s, const intx4 x, const intx4 y)
{
    dot_dword<NS>(s, x.x, y.x);
    dot_dword<NS>(s, x.y, y.y);
    dot_dword<NS>(s, x.z, y.z);
    dot_dword<NS>(s, x.w, y.w);
}

template <uint32_t NS> // nr_stokes: 1 (I) or 4 (I, Q, U, V)
__global__ void __launch_bounds__(kWaves * 64) bf_stokes_block_kernel(const bf_stokes_args a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const char *bx = reinterpret_cast<const char *>(a.beams_x);
    const char *by = reinterpret_cast<const char *>(a.beams_y);
    const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
    // the wave's number as a scalar: the trip's first row is then scalar arithmetic
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave; g < a.n_groups; g += nwaves) {
        const uint64_t r0 = g * kWaveRows + lane;
        intx4 x[kRows][2], y[kRows][2];
#pragma unroll
        for (uint32_t r = 0; r < kRows; r++) {
            const uint64_t row = r0 + r * 64u < a.rows ? r0 + r * 64u : a.rows - 1u;
            const intx4 *px = reinterpret_cast<const intx4 *>(bx + row * 32u);
            const intx4 *py = reinterpret_cast<const intx4 *>(by + row * 32u);
            x[r][0] = px[0];
            x[r][1] = px[1];
            y[r][0] = py[0];
            y[r][1] = py[1];
        }
#pragma unroll
        for (uint32_t r = 0; r < kRows; r++) {
            row_sums s = {0, 0, 0, 0, 0};
            dot_unit<NS>(s, x[r][0], y[r][0]);
            dot_unit<NS>(s, x[r][1], y[r][1]);
            const uint64_t row = r0 + r * 64u;
            if (row < a.rows) {
                if (NS == 4u) {
                    intx4 out;
                    out.x = s.pxx + s.pyy;
                    out.y = s.pxx - s.pyy;
                    out.z = 2 * s.cr;
                    out.w = 2 * (s.xiyr - s.xryi);
                    reinterpret_cast<intx4 *>(a.block_stokes)[row] = out;
                } else {
                    a.block_stokes[row] = s.pxx + s.pyy;
                }
            }
        }
    }
}

template <uint32_t NS>
void launch_block(const bf_stokes_args &args, hipStream_t stream)
{
    bf_stokes_args a = args;
    a.n_groups = (a.rows + kWaveRows - 1u) / kWaveRows;
    const uint64_t blocks = (a.n_groups + kWaves - 1u) / kWaves;
    hipLaunchKernelGGL(bf_stokes_block_kernel<NS>, dim3((uint32_t)(blocks < kGrid ? blocks : kGrid)), dim3(kWaves * 64u), 0, stream,
                       a);
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_stokes()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_stokes_block_kernel<4>));
}

static hipError_t bf_launch_stokes_block(const bf_stokes_args &a, hipStream_t stream)
{
    if (a.rows == 0u) return hipSuccess;
    switch (a.nr_stokes) {
    case 1: launch_block<1>(a, stream); break;
    case 4: launch_block<4>(a, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The host side of include/dcs_stokes.h, behind the table as in bf_integrate.hip.  No coefficients, nothing allocated, and
// math_mode plays no part.
namespace bf_host {

int stokes_block_impl(dcs_bf_context *c, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                      uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream)
{
    if (int e = stokes_block_args(c, nt, d_beams_x, d_beams_y, nr_stokes, d_block_stokes)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t B = (uint32_t)c->p.nr_beams, C = (uint32_t)c->p.nr_channels;
    if (!holds(beams_bytes, C, nt, B, 2u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(stokes_bytes, C, nt / 16u, B, (uint64_t)nr_stokes * sizeof(int32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_stokes_args a;
    std::memset(&a, 0, sizeof(a));
    a.beams_x = d_beams_x;
    a.beams_y = d_beams_y;
    a.block_stokes = d_block_stokes;
    a.rows = (uint64_t)C * (nt / 16u) * B;
    a.nr_stokes = nr_stokes;
    return (int)bf_launch_stokes_block(a, as_stream(stream));
}

int integrate_stokes_impl(dcs_bf_context *c, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                          uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                          size_t spectra_bytes, void *stream)
{
    if (int e = integrate_stokes_args(c, d_block_stokes, nr_blocks, blocks_per_spectrum, nr_stokes, d_spectra)) return e;
    return integrate_blocks(c, BF_INTEGRATE_I32, d_block_stokes, stokes_bytes, (uint64_t)(uint32_t)c->p.nr_beams * nr_stokes, nr_blocks,
                            blocks_per_spectrum, accumulate, d_spectra, spectra_bytes, stream);
}

} // namespace bf_host
