// bf_dedisperse.hip -- incoherent dedispersion of the 8-bit search filterbanks (include/dcs_dedisperse.h; DESIGN.md section
// 5.16), gfx950 only: the delay table of a band and a list of DMs, and the DM-time planes of any delay table.  Every term of
// a plane is a byte and every sum an exact integer, so nothing here depends on an order of summation.
//
// bf_dedisperse_kernel.  A workgroup of four waves owns one beam, kTileT = 512 consecutive output times and kTileD = 16
// consecutive DMs, and walks the columns in chunks of kChunk = 32:
//
//  * a wave owns ONE DM at a time (four of the tile's, one after the other) and a lane 8 consecutive times of it.  The
//    delay of a (DM, column) is then the same in every lane: it comes out of a register with v_readlane_b32, and the dword
//    address and the byte shift of the unaligned read are scalar arithmetic.  The accumulators of the wave's four DMs are 32
//    registers, indexed by unrolled loops only;
//  * per chunk every lane holds two of the tile's 16 x 32 table entries, loaded under the sums of the chunk before, -1
//    where the term drops (outside [0, max_delay], column masked or past C, DM past nr_dm).  Through LDS and five cross-lane
//    steps they give [lo, hi] per column, the rows that the chunk's windows span together and the widest window.  If every
//    window 512 + hi - lo fits the pitch that kWinBytes allow, and the spanned rows are not many more than one window, the
//    chunk is STAGED: the rows of the chunk are read from global memory once -- 4 rows x 4 columns per lane as four dwords
//    where C % 4 == 0, kBatch such units in flight per lane, transposed in registers with 8 v_perm_b32 and written as four
//    dwords; byte by byte for a ragged C -- into LDS as [column][time], with a pitch whose dword count is odd, so the byte
//    form's column-strided writes fall into different banks, the dword form's are 2-way at the most, and the reads, 64 lanes
//    x 8 contiguous bytes, have no conflict at all.  Each input byte then comes from L2/HBM once per 16 DMs;
//  * otherwise the chunk takes the DIRECT form, which reads every term from global memory.  The choice is made on the
//    device, because the table lives there, and is the same in every lane of the workgroup (every wave reduces the same 32
//    columns);
//  * per (DM, column) a lane reads the three aligned dwords that cover its 8 bytes, and per 4 bytes two v_perm_b32 with a
//    scalar selector take the even and the odd bytes at the wave's byte shift into two 16-bit lanes each; v_add3_u32 adds
//    two columns at once: 8 VALU instructions per column, one lane-operation per byte added.  The loop has no branch: a
//    term that drops reads kZero zero bytes kept in front of the windows.  A 16-bit lane holds at most 32 terms of 255
//    before it is flushed into the 32-bit accumulators at the end of the chunk (it could hold 257);
//  * the outputs are plain dword stores, and every offset into the filterbanks and the planes is 64-bit.
//
// Reads stay inside the rows [first, first + T + max_delay) of a beam whatever the table holds: an entry that takes part is
// at most max_delay, a staged window ends at hi + (the tile's times), and the direct form reads only for times below T.

#include "bf_host.h"

#include <hip/hip_runtime.h>

// Incoherent dedispersion (include/dcs_dedisperse.h).
// The delay table int32 [nr_dm][C] of a band and DMs, in fp64 rounded once per operation
struct bf_dmdelay_args {
    const double *dms; // [nr_dm], 8-byte aligned; read when the work runs
    int32_t *delays;   // [nr_dm][C]
    uint64_t total;    // nr_dm * C
    uint32_t C;
    double freq_first, freq_step, sample_time;
};
// Filterbanks uint8 [B][in_spectra][C] shifted by the table and summed over the columns into out uint32 [B][nr_dm][out_spectra],
// words first_out .. first_out + T - 1 of every series
struct bf_dedisp_args {
    const uint8_t *in;     // 16-byte aligned
    const int32_t *delays; // [nr_dm][C]; read when the work runs; an entry outside [0, max_delay] drops its term
    const uint8_t *mask;   // nullptr (every column), or [C]: a zero byte drops the column
    uint32_t *out;
    uint64_t in_spectra, first, out_spectra, first_out;
    uint32_t C, B, T, nr_dm, max_delay;
    uint32_t t_tiles, dm_tiles; // filled by the launcher: tiles of output times and of DMs
};

namespace {

constexpr uint32_t kThreads = 256;                       // four waves
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kDmPerWave = 4;                       // DMs a wave carries, one after the other
constexpr uint32_t kTileD = kWaves * kDmPerWave;         // 16 DMs per workgroup
constexpr uint32_t kTimesPerLane = 8;
constexpr uint32_t kTileT = 64u * kTimesPerLane;         // 512 output times per workgroup
constexpr uint32_t kChunk = 32;                          // columns per chunk
constexpr uint32_t kWinBytes = 36u << 10;                // LDS for the windows: with the 2.8 KiB beside them four workgroups per CU
constexpr uint32_t kMaxPitch = kWinBytes / kChunk;       // 1152 bytes of one column's window
constexpr uint32_t kZero = 528;                          // zero bytes in front of the windows: 8 * 63 + 12 are read from any start
constexpr uint32_t kBatch = 4;                           // units of 4 rows x 4 columns a lane loads before it transposes the first
constexpr uint32_t kSlack = 16;                          // window bytes beyond 512 + hi - lo: alignment of the start (3), of
                                                         // the rows staged four at a time (3) and of the last dword read (3)

static_assert(kThreads / kChunk * 2u == kTileD, "a lane holds two of a chunk's kTileD x kChunk table entries");
static_assert(kChunk == 32u && kChunk % 8u == 0u, "a chunk's read positions fill half a wave's lanes of one register");
static_assert(kZero >= kTimesPerLane * 63u + 12u && kZero % 16u == 0u && kZero / 4u <= kThreads, "the zeros a dropped term reads");
static_assert(kChunk * 255u <= 0xffffu, "a 16-bit lane takes a chunk's terms before it is flushed");

// bytes b0 b1 b2 b3 of four dwords w0 .. w3 -> the four dwords (w0.bk, w1.bk, w2.bk, w3.bk), k = 0 .. 3
__device__ __forceinline__ void transpose4(const uint32_t w[4], uint32_t out[4])
{
    const uint32_t a = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u); // w0.b0 w1.b0 w0.b1 w1.b1
    const uint32_t b = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u); // w0.b2 w1.b2 w0.b3 w1.b3
    const uint32_t c = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);
    const uint32_t d = __builtin_amdgcn_perm(w[3], w[2], 0x07030602u);
    out[0] = __builtin_amdgcn_perm(c, a, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(d, b, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(d, b, 0x07060302u);
}

__global__ void __launch_bounds__(kThreads) bf_dedisperse_kernel(const bf_dedisp_args a)
{
    // kZero zero bytes, which a term that drops reads, then [column][time], pitch bytes per column
    __shared__ __attribute__((aligned(16))) uint8_t s_img[kZero + kWinBytes];
    __shared__ int32_t s_off[kTileD][kChunk];      // first the entries that take part (-1: the term drops), then where to read
    __shared__ int32_t s_lo[kChunk], s_hi[kChunk]; // lo > hi: no DM of the tile takes the column

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t j = tid & (kChunk - 1u), m0 = tid / kChunk; // this lane's column of a chunk and its two DMs, m0 and m0 + 8
    // DM tiles fastest: the workgroups that run together read the same rows
    uint32_t blk = blockIdx.x;
    const uint32_t dm0 = (blk % a.dm_tiles) * kTileD;
    blk /= a.dm_tiles;
    const uint32_t t0 = (blk % a.t_tiles) * kTileT;
    const uint32_t beam = blk / a.t_tiles;
    const uint32_t nt = a.T - t0 < kTileT ? a.T - t0 : kTileT; // the tile's times
    const uint32_t nd = a.nr_dm - dm0 < kTileD ? a.nr_dm - dm0 : kTileD;
    // row 0 of this tile: time t0 of the beam's window, at delay 0
    const uint8_t *in0 = a.in + ((size_t)beam * a.in_spectra + a.first + t0) * (size_t)a.C;
    uint8_t *s_win = s_img + kZero;
    const uint32_t *s_img32 = reinterpret_cast<const uint32_t *>(s_img);

    // the table entry of (DM m of the tile, column c) if the term takes part, else -1
    auto entry = [&](uint32_t c, uint32_t m) -> int32_t {
        if (c >= a.C || m >= nd || (a.mask && !a.mask[c])) return -1;
        const int32_t d = a.delays[(size_t)(dm0 + m) * a.C + c];
        return d >= 0 && (uint32_t)d <= a.max_delay ? d : -1;
    };

    if (tid < kZero / 4u) reinterpret_cast<uint32_t *>(s_img)[tid] = 0u;
    uint32_t acc[kDmPerWave][kTimesPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kDmPerWave; k++)
#pragma unroll
        for (uint32_t i = 0; i < kTimesPerLane; i++) acc[k][i] = 0u;

    int32_t d0 = entry(j, m0), d1 = entry(j, m0 + kTileD / 2u);
    for (uint32_t c0 = 0; c0 < a.C; c0 += kChunk) {
        const uint32_t cc = a.C - c0 < kChunk ? a.C - c0 : kChunk;
        __syncthreads(); // the chunk before is read out
        s_off[m0][j] = d0;
        s_off[m0 + kTileD / 2u][j] = d1;
        __syncthreads();
        // [lo, hi] of this lane's column over the tile's DMs
        int32_t lo = 0x7fffffff, hi = -1;
#pragma unroll
        for (uint32_t m = 0; m < kTileD; m++) {
            const int32_t d = s_off[m][j];
            if (d >= 0) {
                lo = d < lo ? d : lo;
                hi = d > hi ? d : hi;
            }
        }
        // over the chunk's columns (lanes l and l + 32 hold the same column): the rows [rlo, rhi + nt) that the windows
        // span, and the widest window.  Every wave gets the same three values
        int32_t rlo = lo, rhi = hi;
        uint32_t spread = lo <= hi ? (uint32_t)(hi - lo) : 0u;
#pragma unroll
        for (int x = 1; x < (int)kChunk; x <<= 1) {
            const int32_t olo = __shfl_xor(rlo, x), ohi = __shfl_xor(rhi, x);
            const uint32_t os = (uint32_t)__shfl_xor((int)spread, x);
            rlo = olo < rlo ? olo : rlo;
            rhi = ohi > rhi ? ohi : rhi;
            spread = os > spread ? os : spread;
        }
        // as scalars: the inner loop's addresses and selectors are then scalar arithmetic
        rlo = __builtin_amdgcn_readfirstlane(rlo);
        rhi = __builtin_amdgcn_readfirstlane(rhi);
        spread = (uint32_t)__builtin_amdgcn_readfirstlane((int)spread);
        uint32_t pitch = (kTileT + spread + kSlack) & ~3u; // spread < 2^31: no overflow
        pitch |= 4u;                                       // an odd number of dwords
        const uint32_t rows = (uint32_t)(rhi - rlo) + nt;  // <= max_delay + T: inside the beam's window
        const bool staged = spread <= kMaxPitch - kTileT - kSlack - 4u && rows <= 2u * pitch + 64u;
        if (rhi >= 0) { // else no term in this chunk; the same in every lane of the workgroup
            if (tid < kChunk) {
                s_lo[j] = lo;
                s_hi[j] = hi;
            }
            // where the inner loop reads: the window of column j starts at row wl = lo - ((lo - rlo) & 3) >= rlo, so that the
            // rows rlo + 4 g fall on its dwords; a term that drops reads the zeros (staged) or nothing (direct)
            const int32_t wl = lo - ((lo - rlo) & 3);
            const int32_t base = (int32_t)(kZero + j * pitch) - wl;
            const int32_t f0 = !staged ? d0 : d0 >= 0 ? base + d0 : 0;
            const int32_t f1 = !staged ? d1 : d1 >= 0 ? base + d1 : 0;
            __syncthreads(); // every lane has read the entries
            s_off[m0][j] = f0;
            s_off[m0 + kTileD / 2u][j] = f1;
            if (staged) {
                if ((a.C & 3u) == 0u) {
                    // 4 rows x 4 columns per lane: the row starts are 4-byte aligned (C % 4 == 0, c0 % 32 == 0, the base 16);
                    // kBatch such units' loads are in flight before the first is transposed
                    const uint32_t quads = cc / 4u, units = ((rows + 3u) / 4u) * quads; // cc % 4 == 0 here
                    for (uint32_t u0 = tid; u0 < units; u0 += kBatch * kThreads) {
                        uint32_t w[kBatch][4];
#pragma unroll
                        for (uint32_t b = 0; b < kBatch; b++) {
                            const uint32_t u = u0 + b * kThreads, g = u / quads, q = u % quads;
#pragma unroll
                            for (uint32_t r = 0; r < 4u; r++) {
                                const uint32_t row = 4u * g + r; // rows at or past `rows` are not read: they may lie outside the window
                                w[b][r] = u < units && row < rows
                                              ? *reinterpret_cast<const uint32_t *>(in0 + ((size_t)(uint32_t)rlo + row) * a.C + c0 + 4u * q)
                                              : 0u;
                            }
                        }
#pragma unroll
                        for (uint32_t b = 0; b < kBatch; b++) {
                            const uint32_t u = u0 + b * kThreads, g = u / quads, q = u % quads;
                            if (u >= units) break;
                            uint32_t o[4];
                            transpose4(w[b], o);
#pragma unroll
                            for (uint32_t k = 0; k < 4u; k++) {
                                const uint32_t col = 4u * q + k;
                                const int32_t clo = s_lo[col];
                                if (clo > s_hi[col]) continue;
                                // row rlo + 4 g at byte rlo + 4 g - wl of the window: a multiple of 4
                                const int32_t at = rlo + (int32_t)(4u * g) - (clo - ((clo - rlo) & 3));
                                if (at >= 0 && (uint32_t)at + 4u <= pitch)
                                    *reinterpret_cast<uint32_t *>(s_win + col * pitch + (uint32_t)at) = o[k];
                            }
                        }
                    }
                } else {
                    for (uint32_t u = tid; u < rows * cc; u += kThreads) {
                        const uint32_t row = u / cc, col = u % cc;
                        const int32_t clo = s_lo[col];
                        if (clo > s_hi[col]) continue;
                        const int32_t at = rlo + (int32_t)row - (clo - ((clo - rlo) & 3));
                        if (at >= 0 && (uint32_t)at < pitch)
                            s_win[col * pitch + (uint32_t)at] = in0[((size_t)(uint32_t)rlo + row) * a.C + c0 + col];
                    }
                }
            }
        }
        // the next chunk's entries: their way from global memory lies under this chunk's sums
        const int32_t n0 = entry(c0 + kChunk + j, m0), n1 = entry(c0 + kChunk + j, m0 + kTileD / 2u);
        if (rhi >= 0) {
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kDmPerWave; k++) {
                const uint32_t m = wave * kDmPerWave + k;
                if (m >= nd) break; // the same in the whole wave
                uint32_t e0 = 0u, o0 = 0u, e1 = 0u, o1 = 0u; // times (0, 2), (1, 3), (4, 6), (5, 7) as 2 x u16
                // the chunk's 32 read positions of this DM in the lanes of one register, read out with v_readlane_b32
                const int32_t offs = s_off[m][j];
                if (staged) {
#pragma unroll 8
                    for (uint32_t col = 0; col < kChunk; col++) {
                        const uint32_t at = (uint32_t)__builtin_amdgcn_readlane(offs, (int)col);
                        // bytes sh, sh + 2 and sh + 1, sh + 3 of a dword pair at the byte shift sh, each over a zero byte
                        const uint32_t sel_e = 0x0c020c00u + (at & 3u) * 0x10001u, sel_o = sel_e + 0x00010001u;
                        const uint32_t *p = s_img32 + (at >> 2) + 2u * lane;
                        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
                        e0 += __builtin_amdgcn_perm(w1, w0, sel_e);
                        o0 += __builtin_amdgcn_perm(w1, w0, sel_o);
                        e1 += __builtin_amdgcn_perm(w2, w1, sel_e);
                        o1 += __builtin_amdgcn_perm(w2, w1, sel_o);
                    }
                } else {
                    for (uint32_t col = 0; col < cc; col++) {
                        const int32_t off = __builtin_amdgcn_readlane(offs, (int)col);
                        if (off < 0) continue;
                        const uint8_t *p = in0 + ((size_t)(uint32_t)off + kTimesPerLane * lane) * a.C + c0 + col;
                        uint32_t v[kTimesPerLane];
#pragma unroll
                        for (uint32_t i = 0; i < kTimesPerLane; i++) v[i] = kTimesPerLane * lane + i < nt ? p[(size_t)i * a.C] : 0u;
                        e0 += v[0] | (v[2] << 16);
                        o0 += v[1] | (v[3] << 16);
                        e1 += v[4] | (v[6] << 16);
                        o1 += v[5] | (v[7] << 16);
                    }
                }
                acc[k][0] += e0 & 0xffffu;
                acc[k][1] += o0 & 0xffffu;
                acc[k][2] += e0 >> 16;
                acc[k][3] += o0 >> 16;
                acc[k][4] += e1 & 0xffffu;
                acc[k][5] += o1 & 0xffffu;
                acc[k][6] += e1 >> 16;
                acc[k][7] += o1 >> 16;
            }
        }
        d0 = n0;
        d1 = n1;
    }
#pragma unroll
    for (uint32_t k = 0; k < kDmPerWave; k++) {
        const uint32_t m = wave * kDmPerWave + k;
        if (m >= nd) break;
        uint32_t *o = a.out + ((size_t)beam * a.nr_dm + dm0 + m) * a.out_spectra + a.first_out + t0;
#pragma unroll
        for (uint32_t i = 0; i < kTimesPerLane; i++) {
            const uint32_t t = kTimesPerLane * lane + i;
            if (t < nt) o[t] = acc[k][i];
        }
    }
}

// One lane per (DM, column).  fp64, every operation rounded once: the build has -ffp-contract=off, and the divides are the
// correctly rounded ones (as bf_filterbank.hip's scales rely on).
__global__ void __launch_bounds__(256) bf_dm_delays_kernel(const bf_dmdelay_args a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; // m * C + j
    if (g >= a.total) return;
    const uint32_t j = (uint32_t)(g % a.C);
    const double dm = a.dms[g / a.C];
    const double f = a.freq_first + (double)j * a.freq_step;
    const double f_ref = a.freq_step <= 0.0 ? a.freq_first : a.freq_first + (double)(a.C - 1u) * a.freq_step;
    const double aj = 1.0 / (f * f), b = 1.0 / (f_ref * f_ref);
    const double s = ((4.148808e3 * dm) * (aj - b)) / a.sample_time;
    int32_t d;
    if (s != s || s > 2147483647.0) d = 0x7fffffff;
    else if (s < -2147483648.0) d = (int32_t)0x80000000u;
    else d = (int32_t)rint(s);
    a.delays[g] = d;
}

} // namespace

// This translation unit is a code object of its own: load it when the context is created, so that a first call -- which may
// be under stream capture -- only launches.
hipError_t bf_warm_module_dedisperse()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&bf_dedisperse_kernel));
}

static hipError_t bf_launch_dm_delays(const bf_dmdelay_args &a, hipStream_t stream)
{
    if (a.total == 0u) return hipSuccess;
    const uint64_t blocks = (a.total + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_dm_delays_kernel, dim3((uint32_t)blocks), dim3(256u), 0, stream, a);
    return hipGetLastError();
}

static hipError_t bf_launch_dedisperse(const bf_dedisp_args &args, hipStream_t stream)
{
    if (args.T == 0u || args.nr_dm == 0u || args.B == 0u) return hipSuccess;
    bf_dedisp_args a = args;
    a.t_tiles = (a.T - 1u) / kTileT + 1u;
    a.dm_tiles = (a.nr_dm - 1u) / kTileD + 1u;
    const uint64_t blocks = (uint64_t)a.t_tiles * a.dm_tiles * a.B;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_dedisperse_kernel, dim3((uint32_t)blocks), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

// The host side of include/dcs_dedisperse.h, behind the table as in bf_integrate.hip.  No coefficients, nothing allocated, and
// math_mode plays no part; the band is host memory and travels by value in the kernel's arguments.
namespace bf_host {

int dm_delays_impl(dcs_bf_context *c, const dcs_bf_band *band, const double *d_dms, uint32_t nr_dm, int32_t *d_delays,
                   size_t delays_bytes, void *stream)
{
    if (int e = dm_delays_args(c, band, d_dms, d_delays)) return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    const double f_last = band->freq_first_mhz + (double)(C - 1u) * band->freq_step_mhz; // the kernel's own f_(C-1)
    if (!(f_last > 0.0) || !std::isfinite(f_last)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(delays_bytes, nr_dm, C, sizeof(int32_t), 1u)) return DCS_ERR_INVALID_ARGUMENT;
    bf_dmdelay_args a;
    std::memset(&a, 0, sizeof(a));
    a.dms = d_dms;
    a.delays = d_delays;
    a.total = (uint64_t)nr_dm * C;
    a.C = C;
    a.freq_first = band->freq_first_mhz;
    a.freq_step = band->freq_step_mhz;
    a.sample_time = band->sample_time_s;
    return (int)bf_launch_dm_delays(a, as_stream(stream));
}

int dedisperse_q8_impl(dcs_bf_context *c, const uint8_t *d_filterbank, size_t filterbank_bytes, uint64_t in_spectra,
                       uint64_t first_spectrum, uint32_t nr_spectra, uint32_t nr_beams, const int32_t *d_delays, uint32_t nr_dm,
                       uint32_t max_delay, const uint8_t *d_channel_mask, uint32_t *d_dm_time, size_t dm_time_bytes,
                       uint64_t out_spectra, uint64_t first_out, void *stream)
{
    if (int e = dedisperse_q8_args(c, d_filterbank, in_spectra, first_spectrum, nr_spectra, nr_beams, d_delays, max_delay, d_dm_time,
                                   out_spectra, first_out))
        return e;
    DCS_CHECK_DEVICE(c);
    const uint32_t C = (uint32_t)c->p.nr_channels;
    if (!holds(filterbank_bytes, nr_beams, in_spectra, C, 1u)) return DCS_ERR_INVALID_ARGUMENT;
    if (!holds(dm_time_bytes, nr_beams, nr_dm, out_spectra, sizeof(uint32_t))) return DCS_ERR_INVALID_ARGUMENT;
    bf_dedisp_args a;
    std::memset(&a, 0, sizeof(a));
    a.in = d_filterbank;
    a.delays = d_delays;
    a.mask = d_channel_mask;
    a.out = d_dm_time;
    a.in_spectra = in_spectra;
    a.first = first_spectrum;
    a.out_spectra = out_spectra;
    a.first_out = first_out;
    a.C = C;
    a.B = nr_beams;
    a.T = nr_spectra;
    a.nr_dm = nr_dm;
    a.max_delay = max_delay;
    return (int)bf_launch_dedisperse(a, as_stream(stream));
}

} // namespace bf_host
