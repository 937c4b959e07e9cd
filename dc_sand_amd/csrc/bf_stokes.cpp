// bf_stokes.cpp -- include/dcs_stokes.h, the companion library libdcs_stokes.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_stokes.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  The checks that need no device are made here, before the table is read.

#include "../../include/dcs_stokes.h"

#include "bf_ctx_ext.h"

namespace {

bool aligned(const void *p, uintptr_t bytes) { return !(reinterpret_cast<uintptr_t>(p) & (bytes - 1u)); }

bool stokes_ok(uint32_t nr_stokes) { return nr_stokes == DCS_BF_STOKES_I || nr_stokes == DCS_BF_STOKES_IQUV; }

} // namespace

extern "C" {

int dcs_bf_stokes_block(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                        uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream)
{
    if (!ctx || !d_beams_x || !d_beams_y || !d_block_stokes || !stokes_ok(nr_stokes)) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_beams_x, 16u) || !aligned(d_beams_y, 16u) || !aligned(d_block_stokes, 4u * nr_stokes) || nt % 16u)
        return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->stokes_block(ctx, nt, d_beams_x, d_beams_y, beams_bytes, nr_stokes, d_block_stokes, stokes_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_integrate_stokes(dcs_bf_context *ctx, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                            uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                            size_t spectra_bytes, void *stream)
{
    if (!ctx || !d_block_stokes || !d_spectra || !stokes_ok(nr_stokes)) return DCS_ERR_INVALID_ARGUMENT;
    if (!aligned(d_block_stokes, 4u * nr_stokes) || !aligned(d_spectra, 4u * nr_stokes)) return DCS_ERR_INVALID_ARGUMENT;
    if (blocks_per_spectrum == 0u || nr_blocks % blocks_per_spectrum) return DCS_ERR_INVALID_ARGUMENT;
    const bf_ctx_ext_ops *ops = ops_of(ctx);
    return ops ? ops->integrate_stokes(ctx, d_block_stokes, stokes_bytes, nr_blocks, blocks_per_spectrum, nr_stokes, accumulate,
                                       d_spectra, spectra_bytes, stream)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
