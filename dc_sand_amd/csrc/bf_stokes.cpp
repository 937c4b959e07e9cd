// bf_stokes.cpp -- include/dcs_stokes.h, the companion library libdcs_stokes.so.  Host code only: the kernels are
// libdcs_beamformer.so's (bf_stokes.hip, bf_integrate.hip), reached through the table at the head of every context it makes
// (bf_ctx_ext.h).  Each export makes its entry's device-free checks (bf_arg_checks.h), then forwards.

#include "../../include/dcs_stokes.h"

#include "bf_ctx_ext.h"

extern "C" {

int dcs_bf_stokes_block(dcs_bf_context *ctx, uint32_t nt, const int8_t *d_beams_x, const int8_t *d_beams_y, size_t beams_bytes,
                        uint32_t nr_stokes, int32_t *d_block_stokes, size_t stokes_bytes, void *stream)
{
    if (int e = stokes_block_args(ctx, nt, d_beams_x, d_beams_y, nr_stokes, d_block_stokes)) return e;
    return forward(ctx, &bf_ctx_ext_ops::stokes_block, nt, d_beams_x, d_beams_y, beams_bytes, nr_stokes, d_block_stokes, stokes_bytes,
                   stream);
}

int dcs_bf_integrate_stokes(dcs_bf_context *ctx, const int32_t *d_block_stokes, size_t stokes_bytes, uint32_t nr_blocks,
                            uint32_t blocks_per_spectrum, uint32_t nr_stokes, uint32_t accumulate, float *d_spectra,
                            size_t spectra_bytes, void *stream)
{
    if (int e = integrate_stokes_args(ctx, d_block_stokes, nr_blocks, blocks_per_spectrum, nr_stokes, d_spectra)) return e;
    return forward(ctx, &bf_ctx_ext_ops::integrate_stokes, d_block_stokes, stokes_bytes, nr_blocks, blocks_per_spectrum, nr_stokes,
                   accumulate, d_spectra, spectra_bytes, stream);
}

} // extern "C"
