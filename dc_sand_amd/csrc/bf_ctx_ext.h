// bf_ctx_ext.h -- the internal contract between libdcs_beamformer.so and its companions libdcs_beam_weights.so
// (include/dcs_beam_weights.h), libdcs_beam_quant.so (include/dcs_beam_quant.h), libdcs_beam_power.so
// (include/dcs_beam_power.h) and libdcs_incoherent_beam.so (include/dcs_incoherent_beam.h).  All are built from this tree
// together.  Every dcs_bf_context begins with a bf_ctx_ext_head whose table points at the product library's
// implementation of the weighted, the quantised and the detecting beamformer calls and of the incoherent beam; a companion checks the arguments it can check
// without a device, then the table's version, and forwards.  Not a public interface.
#ifndef BF_CTX_EXT_H
#define BF_CTX_EXT_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/dcs_beamformer.h"

// 2: beamform_accumulated_q8 appended; 3: beamform_accumulated_power, integrate_block_power appended; 5: incoherent_block_power,
// integrate_incoherent_power appended.  4 is skipped for good: tests/test_host_abi_beam_power.py hands the power companion a
// zeroed table whose version word is 4 and expects DCS_ERR_UNSUPPORTED -- at version 4 it would call a null pointer.
#define BF_CTX_EXT_VERSION 5u

struct bf_ctx_ext_ops {
    uint32_t version; // BF_CTX_EXT_VERSION
    // dt: nt fDeltaTime values, or nullptr for the times of samples t0 .. t0 + nt - 1
    int (*generate_and_beamform_weighted)(dcs_bf_context *c, const float *dt, uint64_t t0, uint32_t nt,
                                          const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                          float *d_beams, size_t beams_bytes, void *stream);
    // dt_coeff: the coefficients' fDeltaTime, or nullptr for that of sample t_coeff
    int (*beamform_accumulated_weighted)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                         const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                         float *d_beams, size_t beams_bytes, void *stream);
    // the same with int8 output (include/dcs_beam_quant.h); d_weights: nullptr = unweighted; d_clip_count: nullptr = no counting
    int (*beamform_accumulated_q8)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                   const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                   const float *d_quant_gains, int8_t *d_beams_q8, size_t beams_bytes,
                                   unsigned long long *d_clip_count, void *stream);
    // the same with detected block power out (include/dcs_beam_power.h): float [C][nt / 16][B]; d_weights: nullptr = unweighted
    int (*beamform_accumulated_power)(dcs_bf_context *c, const float *dt_coeff, uint64_t t_coeff, uint32_t nt,
                                      const int8_t *d_antenna, size_t antenna_bytes, const float *d_weights,
                                      float *d_block_power, size_t power_bytes, void *stream);
    // block powers [C][nr_blocks][B] -> spectra [nr_blocks / blocks_per_spectrum][C][B]
    int (*integrate_block_power)(dcs_bf_context *c, const float *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                 uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                 void *stream);
    // the incoherent beam (include/dcs_incoherent_beam.h): exact block powers uint32 [C][nt / 16] of the antennas that
    // d_weights ([A], nullptr = all) flags with a value != 0
    int (*incoherent_block_power)(dcs_bf_context *c, uint32_t nt, const int8_t *d_antenna, size_t antenna_bytes,
                                  const float *d_weights, uint32_t *d_block_power, size_t power_bytes, void *stream);
    // block powers [C][nr_blocks] -> spectra [nr_blocks / blocks_per_spectrum][C]
    int (*integrate_incoherent_power)(dcs_bf_context *c, const uint32_t *d_block_power, size_t power_bytes, uint32_t nr_blocks,
                                      uint32_t blocks_per_spectrum, uint32_t accumulate, float *d_spectra, size_t spectra_bytes,
                                      void *stream);
};

// the first member of struct dcs_bf_context
struct bf_ctx_ext_head {
    const bf_ctx_ext_ops *ops;
};

// a companion's way to the table, once its own checks have found c non-null: nullptr where the versions differ
static inline const bf_ctx_ext_ops *ops_of(dcs_bf_context *c)
{
    const bf_ctx_ext_ops *ops = reinterpret_cast<const bf_ctx_ext_head *>(c)->ops;
    return ops && ops->version == BF_CTX_EXT_VERSION ? ops : nullptr;
}

#endif // BF_CTX_EXT_H
