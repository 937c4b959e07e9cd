// bf_stream_ext.h -- the internal contract between libdcs_beamformer.so and its companion libdcs_stream_staging.so
// (include/dcs_stream_staging.h).  Both are built from this tree together.  Every dcs_bf_stream begins with a
// bf_stream_ext_head whose table points at the product library's implementation of the staging calls; the companion
// only checks the table's version and forwards.  Not a public interface.
#ifndef BF_STREAM_EXT_H
#define BF_STREAM_EXT_H

#include <stdint.h>

#include "../../include/dcs_beamformer.h"

#define BF_STREAM_EXT_VERSION 1u

struct bf_stream_ext_ops {
    uint32_t version; // BF_STREAM_EXT_VERSION
    int (*stage_table)(dcs_bf_stream *s, const struct dcs_delay_vals *table, int flags);
    int (*stage_table_from_global)(dcs_bf_stream *s, const void *d_global_table, uint32_t nr_beams_total,
                                   uint32_t beam_offset, void *ready_event);
};

// the first member of struct dcs_bf_stream
struct bf_stream_ext_head {
    const bf_stream_ext_ops *ops;
};

#endif // BF_STREAM_EXT_H
