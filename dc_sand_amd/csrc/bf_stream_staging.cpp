// bf_stream_staging.cpp -- include/dcs_stream_staging.h, the companion library libdcs_stream_staging.so.  Host code
// only: the staging itself (internal stream, events, the copy or gather kernel) is libdcs_beamformer.so's, reached
// through the table at the head of every stream it makes (bf_stream_ext.h).

#include "../../include/dcs_stream_staging.h"

#include "bf_stream_ext.h"

namespace {

const bf_stream_ext_ops *ops_of(dcs_bf_stream *s)
{
    const bf_stream_ext_ops *ops = reinterpret_cast<const bf_stream_ext_head *>(s)->ops;
    return ops && ops->version == BF_STREAM_EXT_VERSION ? ops : nullptr;
}

} // namespace

extern "C" {

int dcs_bf_stream_stage_table(dcs_bf_stream *s, const dcs_delay_vals *table, int flags)
{
    if (!s || !table) return DCS_ERR_INVALID_ARGUMENT;
    if (flags != 0 && flags != DCS_BF_STAGE_CALLER_PINNED) return DCS_ERR_INVALID_ARGUMENT;
    const bf_stream_ext_ops *ops = ops_of(s);
    return ops ? ops->stage_table(s, table, flags) : DCS_ERR_UNSUPPORTED;
}

int dcs_bf_stream_stage_table_from_global(dcs_bf_stream *s, const void *d_global_table, uint32_t nr_beams_total,
                                          uint32_t beam_offset, void *ready_event)
{
    if (!s || !d_global_table) return DCS_ERR_INVALID_ARGUMENT;
    const bf_stream_ext_ops *ops = ops_of(s);
    return ops ? ops->stage_table_from_global(s, d_global_table, nr_beams_total, beam_offset, ready_event)
               : DCS_ERR_UNSUPPORTED;
}

} // extern "C"
