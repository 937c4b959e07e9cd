/*
 * dcs_stream_staging.h -- staged delay tables for the streams of dcs_beamformer.h (BASELINE config 5): the next
 * tick's delay table lands WHILE the current tick runs -- what replaces the reference's blocking table copy before
 * each launch (BCT.cu:210).  A table that comes with its tick (dcs_bf_stream_tick*(..., new_table),
 * dcs_bf_stream_tick*_from_global) is copied or gathered in front of that tick's generator, on its critical path; a
 * staged one is not.
 *
 * Library: dc_sand_amd/csrc/libdcs_stream_staging.so, a companion of libdcs_beamformer.so built with it from the same
 * tree (`python -m dc_sand_amd.build`); it takes the dcs_bf_stream handles that library's dcs_bf_stream_begin returns.
 * libdcs_beamformer.so itself keeps its ABI version 3 and its entry points unchanged.  Status codes as dcs_beamformer.h.
 *
 * Fill the stream's staging buffer with the next delay table on an internal copy stream, overlapping whatever the
 * caller's stream is running.  The next tick that brings no table of its own (tick / tick_dt / tick_at with
 * new_table == NULL) makes it current: its stream waits on the copy's event (a device-side wait, never the host)
 * and its replay carries no copy or gather in front of the generator.  The rules:
 *   host memory: flags == 0 copies `table` into the stream's ring of four pinned buffers (the ring the host-table ticks
 *     use), so the caller's array is free again when the call returns; the host blocks only while four stagings are
 *     still in flight.  flags == DCS_BF_STAGE_CALLER_PINNED: `table` is pinned memory (dcs_host_alloc,
 *     pagelocked_empty), copied from where it is -- no host memcpy, no host wait -- and the caller keeps it unchanged
 *     until the consuming tick has run on its stream.  Any other flags: DCS_ERR_INVALID_ARGUMENT.
 *   buffers: the stream owns a third table buffer; the consuming tick exchanges it with the context's current one.
 *     The staging write into that buffer waits (on the internal stream) only for the work queued on the caller's stream
 *     before the LAST consuming tick -- never for the tick that runs now.  The internal stream is non-blocking (the
 *     null stream does not serialise it) and of the highest stream priority.
 *   consumption: a tick with new_table == NULL consumes the staged table.  While a table is staged, a tick that
 *     brings its own (new_table != NULL, any *_from_global tick) returns DCS_ERR_INVALID_ARGUMENT, enqueues nothing
 *     and leaves the staged table pending.  Staging twice before a tick: the last table staged wins.  A tick that
 *     fails its own checks (e.g. tick(t) with t out of range) consumes nothing.  The exchange happens only once the
 *     tick's replay is enqueued; if that fails the context still reads its previous table and the staged one stays
 *     pending.
 *   the context: generate*, upload_delays and set_delays_from_global between a staging call and its tick neither see
 *     nor race the staged table; from the consuming tick on they see it (as a table that comes with a tick).  Several
 *     streams on one context each keep their own staging state (the context's STREAM RULE still holds).
 *   capture: on a capturing caller stream both calls return DCS_ERR_UNSUPPORTED up front.
 *   teardown: dcs_bf_stream_end synchronises the caller's and the internal stream, destroys the internal stream and
 *     its events and frees exactly the buffer the stream holds then; a table staged but never consumed is dropped and
 *     the context keeps the table it had.  dcs_bf_stream_end does not touch the context, so either order of
 *     dcs_bf_stream_end and dcs_bf_destroy frees every buffer exactly once; no tick or staging call may follow
 *     dcs_bf_destroy of the stream's context.
 * The first staging call of a stream allocates its buffer, internal stream and events.  A stream made by a
 * libdcs_beamformer.so of another build returns DCS_ERR_UNSUPPORTED.
 */
#ifndef DCS_STREAM_STAGING_H
#define DCS_STREAM_STAGING_H

#include "dcs_beamformer.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define DCS_BF_STAGE_CALLER_PINNED 1

/* BCT.cu:210 (transfer_HtoD before each launch) */
int dcs_bf_stream_stage_table(dcs_bf_stream *s, const struct dcs_delay_vals *table, int flags);

/* The same from a device-resident GLOBAL table [nr_stations][nr_beams_total] (as dcs_bf_stream_tick_*_from_global;
 * 16-byte aligned, DCS_ERR_OUT_OF_RANGE when the slice runs past it): the bf_gather_beams kernel runs on the internal
 * stream after it has waited on ready_event (a hipEvent_t the producer, e.g. an RCCL broadcast, recorded; NULL = the
 * table is already complete).  The global table must stay unchanged until the gather has run (the consuming tick's
 * stream has waited for it). */
int dcs_bf_stream_stage_table_from_global(dcs_bf_stream *s, const void *d_global_table, uint32_t nr_beams_total,
                                          uint32_t beam_offset, void *ready_event);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DCS_STREAM_STAGING_H */
