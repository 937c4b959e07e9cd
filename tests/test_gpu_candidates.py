"""The candidate sifter on the GPU (include/dcs_candidates.h).  No tolerance anywhere: the records
are compared with the numpy model (helpers/candidates_model.py, anchored on the CPU by tests/test_candidates_model.py) as
words -- integers and float bits -- and so are both count words.  Every buffer is exactly sized; the records and the counts
are prefilled with a non-zero pattern and have a 0xA5 canary behind them: a record beyond d_count[1] must stay as it was."""
from functools import lru_cache

import numpy as np
import pytest

from helpers import candidates_cases as cc
from helpers import hip_graph
from helpers.candidates_model import CANDIDATE, collapse, expected_buffer, find_candidates, same_bits, seeded_planes
from helpers.dedisperse_model import BAND_DESCENDING_64, DMS_40, dedisperse, dm_delays
from helpers.device_buffers import Context
from helpers.examples import run_example
from helpers.single_pulse_model import CHAIN, chain_filterbank, nr_blocks_of, peaks as model_peaks, snr as model_snr, sums as model_sums

pytestmark = pytest.mark.gpu

PREFILL = 0x3C
PREFILL_WORD = 0x3C3C3C3C


class CCase(Context):
    """One context (the sifter uses none of its parameters; nr_beams is an argument) and the device buffers of its calls,
    exactly sized, outputs with a canary behind; all freed by close()."""

    def __init__(self, gpu):
        super().__init__(gpu, 64)

    def out(self, nbytes):
        return super().out(nbytes, PREFILL)

    def find(self, snr, peaks, first_block, nr_blocks, threshold, radii, max_candidates=None, d_planes=None):
        """One dcs_bf_find_candidates call into prefilled records and counts, held to the model: the records of
        max_candidates (default: three more than are found) and both counts.  max_candidates == 0 passes a NULL d_cands.
        Returns (every record the model finds, the counts)."""
        from dc_sand_amd.generator import boxcar_peaks_bytes, candidates_bytes, candidates_workspace_bytes, peak_snr_bytes

        B, nr_dm, nw, pb = snr.shape
        rec, _ = find_candidates(snr, peaks, first_block, nr_blocks, threshold, *radii, 0)
        cap = len(rec) + 3 if max_candidates is None else max_candidates
        exp_count = np.array([len(rec), min(len(rec), cap)], np.uint32)
        sbytes, kbytes, cbytes = peak_snr_bytes(B, nr_dm, nw, pb), boxcar_peaks_bytes(B, nr_dm, nw, pb), candidates_bytes(cap)
        wbytes = candidates_workspace_bytes(B, nr_dm, nr_blocks)
        assert (sbytes, kbytes, cbytes) == (snr.nbytes, peaks.nbytes, 32 * cap)
        d_snr, d_peaks = d_planes if d_planes else (self.upload(snr), self.upload(peaks))
        d_cands, d_count, d_work = self.out(cbytes) if cap else None, self.out(8), self.out(wbytes)
        self.g.find_candidates(d_snr, sbytes, d_peaks, kbytes, pb, first_block, nr_blocks, B, nr_dm, nw, threshold, *radii, d_cands,
                               cbytes, cap, d_count, d_work, wbytes)
        self.gpu.synchronize()
        count = self.read(d_count, 8, np.uint32)
        assert count.tolist() == exp_count.tolist()
        self.read(d_work, wbytes, np.uint8)  # the canary behind the workspace
        if cap:
            prefill = np.zeros(cap, CANDIDATE)
            prefill.view(np.uint32)[:] = PREFILL_WORD
            got, exp = self.read(d_cands, cbytes, CANDIDATE), expected_buffer(rec, exp_count, prefill)
            bad = np.flatnonzero((got.view(np.uint32) != exp.view(np.uint32)).reshape(cap, 8).any(axis=1))
            assert bad.size == 0, (len(bad), bad[0], got[bad[0]], exp[bad[0]])
            assert same_bits(got, exp)
        return rec, count


@pytest.fixture
def case(gpu):
    c = CCase(gpu)
    yield c
    c.close()


@lru_cache(maxsize=None)
def ragged_planes(special=0.0):
    return seeded_planes(*cc.RAGGED, seed=21, special=special, step=1024)  # few ties: candidates in every tile, at every radius


def tiles_of(B, nr_dm, nr_blocks):
    from dc_sand_amd.generator import CANDIDATES_TILE_BLOCKS, CANDIDATES_TILE_DMS

    return B, -(-nr_dm // CANDIDATES_TILE_DMS), -(-nr_blocks // CANDIDATES_TILE_BLOCKS)


# -------------------------------------------------------------------------------------------------- ragged tiles, with offsets

@pytest.mark.parametrize("radii", [(0, 0), (1, 1), (8, 8), (8, 0), (0, 8)])
def test_ragged_tiles_on_both_axes_with_offsets(case, radii):
    from dc_sand_amd.generator import CANDIDATES_TILE_BLOCKS, CANDIDATES_TILE_DMS

    snr, peaks = ragged_planes()
    B, nr_dm, _, pb = snr.shape
    first_block, nr_blocks = 3, 131
    _, dm_tiles, k_tiles = tiles_of(B, nr_dm, nr_blocks)
    assert dm_tiles >= 2 and k_tiles >= 2 and nr_dm % CANDIDATES_TILE_DMS and nr_blocks % CANDIDATES_TILE_BLOCKS
    assert first_block and first_block + nr_blocks < pb  # blocks of the plane on both sides that are no cells of the call
    rec, count = case.find(snr, peaks, first_block, nr_blocks, 6.25, radii)
    assert count[0] > 20 and len(np.unique(rec["dm"] // CANDIDATES_TILE_DMS)) == dm_tiles
    assert len(np.unique((rec["block"] - first_block) // CANDIDATES_TILE_BLOCKS)) == k_tiles
    assert rec["block"].min() >= first_block and rec["block"].max() < first_block + nr_blocks


# ---------------------------------------------------------------------------------------- tile borders and halo corners: ties

def test_equal_maxima_across_tile_borders_and_halo_corners(case):
    """Pairs of equal maxima that straddle the border between two tiles of blocks, between two tiles of DMs, and both
    diagonals of the corner where four tiles meet: of each pair the lexicographically first cell is the candidate, for
    every radius that joins them, and both where the radius does not."""
    from dc_sand_amd.generator import CANDIDATES_TILE_BLOCKS as TK, CANDIDATES_TILE_DMS as TD

    first_block, nr_dm, nr_blocks = 5, 3 * TD - 2, 2 * TK + 30
    s = np.zeros((nr_dm, nr_blocks), np.float32)
    pairs = [((4, TK - 1), (4, TK)), ((TD - 1, 10), (TD, 10)), ((TD - 1, TK - 1), (TD, TK)), ((2 * TD - 1, TK), (2 * TD, TK - 1)),
             ((TD + 5, 2 * TK - 1), (TD + 5, 2 * TK)), ((2 * TD - 1, 2 * TK + 7), (2 * TD, 2 * TK + 7))]
    for n, (p, q) in enumerate(pairs):
        s[p] = s[q] = 20.0 + n
    # a plateau over the corner of four tiles, and maxima eight cells apart on both axes: the far corner of the halo
    s[2 * TD - 2:2 * TD + 2, TK - 20:TK - 16] = 9.0
    s[TD - 1, TK + 20], s[TD + 7, TK + 28], s[TD + 7, TK + 12] = 15.0, 15.0, 15.0
    snr = np.full((1, nr_dm, cc.BORDER_WIDTHS, first_block + nr_blocks + 1), -np.inf, np.float32)
    snr[0, :, 1, first_block:first_block + nr_blocks] = s
    peaks = seeded_planes(1, nr_dm, cc.BORDER_WIDTHS, snr.shape[3], seed=5)[1]
    d_planes = (case.upload(snr), case.upload(peaks))
    for radii in ((1, 1), (8, 8), (0, 1), (1, 0), (0, 0), (8, 7), (7, 8)):
        rec, _ = case.find(snr, peaks, first_block, nr_blocks, 5.0, radii, d_planes=d_planes)
        got = {(int(r["dm"]), int(r["block"]) - first_block) for r in rec}
        for p, q in pairs:
            joined = abs(p[0] - q[0]) <= radii[0] and abs(p[1] - q[1]) <= radii[1]
            assert p in got and (q in got) != joined, (radii, p, q)
        assert ((2 * TD - 2, TK - 20) in got) and (((2 * TD - 1, TK - 19) in got) == (radii == (0, 0)))
        assert (TD - 1, TK + 20) in got and ((TD + 7, TK + 28) in got) != (radii == (8, 8))
        assert ((TD + 7, TK + 12) in got) != (radii == (8, 8))
        assert np.all(rec["width_index"] == 1)


# ------------------------------------------------------------------------------------------------------- the scan's loop carries

def test_more_segments_than_two_rounds_of_the_scan(case):
    from dc_sand_amd.generator import CANDIDATES_SCAN_SPAN

    B, nr_dm, nw, nr_blocks = cc.SCAN
    _, dm_tiles, k_tiles = tiles_of(B, nr_dm, nr_blocks)
    tiles, segments = B * dm_tiles * k_tiles, B * nr_dm * k_tiles
    assert (dm_tiles, k_tiles) == (38, 18) and tiles == 1368 > 1024  # more tiles than the scan workgroup has lanes
    assert segments > 2 * CANDIDATES_SCAN_SPAN and segments % CANDIDATES_SCAN_SPAN  # three rounds and more, the last one short
    snr, peaks = seeded_planes(B, nr_dm, nw, nr_blocks, seed=33)
    rec, count = case.find(snr, peaks, 0, nr_blocks, 7.0, (1, 1))
    assert count[0] > 3 * CANDIDATES_SCAN_SPAN  # candidates in every round's segments
    per_round = np.bincount(((rec["beam"].astype(np.int64) * nr_dm + rec["dm"]) * k_tiles + rec["block"] // 64) // CANDIDATES_SCAN_SPAN)
    assert per_round.size == -(-segments // CANDIDATES_SCAN_SPAN) and per_round.min() > 0


# ----------------------------------------------------------------------------------------------------------- every cell, and none

def test_every_cell_a_candidate_and_none(case):
    snr, peaks = ragged_planes()
    B, nr_dm, _, _ = snr.shape
    d_planes = (case.upload(snr), case.upload(peaks))
    assert snr.min() > -100.0 and snr.max() < 1000.0
    rec, count = case.find(snr, peaks, 3, 131, -100.0, (0, 0), d_planes=d_planes)
    assert count.tolist() == [B * nr_dm * 131] * 2 and np.all(rec["members"] == 1)
    rec, count = case.find(snr, peaks, 3, 131, 1000.0, (0, 0), d_planes=d_planes)
    assert count.tolist() == [0, 0]
    rec, count = case.find(snr, peaks, 3, 131, 1000.0, (8, 8), max_candidates=4, d_planes=d_planes)
    assert count.tolist() == [0, 0]
    # every cell at or above threshold, and one plateau each beam: one candidate per beam, the window full of members
    flat = np.full((2, 20, 1, 70), 2.5, np.float32)
    rec, count = case.find(flat, seeded_planes(2, 20, 1, 70, seed=3)[1], 0, 70, 2.5, (8, 8))
    assert count[0] == 2 and rec["members"].tolist() == [81, 81] and rec["block"].tolist() == [0, 0]


# --------------------------------------------------------------------------------------------------------------------- overflow

def test_overflow_truncates_in_order(case):
    snr, peaks = ragged_planes()
    d_planes = (case.upload(snr), case.upload(peaks))
    rec, count = case.find(snr, peaks, 3, 131, 6.25, (1, 1), d_planes=d_planes)
    found = int(count[0])
    assert found > 10
    for cap in (0, 1, found - 1, found):
        _, count = case.find(snr, peaks, 3, 131, 6.25, (1, 1), max_candidates=cap, d_planes=d_planes)
        assert count.tolist() == [found, cap]


# ------------------------------------------------------------------------------------------------------------ non-finite planes

def test_non_finite_planes(case):
    snr, peaks = (a.copy() for a in ragged_planes(special=0.3))
    snr[0, 5] = -np.inf         # a DM without a width that takes part
    snr[1, 20, :, 40:90] = np.nan
    snr[1, 21, :, 40:90] = np.inf  # a plateau of +infinity
    assert np.isnan(snr).sum() > 1000 and np.isposinf(snr).sum() > 1000 and np.signbit(snr[snr == 0]).any()
    d_planes = (case.upload(snr), case.upload(peaks))
    for radii, threshold in (((1, 1), 0.0), ((0, 0), -5.0), ((8, 8), 3.0e38), ((2, 3), -3.0e38)):
        rec, count = case.find(snr, peaks, 3, 131, threshold, radii, d_planes=d_planes)
        assert count[0] > 0 and not np.isnan(rec["snr"]).any() and np.isposinf(rec["snr"]).any()
        assert not ((rec["beam"] == 0) & (rec["dm"] == 5)).any()
    # nr_widths == 0: every cell is -infinity
    none = np.zeros((2, 37, 0, 200), np.float32)
    rec, count = case.find(none, np.zeros(none.shape + (2,), np.uint32), 3, 131, -3.0e38, (1, 1), max_candidates=2)
    assert count.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------- every unrolled chain of widths

@pytest.mark.parametrize("nw", cc.FORM_NR_WIDTHS)
def test_every_width_of_every_unrolled_chain(case, nw):
    """Eight widths and more: the collapse takes them eight at a time, then four, then one by one (helpers/launch_forms.py,
    candidate_width_chain).  In every plane each width index is the winning one of some candidate, at both radii, and the
    hand-made cells hold equal maxima at two indices (the lower one wins), a NaN at one of such a pair, and -infinity in all
    widths but the last: helpers/candidates_cases.py, whose conditions tests/test_launch_forms.py asserts on the model; here
    they are asserted on the model's records before the device is called."""
    _, _, blocks = cc.FORM_SHAPE
    snr, peaks = cc.form_planes(nw)
    d_planes = (case.upload(snr), case.upload(peaks))
    for radii in cc.FORM_RADII:
        rec, _ = find_candidates(snr, peaks, 0, blocks, cc.FORM_THRESHOLD, *radii, 0)
        assert set(rec["width_index"].tolist()) == set(range(nw)), radii
        won = {(int(r["dm"]), int(r["block"])): int(r["width_index"]) for r in rec}
        assert all(won[cell] == winner for cell, (_, winner) in cc.hand_cells(nw).items()), radii
        got, count = case.find(snr, peaks, 0, blocks, cc.FORM_THRESHOLD, radii, d_planes=d_planes)
        assert count[0] == len(rec) >= nw + len(cc.hand_cells(nw))


# ------------------------------------------------------------------------------------------- width_index is peak_snr's d_best

def test_width_index_is_the_best_width_of_peak_snr(case, gpu):
    from dc_sand_amd.generator import best_width_bytes, peak_snr_bytes

    T, widths, max_width = 1500, np.array(cc.BEST_WIDTHS, np.uint32), 32
    plane = np.random.default_rng(44).integers(0, 1 << 20, size=(2, 19, T + max_width - 1), dtype=np.uint32)
    plane[1, 3] = 777  # a constant series: every width gives 0, the lowest index is the best
    pk, sm = model_peaks(plane, 0, T, widths, max_width, 64), model_sums(plane, 0, T)
    B, nr_dm, nw, pb, _ = pk.shape
    sbytes, bbytes = peak_snr_bytes(B, nr_dm, nw, pb), best_width_bytes(B, nr_dm, pb)
    d_peaks, d_snr, d_best = case.upload(pk), case.out(sbytes), case.out(bbytes)
    case.g.peak_snr(d_peaks, pk.nbytes, pb, 0, pb, B, nr_dm, case.upload(widths), nw, max_width, case.upload(sm), sm.nbytes, T, d_snr,
                    sbytes, d_best, bbytes)
    gpu.synchronize()
    snr = case.read(d_snr, sbytes, np.float32).reshape(B, nr_dm, nw, pb)
    best = case.read(d_best, bbytes, np.uint32).reshape(B, nr_dm, pb)
    rec, count = case.find(snr, pk, 0, pb, -3.0e38, (0, 0), d_planes=(d_snr, d_peaks))
    assert count[0] == B * nr_dm * pb and len(np.unique(rec["width_index"])) >= 3
    assert np.array_equal(rec["width_index"], best[rec["beam"], rec["dm"], rec["block"]])
    assert np.all(rec["width_index"][(rec["beam"] == 1) & (rec["dm"] == 3)] == 0)


# ------------------------------------------------------------------------------------------------------------------ refusals

def test_short_buffers_are_refused_and_nothing_is_enqueued(case, gpu):
    """The refusals that come after the version check."""
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DCS_ERR_UNSUPPORTED, DcsError
    from dc_sand_amd.generator import candidates_bytes, candidates_workspace_bytes

    (B, nr_dm, nw, pb), first_block, nr_blocks, cap = cc.SHORT, 2, 70, 6
    snr, peaks = seeded_planes(B, nr_dm, nw, pb, seed=50)
    sbytes, kbytes, cbytes, wbytes = snr.nbytes, peaks.nbytes, candidates_bytes(cap), candidates_workspace_bytes(B, nr_dm, nr_blocks)
    d_snr, d_peaks = case.upload(snr), case.upload(peaks)
    d_cands, d_count, d_work = case.out(cbytes), case.out(8), case.out(wbytes)
    g = case.g

    def find(snr_bytes=sbytes, peaks_bytes=kbytes, cands_bytes=cbytes, work_bytes=wbytes, beams=B, dms=nr_dm, widths=nw, blocks=nr_blocks,
             first=first_block, peak_blocks=pb, max_candidates=cap):
        return g.find_candidates(d_snr, snr_bytes, d_peaks, peaks_bytes, peak_blocks, first, blocks, beams, dms, widths, 6.0, 1, 1,
                                 d_cands, cands_bytes, max_candidates, d_count, d_work, work_bytes)

    calls = [
        (lambda: find(snr_bytes=sbytes - 1), DCS_ERR_INVALID_ARGUMENT), (lambda: find(peaks_bytes=kbytes - 1), DCS_ERR_INVALID_ARGUMENT),
        (lambda: find(cands_bytes=cbytes - 1), DCS_ERR_INVALID_ARGUMENT), (lambda: find(work_bytes=wbytes - 1), DCS_ERR_INVALID_ARGUMENT),
        (lambda: find(work_bytes=0), DCS_ERR_INVALID_ARGUMENT), (lambda: find(max_candidates=cap + 1), DCS_ERR_INVALID_ARGUMENT),
        (lambda: find(beams=B + 1), DCS_ERR_INVALID_ARGUMENT), (lambda: find(dms=nr_dm + 1), DCS_ERR_INVALID_ARGUMENT),
        (lambda: find(widths=nw + 1), DCS_ERR_INVALID_ARGUMENT),
        (lambda: find(beams=B, dms=nr_dm + 1, snr_bytes=2**40, peaks_bytes=2**40), DCS_ERR_INVALID_ARGUMENT),  # the workspace
        # 2^32 cells and more, and a block past 2^32: the counts and the records' block are 32-bit words
        (lambda: find(beams=2**16, dms=2**16, blocks=1, snr_bytes=2**62, peaks_bytes=2**62, work_bytes=2**62), DCS_ERR_UNSUPPORTED),
        (lambda: find(first=2**32 - 1, blocks=2, peak_blocks=2**33, snr_bytes=2**62, peaks_bytes=2**62), DCS_ERR_UNSUPPORTED),
    ]
    for i, (call, status) in enumerate(calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == status, i
    gpu.synchronize()
    for d, n in ((d_cands, cbytes), (d_count, 8), (d_work, wbytes)):
        assert np.all(case.read(d, n, np.uint8) == PREFILL)
    # nothing to do: only the counts are written, as zeros
    for kw in (dict(blocks=0), dict(dms=0, work_bytes=0), dict(blocks=0, first=pb, work_bytes=0, snr_bytes=0, peaks_bytes=0, widths=0)):
        gpu.memset(d_count, PREFILL, 8)
        find(**kw)
        gpu.synchronize()
        assert case.read(d_count, 8, np.uint32).tolist() == [0, 0], kw
    assert np.all(case.read(d_cands, cbytes, np.uint8) == PREFILL) and np.all(case.read(d_work, wbytes, np.uint8) == PREFILL)


# ------------------------------------------------------------------------------------------------------------------ capture

def test_captured_on_first_use_and_replayed_with_new_contents(case, gpu):
    """The first call of a fresh context, captured; replayed after the planes were changed on the device: the list and
    both counts follow the new contents, a different number of candidates each time, one of them more than fit."""
    from dc_sand_amd.generator import candidates_bytes, candidates_workspace_bytes

    (B, nr_dm, nw, pb), first_block, nr_blocks, cap = cc.CAPTURE, 3, 131, 1000
    c = case
    snr0, peaks0 = seeded_planes(B, nr_dm, nw, pb, seed=60)
    sbytes, kbytes, cbytes, wbytes = snr0.nbytes, peaks0.nbytes, candidates_bytes(cap), candidates_workspace_bytes(B, nr_dm, nr_blocks)
    d_snr, d_peaks = c.alloc(sbytes), c.alloc(kbytes)
    d_cands, d_count, d_work = c.out(cbytes), c.out(8), c.out(wbytes)
    s = gpu.Stream()
    others = []
    nodes = hip_graph.launches(s, lambda: c.g.find_candidates(d_snr, sbytes, d_peaks, kbytes, pb, first_block, nr_blocks, B, nr_dm, nw,
                                                               9.5, 2, 2, d_cands, cbytes, cap, d_count, d_work, wbytes,
                                                               stream=s.handle), others)
    tiles = int(np.prod(tiles_of(B, nr_dm, nr_blocks)))
    assert [g for g, _ in nodes] == [(tiles, 1, 1), (1, 1, 1), (tiles, 1, 1)] and not others  # three kernels, nothing else
    with hip_graph.capture(s) as graph:
        c.g.find_candidates(d_snr, sbytes, d_peaks, kbytes, pb, first_block, nr_blocks, B, nr_dm, nw, 9.5, 2, 2, d_cands, cbytes, cap,
                            d_count, d_work, wbytes, stream=s.handle)
    prefill = np.zeros(cap, CANDIDATE)
    prefill.view(np.uint32)[:] = PREFILL_WORD
    seen = []
    for i in range(3):
        snr, peaks = seeded_planes(B, nr_dm, nw, pb, seed=60 + i, plateau=i != 1)
        if i == 2:
            snr[:] = -1.0
            snr[:, ::3, :, ::3] = 10.0  # a lattice of maxima wider apart than the radii: more candidates than fit
        gpu.memcpy_htod(d_snr, snr, stream=s.handle, sync=False)
        gpu.memcpy_htod(d_peaks, peaks, stream=s.handle, sync=False)
        gpu.memset(d_cands, PREFILL, cbytes, stream=s.handle)
        gpu.memset(d_count, PREFILL, 8, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        rec, exp_count = find_candidates(snr, peaks, first_block, nr_blocks, 9.5, 2, 2, cap)
        assert c.read(d_count, 8, np.uint32).tolist() == exp_count.tolist(), i
        assert same_bits(c.read(d_cands, cbytes, CANDIDATE), expected_buffer(rec, exp_count, prefill)), i
        seen.append(exp_count.tolist())
    assert len({tuple(x) for x in seen}) == 3 and seen[2][0] > cap == seen[2][1] and 0 < seen[0][0] < cap
    graph.close()


# -------------------------------------------------------------------------------------------------------------------- chain

def test_the_chain_ends_in_one_record_for_the_injected_pulse(case, gpu):
    """The chain of tests/test_gpu_single_pulse.py -- noise bytes with a pulse of 8 spectra along the track of DM index 20 ->
    dm_delays -> dedisperse_q8 -> sums, peaks, signal-to-noise -- and the sifter behind it: one record, at the pulse's DM,
    block, width and time.  (The figures are those of tests/test_single_pulse_model.py: the pulse is above 23, nothing
    outside DMs 18 to 22 is above 9.3.)"""
    from dc_sand_amd.generator import (boxcar_peaks_bytes, candidates_bytes, candidates_workspace_bytes, dm_delays_bytes, dm_time_bytes,
                                       dm_time_sums_bytes, peak_snr_bytes)

    k = CHAIN
    C, outputs, widths, max_width, block_len = k["C"], k["outputs"], np.array(k["widths"], np.uint32), k["max_width"], k["block_len"]
    table = dm_delays(C, *BAND_DESCENDING_64, DMS_40)
    nr_dm, max_delay = table.shape[0], int(table.max())
    fb = chain_filterbank(table, seed=0)
    rows, T = fb.shape[1], outputs - max_width + 1
    nb = nr_blocks_of(T, block_len)
    tbytes, pbytes, sbytes = dm_delays_bytes(case.bp, nr_dm), dm_time_bytes(1, nr_dm, outputs), dm_time_sums_bytes(1, nr_dm)
    kbytes, nbytes = boxcar_peaks_bytes(1, nr_dm, widths.size, nb), peak_snr_bytes(1, nr_dm, widths.size, nb)
    cap, wbytes = 8, candidates_workspace_bytes(1, nr_dm, nb)
    d_fb, d_dms, d_widths = case.upload(fb), case.upload(DMS_40), case.upload(widths)
    d_delays, d_plane, d_sums = case.out(tbytes), case.out(pbytes), case.out(sbytes)
    d_peaks, d_snr = case.out(kbytes), case.out(nbytes)
    d_cands, d_count, d_work = case.out(candidates_bytes(cap)), case.out(8), case.out(wbytes)
    g = case.g
    g.dm_delays(*BAND_DESCENDING_64, d_dms, nr_dm, d_delays, tbytes)
    g.dedisperse_q8(d_fb, fb.nbytes, rows, 0, outputs, 1, d_delays, nr_dm, max_delay, d_plane, pbytes, outputs)
    g.dm_time_sums(d_plane, pbytes, outputs, 0, k["count"], 1, nr_dm, d_sums, sbytes)
    g.boxcar_peaks(d_plane, pbytes, outputs, 0, T, 1, nr_dm, d_widths, widths.size, max_width, block_len, d_peaks, kbytes, nb)
    g.peak_snr(d_peaks, kbytes, nb, 0, nb, 1, nr_dm, d_widths, widths.size, max_width, d_sums, sbytes, k["count"], d_snr, nbytes)
    g.find_candidates(d_snr, nbytes, d_peaks, kbytes, nb, 0, nb, 1, nr_dm, widths.size, 10.0, 8, 1, d_cands, candidates_bytes(cap), cap,
                      d_count, d_work, wbytes)
    gpu.synchronize()
    plane = dedisperse(fb, table, 0, outputs, max_delay)
    exp_peaks = model_peaks(plane, 0, T, widths, max_width, block_len)
    exp_snr, _ = model_snr(exp_peaks, widths, max_width, model_sums(plane, 0, k["count"]), k["count"])
    rec, count = find_candidates(exp_snr, exp_peaks, 0, nb, 10.0, 8, 1, cap)
    assert case.read(d_count, 8, np.uint32).tolist() == count.tolist() == [1, 1]
    got = case.read(d_cands, candidates_bytes(cap), CANDIDATE)
    assert same_bits(got[:1], rec) and np.all(got[1:].view(np.uint32) == PREFILL_WORD)
    r = got[0]
    assert (r["beam"], r["dm"], r["block"], r["width_index"], r["time"]) == (0, k["dm_index"], 1, 3, k["row"])
    assert r["snr"] > 23.0 and r["members"] >= 3


# ------------------------------------------------------------------------------------------------------------------ example

def test_example_runs_and_verifies_itself(gpu):
    out = run_example("candidate_list.py", 64, 2, 32, 2048)
    assert "bit-identical to the model: True" in out and "two candidates at the injected pulses: True" in out
