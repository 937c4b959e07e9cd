"""Incoherent dedispersion on the GPU (include/dcs_dedisperse.h).  No tolerance anywhere: delays
and DM-time words are integers and are compared with the numpy model (helpers/dedisperse_model.py, anchored on the CPU by
tests/test_dedisperse_model.py).  Every buffer is exactly sized: the filterbanks' last row ends where their allocation
ends; every output has a 0xA5 canary behind it, which must stay untouched; the planes are prefilled, and every word outside
[first_out, first_out + nr_spectra) must stay as it was."""
from functools import partial

import numpy as np
import pytest

from helpers import dedisperse_paths as paths
from helpers import hip_graph
from helpers.dedisperse_cases import (ANY_SHAPE, CAPTURE_DM_SETS, CASES, CHAIN_BAND, DM_SETS, MASK_DMS, RAGGED_C, RAGGED_CASES, any_tables,
                                      capture_mask, some_mask, table_255)
from helpers.dedisperse_model import (BAND_ASCENDING_100, BAND_DESCENDING_64, DMS_40, INT32_MAX, INT32_MIN, dedisperse, dm_delays,
                                      smooth_table, takes_part)
from helpers.device_buffers import Context, closed_after
from helpers.examples import run_example
from helpers.filterbank_model import filterbank

pytestmark = pytest.mark.gpu

PREFILL = 0x3C
PREFILL_WORD = 0x3C3C3C3C


class DCase(Context):
    """One context of C channels (no delay table: the dedispersion has no coefficients; nr_beams is an argument) and the
    device buffers of its calls, exactly sized, outputs with a canary behind; all freed by close()."""

    def delays(self, band, dms):
        """dcs_bf_dm_delays on the device: the device table and its host copy."""
        from dc_sand_amd.generator import dm_delays_bytes

        dms = np.asarray(dms, dtype=np.float64)
        nbytes = dm_delays_bytes(self.bp, dms.size)
        assert nbytes == dms.size * self.C * 4
        d_dms, d_delays = self.upload(dms), self.out(nbytes)
        self.g.dm_delays(*band, d_dms, dms.size, d_delays, nbytes)
        self.gpu.synchronize()
        return d_delays, self.read(d_delays, nbytes, np.int32, (dms.size, self.C))

    def plane(self, fb, d_delays, nr_dm, first, T, max_delay, mask=None, out_spectra=None, first_out=0):
        """One dcs_bf_dedisperse_q8 call from a prefilled plane: the whole plane uint32 [B][nr_dm][out_spectra]."""
        from dc_sand_amd.generator import dm_time_bytes

        B, in_spectra, C = fb.shape
        assert C == self.C and fb.dtype == np.uint8
        out_spectra = first_out + T if out_spectra is None else out_spectra
        nbytes = dm_time_bytes(B, nr_dm, out_spectra)
        assert nbytes == B * nr_dm * out_spectra * 4
        d_fb = self.upload(fb)  # exactly fb.nbytes: the last row ends where the allocation ends
        d_mask = None if mask is None else self.upload(np.asarray(mask, dtype=np.uint8))
        d_out = self.out(nbytes, PREFILL)
        self.g.dedisperse_q8(d_fb, fb.nbytes, in_spectra, first, T, B, d_delays, nr_dm, max_delay, d_out, nbytes, out_spectra,
                             first_out=first_out, d_channel_mask=d_mask)
        self.gpu.synchronize()
        return self.read(d_out, nbytes, np.uint32, (B, nr_dm, out_spectra))

    def check(self, fb, table, first, T, max_delay, mask=None, out_spectra=None, first_out=0, d_delays=None):
        """The call against the model, from a host table (uploaded) or the device table d_delays that holds the same."""
        table = np.ascontiguousarray(table, dtype=np.int32)
        nr_dm = table.shape[0]
        out_spectra = first_out + T if out_spectra is None else out_spectra
        if d_delays is None:
            d_delays = self.upload(table)
        got = self.plane(fb, d_delays, nr_dm, first, T, max_delay, mask, out_spectra, first_out)
        pre = np.full((fb.shape[0], nr_dm, out_spectra), PREFILL_WORD, np.uint32)
        exp = dedisperse(fb, table, first, T, max_delay, mask, out=pre, first_out=first_out)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])
        return got


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(DCase, gpu))


def seeded_bytes(B, rows, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, rows, C), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- delays

DMS_EDGE = np.concatenate([DMS_40[:36], [np.nan, -12.5, 1e300, -1e300]])  # 40 DMs: 0, a NaN, negative ones, huge ones


@pytest.mark.parametrize("C", [1, 3, 64, 100])
def test_delays_are_the_model(gpu, case, C):
    c = case(C)
    bands = [BAND_DESCENDING_64, BAND_ASCENDING_100, (1400.0, 0.0, 64e-6), (600.0, -0.25, 1e-3)]
    for band in bands:
        _, got = c.delays(band, DMS_EDGE)
        exp = dm_delays(C, *band, DMS_EDGE)
        assert got.dtype == exp.dtype and np.array_equal(got, exp), (band, np.argwhere(got != exp)[:4])
        assert np.all(got[0] == 0) and np.all(got[36] == INT32_MAX)
        if C > 1 and band[1] != 0.0:
            assert (got == INT32_MAX).sum() >= 2 * (C - 1) and (got == INT32_MIN).sum() >= C - 1 and got.min() < 0 < got.max()
    # nothing to do: nothing is written
    from dc_sand_amd.generator import dm_delays_bytes

    d_dms, d_out = c.upload(DMS_40), c.out(dm_delays_bytes(c.bp, 4))
    c.g.dm_delays(*BAND_DESCENDING_64, d_dms, 0, d_out, 0)
    gpu.synchronize()
    assert np.all(c.read(d_out, 4 * C * 4, np.uint8, (-1,)) == 0xA5)


# ------------------------------------------------------------------------------------- planes with the tables dm_delays makes

@pytest.fixture(scope="module")
def band_tables():
    """The two bands' full tables from the model, shared."""
    return {64: dm_delays(64, *BAND_DESCENDING_64, DMS_40), 100: dm_delays(100, *BAND_ASCENDING_100, DMS_40)}


@pytest.mark.parametrize("C,band", [(64, BAND_DESCENDING_64), (100, BAND_ASCENDING_100)])
def test_planes_of_the_device_tables(gpu, case, band_tables, C, band):
    c = case(C)
    full = band_tables[C]
    assert 1300 <= full.max() <= 1340 and {int(r) for r in np.unique(full % 4)} == {0, 1, 2, 3}
    for T, B, nr_dm, first, first_out in CASES:
        d_delays, table = c.delays(band, DM_SETS[nr_dm])
        assert np.array_equal(table, dm_delays(C, *band, DM_SETS[nr_dm]))
        max_delay = int(table.max())
        fb = seeded_bytes(B, first + T + max_delay, C, seed=T + 7 * B + nr_dm)
        got = c.check(fb, table, first, T, max_delay, out_spectra=first_out + T + (3 if first_out else 0), first_out=first_out,
                      d_delays=d_delays)
        if T >= 63:
            assert np.unique(got[:, :, first_out:first_out + T]).size >= 30  # no trivial expectation
    # seven consecutive DMs: windows that differ by a few rows
    d_delays, table = c.delays(band, DMS_40[33:])
    fb = seeded_bytes(2, 6 + 700 + int(table.max()), C, seed=C)
    c.check(fb, table, 6, 700, int(table.max()), out_spectra=710, first_out=5, d_delays=d_delays)


@pytest.mark.parametrize("C", RAGGED_C)
def test_ragged_columns_with_smooth_tables(gpu, case, C):
    """Chunks that are no whole 32 columns and rows that start at any byte: C odd."""
    c = case(C)
    for nr_dm, top, T, B, first in RAGGED_CASES:
        table = smooth_table(C, nr_dm, top, seed=C + nr_dm)
        max_delay = int(table.max())
        fb = seeded_bytes(B, first + T + max_delay, C, seed=C * T)
        c.check(fb, table, first, T, max_delay, out_spectra=T + 9, first_out=5)


# ---------------------------------------------------------------------------------------------------------------- any table

def test_any_table_and_entries_that_drop(gpu, case):
    """Random entries in [0, 50000]: 6.4 MB of filterbanks that no LDS window holds.  Then the same table with entries
    outside [0, max_delay] sprinkled in, and a DM whose every term drops."""
    C, B, T, max_delay, nr_dm = ANY_SHAPE
    c = case(C)
    fb = seeded_bytes(B, T + max_delay, C, seed=1)
    assert fb.nbytes >= 6_400_000
    table, bad, smooth = any_tables()
    c.check(fb, table, 0, T, max_delay)
    assert takes_part(table, max_delay).all() and takes_part(bad, max_delay).sum() < table.size - C - 20
    got = c.check(fb, bad, 0, T, max_delay)
    assert not got[:, 5].any() and got[:, 4].all()
    # the same bad entries in a table that is staged: a smooth one
    got = c.check(fb, smooth, 0, T, max_delay)
    assert not got[:, 5].any()


# --------------------------------------------------------------------------------------------------------------------- mask

def test_channel_mask(gpu, case):
    C, B, T = 100, 2, 130
    c = case(C)
    table = dm_delays(C, *BAND_ASCENDING_100, MASK_DMS)
    max_delay = int(table.max())
    fb = seeded_bytes(B, T + max_delay, C, seed=2)
    plain = c.check(fb, table, 0, T, max_delay)
    ones = c.check(fb, table, 0, T, max_delay, mask=np.ones(C, np.uint8))
    assert np.array_equal(plain, ones)
    mask = some_mask(C)
    assert 10 < np.count_nonzero(mask) < C - 34
    some = c.check(fb, table, 0, T, max_delay, mask=mask)
    assert not np.array_equal(some, plain)
    none = c.check(fb, table, 0, T, max_delay, mask=np.zeros(C, np.uint8))
    assert not none.any()


# ------------------------------------------------------------------------------------------------------------ lane overflow

@pytest.mark.parametrize("C", [1030, 1024])
def test_every_byte_255(gpu, case, C):
    """258 columns is the smallest count at which a 16-bit lane can wrap: every word is 255 C."""
    T, B = 100, 1
    c = case(C)
    table = table_255(C)
    max_delay = int(table.max())
    assert max_delay == 300
    fb = np.full((B, T + max_delay, C), 0xFF, np.uint8)
    got = c.check(fb, table, 0, T, max_delay)
    assert np.all(got == 255 * C)


# ------------------------------------------------------------------------------------------------------------------ capture

def test_both_calls_captured_and_replayed_with_new_contents(gpu, case):
    """Both calls as first calls on a fresh context, captured; replayed after the DMs, the filterbank bytes and the mask
    were changed on the device: the outputs follow the new contents."""
    from dc_sand_amd.generator import dm_delays_bytes, dm_time_bytes

    C, B, T, nr_dm, first, first_out, out_spectra = 100, 2, 200, 7, 2, 3, 210
    band = BAND_ASCENDING_100
    dm_sets = CAPTURE_DM_SETS
    max_delay = max(int(dm_delays(C, *band, d).max()) for d in dm_sets)
    in_spectra = first + T + max_delay
    c = case(C)
    tbytes, pbytes = dm_delays_bytes(c.bp, nr_dm), dm_time_bytes(B, nr_dm, out_spectra)
    d_dms, d_fb, d_mask = c.alloc(nr_dm * 8), c.alloc(B * in_spectra * C), c.alloc(C)
    d_delays, d_out = c.out(tbytes), c.out(pbytes, PREFILL)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.g.dm_delays(*band, d_dms, nr_dm, d_delays, tbytes, stream=s.handle)
        c.g.dedisperse_q8(d_fb, B * in_spectra * C, in_spectra, first, T, B, d_delays, nr_dm, max_delay, d_out, pbytes, out_spectra,
                          first_out=first_out, d_channel_mask=d_mask, stream=s.handle)
    seen = []
    for i, dms in enumerate(dm_sets):
        fb = seeded_bytes(B, in_spectra, C, seed=60 + i)
        mask = capture_mask(i, C)
        gpu.memcpy_htod(d_dms, np.ascontiguousarray(dms), stream=s.handle, sync=False)
        gpu.memcpy_htod(d_fb, fb, stream=s.handle, sync=False)
        gpu.memcpy_htod(d_mask, mask, stream=s.handle, sync=False)
        gpu.memset(d_out, PREFILL, pbytes, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        table = dm_delays(C, *band, dms)
        assert np.array_equal(c.read(d_delays, tbytes, np.int32, (nr_dm, C)), table), i
        pre = np.full((B, nr_dm, out_spectra), PREFILL_WORD, np.uint32)
        exp = dedisperse(fb, table, first, T, max_delay, mask, out=pre, first_out=first_out)
        got = c.read(d_out, pbytes, np.uint32, (B, nr_dm, out_spectra))
        assert np.array_equal(got, exp), (i, np.argwhere(got != exp)[:3])
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    graph.close()


# --------------------------------------------------------------------------------- the staged / direct choice at its edges
#
# The kernel chooses per chunk, on the device, from the table's contents ("The choice").  The tables
# below come from helpers/dedisperse_paths.py, whose CPU model says which form every chunk takes; that they sit on the rule's
# edges -- the conditions a to i -- is asserted on that model in tests/test_dedisperse_paths.py, without a GPU.  Here the
# bar is the file's own: every word of the plane is the model's, the canary and the prefill are untouched.

KINDS = ("staged", "direct", "none")


def check_edge(c, table, mask, T, max_delay, seed, B=2, first=0, first_out=0, tail=0):
    """One call on B beams of seeded bytes, different per beam; no trivial expectation."""
    fb = seeded_bytes(B, first + T + max_delay, c.C, seed=seed)
    assert B < 2 or not np.array_equal(fb[0], fb[1])
    got = c.check(fb, table, first, T, max_delay, mask=mask, out_spectra=first_out + T + tail, first_out=first_out)
    assert np.unique(got[:, :, first_out:first_out + T]).size >= min(30, T)
    return got


@pytest.mark.parametrize("C", paths.EDGE_C)
@pytest.mark.parametrize("part", range(paths.EDGE_PARTS))
@pytest.mark.parametrize("nt", paths.EDGE_NT)
def test_chunks_at_the_edges_of_the_choice(gpu, case, nt, part, C):
    """Conditions a-e, h and i: spread 620 against 621 with the widest window last in LDS at residue 3; for every rounding
    of the pitch a chunk at rows = 2 pitch + 64 and one a row past it; in tiles of 512, 487 and 1 times; staged by dwords
    (C = 320) and by bytes with a last chunk of 29 columns (C = 317); a masked and a dead column in a staged edge chunk."""
    table, mask, T, max_delay = paths.edge_case(nt, part, C)
    kinds = {p.kind for p in paths.chunk_paths(table, T, max_delay, mask) if p.nt == nt}
    assert kinds == {"staged", "direct"}
    k = paths.EDGE_NT.index(nt) + part
    check_edge(case(C), table, mask, T, max_delay, seed=nt + part + C, first=(0, 3, 6)[k % 3], first_out=(0, 5)[k % 2], tail=k % 2 * 3)


@pytest.mark.parametrize("C", paths.ORDER_C)
def test_every_order_of_staged_direct_and_no_term(gpu, case, C):
    """Condition f: one workgroup walks chunks whose kinds follow each other in all nine orders; then two DM tiles and two
    time tiles whose workgroups take different forms at the same chunk."""
    c = case(C)
    table, mask, T, max_delay = paths.order_case(C)
    assert paths.orders(paths.chunk_paths(table, T, max_delay, mask)) == {(a, b) for a in KINDS for b in KINDS}
    check_edge(c, table, mask, T, max_delay, seed=C)
    table, mask, T, max_delay = paths.order_case_tiles(C)
    groups = paths.workgroups(paths.chunk_paths(table, T, max_delay, mask))
    assert len(groups) == 4 and any({g[i] for g in groups.values()} == set(KINDS) for i in range(10))
    check_edge(c, table, mask, T, max_delay, seed=C + 1, first=2, first_out=7, tail=2)


def test_dm_counts_at_the_waves_boundaries(gpu, case):
    """Condition g: tiles of 1, 4, 5, 8, 12, 13 and 16 DMs, alone and behind full tiles (nr_dm = 17 and 33 among them)."""
    c = case(paths.SWEEP_C)
    seen = set()
    for nr_dm in paths.SWEEP_NR_DM:
        table, mask, T, max_delay = paths.sweep_case(nr_dm)
        seen |= {p.nd for p in paths.chunk_paths(table, T, max_delay, mask)}
        got = check_edge(c, table, mask, T, max_delay, seed=nr_dm, first=nr_dm % 3, first_out=nr_dm % 2)
        assert got.shape[1] == nr_dm
    assert seen == {1, 4, 5, 8, 12, 13, 16}


def test_the_launch_is_one_kernel_of_the_tiles_the_model_assumes(gpu, case):
    """512 times x 16 DMs x one beam per workgroup of 256 threads, from the device side: the captured call is a single
    kernel node whose grid is ceil(T / 512) ceil(nr_dm / 16) B."""
    from dc_sand_amd.generator import dm_time_bytes

    C, B, T, nr_dm, max_delay = 64, 2, 1025, 33, 40
    c = case(C)
    d_fb = c.upload(seeded_bytes(B, T + max_delay, C, seed=5))
    d_delays = c.upload(smooth_table(C, nr_dm, max_delay, seed=5))
    pbytes = dm_time_bytes(B, nr_dm, T)
    d_out = c.out(pbytes, PREFILL)
    s = gpu.Stream()
    others = []
    nodes = hip_graph.launches(s, lambda: c.g.dedisperse_q8(d_fb, B * (T + max_delay) * C, T + max_delay, 0, T, B, d_delays, nr_dm, max_delay,
                                                            d_out, pbytes, T, stream=s.handle), others)
    s.synchronize()
    assert not others and nodes == [((3 * 3 * 2, 1, 1), (256, 1, 1))], (nodes, others)
    assert (paths.TILE_T, paths.TILE_D) == (512, 16) and (-(-T // 512), -(-nr_dm // 16)) == (3, 3)
    assert np.all(c.read(d_out, pbytes, np.uint8, (-1,)) == PREFILL)  # nothing ran


def test_a_replay_chooses_again_from_the_table_on_the_device(gpu, case):
    """Captured with a table whose chunks are staged; replayed after the table on the device was overwritten with one whose
    same chunks are direct, then with one where they have no term: the choice is made when the work runs."""
    from dc_sand_amd.generator import dm_time_bytes

    tables, T, max_delay = paths.replay_tables()
    C, B, nr_dm, first, first_out, out_spectra = paths.REPLAY_C, 2, 16, 1, 2, 520
    forms = [{p.kind for p in paths.chunk_paths(t, T, max_delay)} for t in tables]
    assert forms == [{"staged"}, {"direct"}, {"none"}]
    in_spectra = first + T + max_delay
    c = case(C)
    fb = seeded_bytes(B, in_spectra, C, seed=96)
    pbytes = dm_time_bytes(B, nr_dm, out_spectra)
    d_fb, d_delays, d_out = c.upload(fb), c.upload(tables[0]), c.out(pbytes, PREFILL)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.g.dedisperse_q8(d_fb, fb.nbytes, in_spectra, first, T, B, d_delays, nr_dm, max_delay, d_out, pbytes, out_spectra,
                          first_out=first_out, stream=s.handle)
    seen = []
    for i, table in enumerate(tables):
        gpu.memcpy_htod(d_delays, np.ascontiguousarray(table), stream=s.handle, sync=False)
        gpu.memset(d_out, PREFILL, pbytes, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        pre = np.full((B, nr_dm, out_spectra), PREFILL_WORD, np.uint32)
        exp = dedisperse(fb, table, first, T, max_delay, out=pre, first_out=first_out)
        got = c.read(d_out, pbytes, np.uint32, (B, nr_dm, out_spectra))
        assert np.array_equal(got, exp), (i, np.argwhere(got != exp)[:3])
        seen.append(got[:, :, first_out:first_out + T])
    assert np.unique(seen[0]).size >= 30 and np.unique(seen[1]).size >= 30 and not np.array_equal(seen[0], seen[1])
    assert not seen[2].any()
    graph.close()


def test_short_buffers_and_a_band_below_zero_are_refused_and_nothing_is_enqueued(gpu, case):
    """The refusals that need the context's C: they come after the version check, with DCS_ERR_INVALID_ARGUMENT."""
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError
    from dc_sand_amd.generator import dm_delays_bytes, dm_time_bytes

    C, B, T, nr_dm, max_delay = 64, 2, 50, 7, 30
    c = case(C)
    g = c.g
    in_spectra = T + max_delay
    fbytes, tbytes, pbytes = B * in_spectra * C, dm_delays_bytes(c.bp, nr_dm), dm_time_bytes(B, nr_dm, T)
    d_fb, d_dms = c.upload(seeded_bytes(B, in_spectra, C, seed=4)), c.upload(DMS_40[:nr_dm])
    d_delays, d_out = c.out(tbytes), c.out(pbytes, PREFILL)
    calls = [
        lambda: g.dm_delays(*BAND_DESCENDING_64, d_dms, nr_dm, d_delays, tbytes - 1),
        lambda: g.dm_delays(100.0, -10.0, 64e-6, d_dms, nr_dm, d_delays, tbytes),          # the last column at -530 MHz
        lambda: g.dm_delays(630.0, -10.0, 64e-6, d_dms, nr_dm, d_delays, tbytes),          # the last column at 0 MHz
        lambda: g.dedisperse_q8(d_fb, fbytes - 1, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, d_out, pbytes, T),
        lambda: g.dedisperse_q8(d_fb, fbytes, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, d_out, pbytes - 1, T),
        lambda: g.dedisperse_q8(d_fb, fbytes, in_spectra, 0, T, B + 1, d_delays, nr_dm, max_delay, d_out, pbytes, T),
        lambda: g.dedisperse_q8(d_fb, fbytes, in_spectra, 0, T, B, d_delays, nr_dm + 1, max_delay, d_out, pbytes, T),
        lambda: g.dedisperse_q8(d_fb, fbytes, in_spectra, 1, T, B, d_delays, nr_dm, max_delay, d_out, pbytes, T),
        lambda: g.dedisperse_q8(d_fb, fbytes, in_spectra, 0, T, B, d_delays, nr_dm, max_delay, d_out, pbytes, T, first_out=1),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    gpu.synchronize()
    assert np.all(c.read(d_delays, tbytes, np.uint8, (-1,)) == 0xA5) and np.all(c.read(d_out, pbytes, np.uint8, (-1,)) == PREFILL)
    # nothing to do: nothing is written, and the calls succeed
    g.dedisperse_q8(d_fb, fbytes, in_spectra, 0, 0, B, d_delays, nr_dm, max_delay, d_out, pbytes, T)
    g.dedisperse_q8(d_fb, fbytes, in_spectra, 0, T, B, d_delays, 0, max_delay, d_out, 0, T)
    gpu.synchronize()
    assert np.all(c.read(d_out, pbytes, np.uint8, (-1,)) == PREFILL)


# -------------------------------------------------------------------------------------------------------------------- chain

def test_filterbank_q8_descending_into_dedisperse(gpu, case):
    """Spectra whose channel c lies at f0 + c df, quantised with DCS_FB_DESCENDING: column j of the bytes is channel
    C - 1 - j, so the band is stated per column, first f0 + (C - 1) df and step -df.  The plane is the model of the chain."""
    from dc_sand_amd.generator import dm_time_bytes, filterbank_bytes, filterbank_scales_bytes

    C, B, nr_dm = 64, 3, 7
    f0, df, ts = CHAIN_BAND
    band = (f0 + (C - 1) * df, -df, ts)
    dms = DMS_40[33:]
    table = dm_delays(C, *band, dms)
    max_delay = int(table.max())
    assert table[-1, C - 1] == max_delay > 1000  # the last column is channel 0, the lowest frequency
    T = 300
    rows = T + max_delay
    rng = np.random.default_rng(11)
    m = np.exp2(rng.uniform(-8.0, 8.0, size=(C, B))).astype(np.float32)
    x = (m[None].astype(np.float64) * (1.0 + 0.25 * rng.standard_normal((rows, C, B)))).astype(np.float32)
    sc = np.stack([m, (24.0 / (0.25 * m.astype(np.float64))).astype(np.float32)], axis=-1)
    c = case(C)
    fbytes, pbytes = filterbank_bytes(c.bp, B, rows), dm_time_bytes(B, nr_dm, T)
    assert filterbank_scales_bytes(c.bp, B) == sc.nbytes
    d_x, d_sc, d_fb = c.upload(x), c.upload(sc), c.alloc(fbytes)
    d_dms, d_delays, d_out = c.upload(dms), c.out(table.nbytes), c.out(pbytes, PREFILL)
    c.g.filterbank_q8(d_x, x.nbytes, rows, B, d_sc, 128.0, d_fb, fbytes, rows, descending=True)
    c.g.dm_delays(*band, d_dms, nr_dm, d_delays, table.nbytes)
    c.g.dedisperse_q8(d_fb, fbytes, rows, 0, T, B, d_delays, nr_dm, max_delay, d_out, pbytes, T)
    gpu.synchronize()
    fb, _ = filterbank(x, sc, 128.0, descending=True)
    assert fb.shape == (B, rows, C) and np.unique(fb).size > 100
    exp = dedisperse(fb, table, 0, T, max_delay)
    got = c.read(d_out, pbytes, np.uint32, (B, nr_dm, T))
    assert np.array_equal(c.read(d_delays, table.nbytes, np.int32, table.shape), table)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:3]


# ------------------------------------------------------------------------------------------------------------------ example

def test_example_runs_and_verifies_itself(gpu):
    out = run_example("dedispersed_pulse.py", 64, 2, 24, 1024)
    assert "bit-identical to the model: True" in out and "the maximum lies at the injected DM and time: True" in out
