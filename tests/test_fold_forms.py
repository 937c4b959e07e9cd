"""The CPU model of the forms the pulsar folder's kernels take (helpers/fold_forms.py; DESIGN.md section 5.24, "The forms"):
its constants and rules against the kernel's source text, and a census of what the table of tests/test_gpu_fold.py presents to
the launcher (helpers/fold_cases.py; printed with pytest -s).  The bar: every form is run against the model with full and
with ragged tiles, with and without a tail of the unroll, with idle and with busy slices, and both sides of every boundary in
nbin between two forms are in the table at a band wide enough to show it."""
import re
from pathlib import Path

import numpy as np

from helpers import fold_cases as fc
from helpers import fold_forms as ff
from helpers import fold_model as fm

SOURCE = Path(__file__).resolve().parent.parent / "dc_sand_amd" / "csrc" / "bf_fold.hip"


def kernel_constants():
    return {name: int(value, 0) for name, value in re.findall(r"^constexpr uint32_t (k\w+) = (\w+?)u?;", SOURCE.read_text(), flags=re.M)}


def test_the_models_constants_and_rules_are_the_kernels():
    k = kernel_constants()
    assert (k["kThreads"], k["kTileWords"], k["kMaxWidth"], k["kMinWidth"], k["kRows"]) == \
        (ff.THREADS, ff.TILE_WORDS, ff.MAX_WIDTH, ff.MIN_WIDTH, ff.ROWS) == (1024, 16384, 256, 16, 8)
    assert (k["kHitsThreads"], k["kMaxBins"], k["kScrunchThreads"]) == (ff.HITS_THREADS, ff.MAX_BINS, ff.SCRUNCH_THREADS) == (256, 1024, 256)
    text = SOURCE.read_text()
    once = ["while ((kMaxWidth >> form) * nbin > kTileWords) form++;",
            "while ((kMaxWidth >> form) > kMinWidth && (kMaxWidth >> (form + 1u)) >= C) form++;",
            "const uint32_t W = kMaxWidth >> a.form, wmask = W - 1u, T = kThreads / W;",
            "a.tiles = (a.C - 1u) / W + 1u;",
            "const uint32_t chunk = (a.L + T - 1u) / T;",
            "if (W >= 64u)",
            "for (uint32_t k = k0; k < k1; k += kRows) {",
            "while (jw < a.nbin && jw < kScrunchThreads) jw <<= 1;",
            "__shared__ uint32_t s_tile[kTileWords];"]
    for line in once:
        assert text.count(line) == 1, line
    # no floating point and no atomic on global memory in the unit: the atomics are the three LDS adds
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", text))
    assert len(re.findall(r"atomicAdd\(&s_", text)) == len(re.findall(r"atomic", re.sub(r"//.*", "", text))) == 5


def test_the_model_on_shapes_worked_out_by_hand():
    assert [ff.nbin_form(n) for n in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert [ff.form_of(64, C) for C in (1, 16, 17, 32, 33, 64, 65, 128, 129, 317)] == [4, 4, 3, 3, 2, 2, 1, 1, 0, 0]
    assert ff.form_of(1024, 4096) == 4 and ff.form_of(300, 100) == 3 and ff.form_of(100, 100) == 1
    f = ff.fold_form(64, 317, 4096)
    assert (f.W, f.T, f.uniform, f.tiles, f.ragged, f.full, f.chunk, f.slices_on, f.tail) == (256, 4, True, 2, True, True, 1024, 4, False)
    f = ff.fold_form(1024, 3, 7)
    assert (f.W, f.T, f.uniform, f.tiles, f.ragged, f.full, f.chunk, f.slices_on, f.tail) == (16, 64, False, 1, True, False, 1, 7, True)
    f = ff.fold_form(257, 317, 513)
    assert (f.W, f.T, f.uniform, f.tiles, f.chunk, f.slices_on, f.tail) == (32, 32, False, 10, 17, 31, True)
    for form in ff.ALL_FORMS:  # the swizzled place of every word of a tile is its own
        W = ff.MAX_WIDTH >> form
        nbin = ff.TILE_WORDS // W
        at = {j * W + (c ^ (j & (W - 1))) for j in range(nbin) for c in range(W)}
        assert at == set(range(ff.TILE_WORDS))
    assert [ff.scrunch_form(n) for n in (1, 3, 64, 100, 256, 257, 1024)] == [(1, 256, 1), (4, 64, 1), (64, 4, 1), (128, 2, 1), (256, 1, 1),
                                                                            (256, 1, 2), (256, 1, 4)]


def test_every_form_is_run_against_the_model():
    c = ff.census(fc.census_calls())
    print("\n" + "\n".join(f"{k}: {sorted(v)}" for k, v in c.items()))
    every = set(ff.ALL_FORMS)
    assert c["forms"] == every and c["forms by nbin on a wide band"] == every
    for what in ("full", "ragged", "several tiles", "tail", "idle slices", "several trips"):
        assert c[what] == every, (what, sorted(every - c[what]))
    assert c["no tail"] >= {0, 1, 2} and c["every slice"] == every
    for b in ff.NBIN_BOUNDARIES:  # both sides of every boundary, at a band of at least 256 channels
        wide = {nbin for C, nbin, _ in fc.census_calls() if C >= ff.MAX_WIDTH}
        assert {b, b + 1} <= wide and ff.nbin_form(b) + 1 == ff.nbin_form(b + 1)
    assert c["nbin"] >= {1, 2, 3, 64, 100, 1024}


def test_the_table_is_what_the_tests_were_asked_to_run():
    rows = fc.all_cases()
    assert len(rows) == len(fc.CHANNELS) * len(fc.NBINS) and {r.C for r in rows} == {1, 3, 64, 100, 317}
    assert {r.L for r in rows} == {1, 7, 513, 4096} and {r.S for r in rows} == {1, 3}
    assert {(r.B, r.bpm) for r in rows} >= {(1, 1), (3, 1), (8, 4), (8, 1)} and {r.B for r in rows} >= {1, 3, 8}
    assert {r.model for r in rows} == set(fc.MODEL_KINDS) and {r.delays for r in rows} == {"none", "dm", "hand"}
    assert {r.hits for r in rows} == {True, False} and {r.first_subint for r in rows} == {0, 2} and {r.mask for r in rows} == {True, False}
    for C in fc.CHANNELS:  # every C meets every kind of model and of delay table
        assert {r.model for r in fc.cases()[C]} == set(fc.MODEL_KINDS) and {r.delays for r in fc.cases()[C]} == {"none", "dm", "hand"}
    assert max(r.B * r.S * r.L * r.C for r in rows) <= fc.LIMIT


def test_the_models_do_what_their_kinds_say():
    for r in fc.all_cases():
        m = fc.models_of(r, 1)
        P = r.B // r.bpm
        assert m.shape == (P, r.S)
        n = max(r.L, 400)
        b = fm.bins(m[0, 0], n, r.nbin)
        if r.model == "zero":
            assert len(set(b.tolist())) == 1
        elif r.model == "bin" and r.nbin > 1:
            d = np.diff(b[1:]) % r.nbin                         # from the wrap at k = 1 on a bin change every spectrum, but for the floor's remainder
            assert np.all(d <= 1) and d.mean() > 0.9
        elif r.model == "skip" and r.nbin >= 3:
            assert np.all((np.diff(b) % r.nbin) >= r.nbin // 2)  # bins are skipped
        elif r.model == "slow" and r.nbin > 1:
            runs = np.diff(np.flatnonzero(np.diff(b) != 0))
            assert runs.size and runs.min() >= 100
        # one step below a wrap: the phase at k = 1 is 0 (no accel term yet), and the last row starts at the last unit
        assert fm.phase_int(m[0, 0], 1) == 0 and (P * r.S == 1 or int(m[-1, -1]["phase0"]) == fc.TURN - 1)
    # step = 2^64 / nbin +- 1 crosses the edges one unit early or late: the bins differ from the exact step's somewhere
    for nbin in (3, 100, 1024):
        exact, late, early = (fm.bins(fm.model(0, fc.step_of(k, nbin)), 4096, nbin) for k in ("bin", "bin-1", "bin+1"))
        # (where nbin is no power of two the floor is itself below the edge, so the step above it is the one that differs)
        assert not np.array_equal(exact, early if nbin & (nbin - 1) else late)
    # both signs of accel change the run lengths over a sub-integration
    for kind in ("accel+", "accel-"):
        b = fm.bins(fm.model(0, fc.step_of(kind, 64), fc.accel_of(kind)), 4096, 64)
        assert not np.array_equal(b, fm.bins(fm.model(0, fc.step_of(kind, 64)), 4096, 64))


def test_hand_tables_hold_the_entries_that_fold_to_zero():
    for r in fc.all_cases():
        if r.delays != "hand":
            continue
        t = fc.hand_table(r, fc.HAND_MAX_DELAY, 3)
        assert t.dtype == np.int32 and t.shape == (r.B // r.bpm, r.C) and np.all(t[:, -1] == fc.HAND_MAX_DELAY)
        if r.C >= 64:
            for row in t:
                assert {-1, fc.INT32_MIN, fc.HAND_MAX_DELAY + 1, fc.INT32_MAX} <= set(row.tolist())
        on, _ = fm.columns_on(r.C, t[0], fc.HAND_MAX_DELAY, fc.mask_of(r, 4))
        assert on[-1] or r.mask
