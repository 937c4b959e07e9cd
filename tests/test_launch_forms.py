"""The CPU model of the forms that five kernels and the integrator take (helpers/launch_forms.py; DESIGN.md, "The forms" of
sections 5.11, 5.17 to 5.20 and 5.22): its rules against the kernels' source text, worked cases, a census of what the older
tables of the GPU tests present to the launchers (helpers/*_cases.py; printed with pytest -s), and the bar: every form that
can exist is run against its model by the tables as they are now.  The conditions that the new GPU cases rely on -- every
width index wins somewhere, every wave of the boxcar kernel takes several pairs, a reordered float sum differs -- are asserted
here on the numpy models alone: if a builder misses one, the builder is wrong."""
from pathlib import Path

import numpy as np

from helpers import candidates_cases as cc
from helpers import correlator_cases as kc
from helpers import ddc_cases as dc
from helpers import incoherent_cases as ic
from helpers import integrate_cases as gc
from helpers import launch_forms as lf
from helpers import single_pulse_cases as sc
from helpers.candidates_model import collapse, find_candidates

CSRC = Path(__file__).resolve().parent.parent / "dc_sand_amd" / "csrc"


def text_of(name):
    return (CSRC / name).read_text()


# ------------------------------------------------------------------------------------------------- rules held to the source

ONCE = {
    "bf_correlator.hip": [
        "constexpr uint32_t kS = 4;", "constexpr uint32_t kSB = 2;", "constexpr uint32_t kWaves = 4;",
        "constexpr uint32_t kGrid = 1u << 20;",
        "a.tiles = (a.A + 15u) / 16u;",
        "a.st = (a.tiles + kS - 1u) / kS;",
        "a.units = a.st + a.st * (a.st - 1u) / 2u * (kS / kSB);",
        "a.items = (uint64_t)a.C * a.nr_vis * a.units;",
        "const uint64_t blocks = (a.items + kWaves - 1u) / kWaves;",
        "const uint32_t grid = ((uint32_t)(blocks < kGrid ? blocks : kGrid) + 7u) & ~7u;",
        "for (uint64_t item = (uint64_t)wg * kWaves + wave; item < a.items; item += nwaves) {",
        "const uint32_t u = (uint32_t)(item % a.units);",
        "if (u < a.st) {",
        "switch (a.tiles - u * kS) {",
        "const uint32_t v = u - a.st, w = v / (kS / kSB);",
        "while (sa * (sa + 1u) / 2u <= w) sa++;",
        "switch (a.tiles - sa * kS) {",
    ] + [f"case {n}: correlate_unit<{d}, {n}>(a, cv, {at}); break;" for d, at in (("true", "u, u * kS"), ("false", "sa, bt0")) for n in (1, 2, 3)]
      + [f"default: correlate_unit<{d}, 4>(a, cv, {at}); break;" for d, at in (("true", "u, u * kS"), ("false", "sa, bt0"))],
    "bf_incoherent.hip": [
        "constexpr uint32_t kLoads = 8;", "constexpr uint32_t kWaves = 4;", "constexpr uint32_t kGrid = 2048;",
        "switch ((a.A + 31u) / 32u) {",
        "constexpr uint32_t RPW = kLoads / NC;",
        "a.n_groups = (a.rows + kLoads / NC - 1u) / (kLoads / NC);",
        "default: launch_power<8>(a, stream); break;",
    ] + [f"case {n}: launch_power<{n}>(a, stream); break;" for n in range(1, 8)],
    "bf_candidates.hip": [
        "for (; i + 8u <= a.nr_widths; i += 8u) take_widths<8>(p, pitch, i, s, best);",
        "if (i + 4u <= a.nr_widths) {",
        "take_widths<4>(p, pitch, i, s, best);",
        "for (; i < a.nr_widths; i++) take_widths<1>(p, pitch, i, s, best);",
        "if (v[j] > s) { // false for a NaN",
    ],
    "bf_single_pulse.hip": [
        "constexpr uint32_t kSegment = 4096;", "constexpr uint32_t kBatch = 8;", "constexpr uint32_t kThreads = 256;",
        "constexpr uint32_t kWaves = kThreads / 64u;",
        "a.run = kSegment / a.block_len;",
        "const uint32_t nb = (nt + a.block_len - 1u) / a.block_len;",
        "const uint32_t batches = (a.nr_widths - 1u) / kBatch + 1u;",
        "uint32_t batch = wave / nb, kb = wave % nb;",
        "while (batch < batches) {",
        "uint32_t next_batch = batch, next_kb = kb + kWaves;",
        "for (; next_kb >= nb; next_kb -= nb) next_batch++;",
    ],
    "bf_ddc.hip": [
        "constexpr uint32_t kGrid = 1u << 20;",
        "constexpr uint32_t kSpanOut = kWaves * kTilesPerWave * 16u;", "constexpr uint32_t kWaves = 4;", "constexpr uint32_t kTilesPerWave = 8;",
        "a.spans = (uint32_t)(((uint64_t)a.nr_out + kSpanOut - 1u) / kSpanOut);",
        "a.items = (uint64_t)a.nr_inputs * a.spans;",
        "dim3((uint32_t)(a.items < kGrid ? a.items : kGrid))",
        "for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {",
        "__syncthreads(); // the previous item's reads of the span are done",
    ],
    "bf_integrate.hip": [
        "#pragma unroll 4", "#pragma unroll 8",
        "for (uint32_t j = a.accumulate ? 0u : 1u; j < a.n; j++) acc = acc + p[(uint64_t)j * bs];",
        "for (uint32_t j = 0; j < a.n; j++) sum += p[(uint64_t)j * bs];",
    ],
}


def test_the_models_rules_are_the_kernels():
    for name, lines in ONCE.items():
        text = text_of(name)
        for line in lines:
            assert text.count(line) == 1, (name, line)
    assert (lf.CORR_S, lf.CORR_SB, lf.CORR_WAVES, lf.CORR_GRID) == (4, 2, 4, 1 << 20)
    assert (lf.INCOH_LOADS, lf.INCOH_WAVES, lf.INCOH_GRID) == (8, 4, 2048)
    assert (lf.BOXCAR_BATCH, lf.BOXCAR_WAVES) == (8, 256 // 64) and lf.DDC_SPAN == 4 * 8 * 16 and lf.DDC_GRID == 1 << 20
    assert lf.INTEGRATE_UNROLL == {"f32": 4, "u32": 8, "i32": 8}


def test_the_model_on_cases_worked_out_by_hand():
    assert lf.correlator_units(100) == [(True, 0, 4), (True, 1, 3), (False, 1, 3), (False, 1, 3)]
    assert lf.correlator_units(64) == [(True, 0, 4)] and lf.correlator_units(1) == [(True, 0, 1)]
    assert lf.correlator_units(65) == [(True, 0, 4), (True, 1, 1), (False, 1, 1), (False, 1, 1)]
    u256 = lf.correlator_units(256)
    assert len(u256) == 16 and u256[:4] == [(True, s, 4) for s in range(4)]
    assert [s for _, s, _ in u256[4:]] == [1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3] and all(f == (False, s, 4) for f, s in zip(u256[4:], [1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3]))
    assert lf.correlator_units(150)[-1] == (False, 2, 2) and lf.correlator_plan(150) == (10, 3, 9)
    assert lf.correlator_grid(3, 3, 256) == (144, 40) and lf.correlator_grid(1, 1, 1) == (1, 8)
    assert lf.correlator_grid(1025, 4093, 2) == (4195325, (1 << 20))
    assert [lf.incoherent_form(A) for A in (1, 32, 33, 96, 97, 128, 129, 161, 193, 225, 256)] == \
        [(1, 8), (1, 8), (2, 4), (3, 2), (4, 2), (4, 2), (5, 1), (6, 1), (7, 1), (8, 1), (8, 1)]
    assert lf.candidate_width_chain(21)[0] == (8, 8, 4, 1) and lf.candidate_width_chain(0) == ((), [])
    assert lf.candidate_width_chain(7) == ((4, 1, 1, 1), [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)])
    assert lf.candidate_width_chain(11)[0] == (8, 1, 1, 1) and lf.candidate_width_chain(13)[1][11:] == [(1, 3), (2, 0)]
    # two batches, three blocks: pairs 0 .. 5 dealt to the waves in turn, blocks fastest
    assert lf.boxcar_walk(9, 3) == ([[(0, 0), (1, 1)], [(0, 1), (1, 2)], [(0, 2)], [(1, 0)]], 2)
    # one block: a wave takes every fourth batch
    assert lf.boxcar_walk(40, 1) == ([[(0, 0), (4, 0)], [(1, 0)], [(2, 0)], [(3, 0)]], 5)
    assert lf.boxcar_walk(17, 2)[0][3] == [(1, 1)] and lf.boxcar_walk(17, 2)[0][0] == [(0, 0), (2, 0)]
    assert lf.boxcar_runs(4196, 64) == [64, 2] and lf.boxcar_runs(9000, 192) == [21, 21, 5] and lf.boxcar_runs(59, 64) == [1]
    assert lf.ddc_grid(3, 1100) == (9, 9) and lf.ddc_grid((1 << 20) + 37, 3) == ((1 << 20) + 37, 1 << 20)
    assert [lf.integrate_trips("f32", n, False) for n in (1, 2, 5, 6, 9, 17)] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 0)]
    assert [lf.integrate_trips("f32", n, True) for n in (1, 4, 5, 8, 9)] == [(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert [lf.integrate_trips("i32", n, a) for n in (1, 8, 9, 16, 17, 40) for a in (False, True)] == \
        [(0, 1)] * 2 + [(1, 0)] * 2 + [(1, 1)] * 2 + [(2, 0)] * 2 + [(2, 1)] * 2 + [(2, 0)] * 2
    # the pairs of a walk are every (batch, block) once
    for nw in (1, 8, 9, 33, 40):
        for nb in (1, 2, 3, 4, 5, 7, 64):
            walks, batches = lf.boxcar_walk(nw, nb)
            assert sorted(p for w in walks for p in w) == [(b, k) for b in range(batches) for k in range(nb)]


# ------------------------------------------------------------------------------------------------------------------- census

CORR_FORMS = lf.correlator_forms_that_exist()
TRIPS = {(0, True), (1, False), (1, True), (2, False), (2, True)}  # (full trips capped at 2, a tail or none)
CHAIN_PAIRS = {(8, 8), (8, 4), (8, 1), (4, 1), (1, 1)}             # every pair of consecutive take_widths calls there can be
NB_CLASSES = {1, 2, 3, 4, 5, 6}


def corr_census(stations):
    return {f for A in stations for f in lf.correlator_units(A)}


def chain_census(widths):
    chains = {lf.candidate_width_chain(nw)[0] for nw in widths}
    return chains, {lf.chain_steps(c)[0] for c in chains}, set().union(*(lf.chain_steps(c)[1] for c in chains))


def walk_census(calls):
    """{(min(batches, 5), class of nb)} over every workgroup of the calls."""
    return {(min(lf.boxcar_walk(nw, nb)[1], 5), lf.nb_class(nb)) for nw, T, block_len in calls for nb in lf.boxcar_runs(T, block_len)}


def trips_census(calls):
    out = {}
    for kind, n, acc in calls:
        trips, tail = lf.integrate_trips(kind, n, acc)
        out.setdefault(kind, set()).add((trips, tail > 0))
    return out


def test_the_forms_that_can_exist():
    assert {f for f in CORR_FORMS if f[0]} == {(True, sa, na) for sa in range(4) for na in range(1, 5)}
    assert {f for f in CORR_FORMS if not f[0]} == {(False, sa, na) for sa in (1, 2, 3) for na in range(1, 5)}
    assert {lf.incoherent_form(A)[0] for A in range(1, 257)} == set(range(1, 9))
    assert set().union(*(lf.chain_steps(lf.candidate_width_chain(nw)[0])[1] for nw in range(64))) == CHAIN_PAIRS


def test_census_of_the_older_tables():
    """Facts about the tables as they were, printed and written into DESIGN.md and the profiles/ note: what the new cases are
    for.  The tables stay, so the facts do."""
    seen = corr_census(kc.STATIONS)
    print(f"\ncorrelator, older table: {sorted(seen)}")
    assert [lf.correlator_plan(A)[0] for A in kc.STATIONS] == [1, 1, 1, 2, 4, 7, 16]
    assert {f for f in seen if not f[0]} == {(False, 1, 3), (False, 1, 4), (False, 2, 4), (False, 3, 4)}
    assert not any(na in (1, 2) for d, _, na in seen if not d) and len(seen) == 4 + 7
    # every A of these ranges takes an off-diagonal form with one or two a tiles, which no test has run
    for lo, hi in ((65, 96), (129, 160), (193, 224)):
        assert all(any(not d and na <= 2 for d, _, na in lf.correlator_units(A)) for A in range(lo, hi + 1))
    grids = [lf.correlator_grid(kc.CHANNELS, v, A) for A in kc.STATIONS for v in kc.NR_VIS]
    assert all(4 * wg >= items for items, wg in grids)  # no wave walks
    nc = {lf.incoherent_form(A)[0] for A, _, _ in ic.SHAPES}
    print(f"incoherent beam, older tables: NC {sorted(nc)}; looping {sorted(lf.incoherent_form(s[0]) for s in ic.LOOPING_SHAPES)}")
    assert nc == {1, 2, 3, 5, 8} and {lf.incoherent_form(s[0])[0] for s in ic.LOOPING_SHAPES} == {1, 3, 8}
    chains, eights, pairs = chain_census(cc.old_nr_widths())
    print(f"sifter, older tests: nr_widths {cc.old_nr_widths()}, chains {sorted(chains)}")
    assert cc.old_nr_widths() == [0, 1, 2, 3, 6, 7] and eights == {0} and pairs == {(4, 1), (1, 1)}
    walk = walk_census(sc.old_peaks_calls())
    print(f"boxcar walk, older tests: (batches, nb) {sorted(walk)}")
    assert max(nw for nw, _, _ in sc.old_peaks_calls()) == 13 and {b for b, _ in walk} == {1, 2}
    assert {k for b, k in walk if b == 2} == {3, 5}  # two batches with three and five blocks only: never with one or two
    assert all(lf.ddc_grid(ni, no)[0] == lf.ddc_grid(ni, no)[1] < lf.DDC_GRID for ni, no in dc.old_calls())  # one item a workgroup
    trips = trips_census(gc.old_calls())
    print(f"integrator, older tests: {({k: sorted(v) for k, v in trips.items()})}")
    assert TRIPS - trips["i32"] == {(1, False), (2, False), (2, True)} and TRIPS - trips["u32"] == {(1, False), (2, True)}
    assert TRIPS <= trips["f32"]  # the float loop had every form; what was missing is a sum that depends on its order


def test_every_form_is_run_against_its_model():
    """The bar.  It fails on the older tables alone, and if an entry that alone covers a form is taken out of the new ones."""
    seen = corr_census(kc.STATIONS + kc.FORM_STATIONS)
    print(f"\ncorrelator: {len(seen)} forms of {len(CORR_FORMS)}")
    assert seen == CORR_FORMS and len(CORR_FORMS) == 16 + 12, sorted(CORR_FORMS - seen)
    assert {lf.correlator_plan(A)[0] for A in kc.FORM_STATIONS} == set(range(1, 17))
    assert {min(A % 16, 2) for A in kc.FORM_STATIONS} == {0, 1, 2} and {65, 80, 81, 96, 129, 150, 200} <= set(kc.FORM_STATIONS)
    assert not set(kc.FORM_STATIONS) & set(kc.STATIONS)
    assert {(n % 4 != 0, (n + 3) // 4) for n in kc.FORM_BLOCKS} == {(True, 1), (False, 1), (True, 2)}
    items, wg = lf.correlator_grid(kc.WALK["C"], kc.WALK["nr_vis"], kc.WALK["A"])
    assert 4 * wg < items < 4 * wg + 4096 and lf.correlator_plan(kc.WALK["A"])[2] == 1
    for table in (ic.SHAPES + ic.FORM_SHAPES,):
        assert {lf.incoherent_form(A)[0] for A, _, _ in table} == set(range(1, 9))  # each is run with and without weights
    for A, C, nt in ic.FORM_SHAPES:
        rows, rpw = C * (nt // 16), lf.incoherent_form(A)[1]
        assert rows % 2 == 1 and (rpw == 1 or rows % rpw)
    assert {a for a, _, _ in ic.FORM_SHAPES} == {96, 97, 128, 129, 160, 161, 192, 193, 224, 225}
    looping = ic.LOOPING_SHAPES + ic.FORM_LOOPING_SHAPES
    assert {lf.incoherent_form(s[0]) for s in looping} == {(1, 8), (3, 2), (4, 2), (8, 1)}
    for A, C, nt, rpw in looping:
        assert lf.incoherent_form(A)[1] == rpw and -(-C * (nt // 16) // rpw) > lf.INCOH_GRID * lf.INCOH_WAVES
    chains, eights, pairs = chain_census(cc.FORM_NR_WIDTHS)
    print(f"sifter: chains {sorted(chains)}")
    assert chains == {(8,), (8, 1), (8, 1, 1, 1), (8, 4), (8, 4, 1), (8, 8), (8, 8, 1), (8, 8, 8), (8, 8, 8, 1)}
    assert eights == {1, 2, 3} and pairs | chain_census(cc.old_nr_widths())[2] == CHAIN_PAIRS
    for n8 in (1, 2, 3):  # each number of eights alone and with a tail behind it
        assert {len(c) > n8 for c in chains if c.count(8) == n8} == {False, True}
    walk = walk_census(sc.walk_calls())
    print(f"boxcar walk: (batches, nb) {sorted(walk)}")
    assert walk >= {(b, k) for b in (1, 2, 3, 4, 5) for k in NB_CLASSES}
    trips = trips_census(gc.form_calls())
    assert all(TRIPS <= trips[kind] for kind in ("f32", "u32", "i32")), trips
    assert all(gc.FORM_NBLK % n == 0 for n in gc.FORM_N) and gc.FORM_NBLK == int(np.lcm.reduce(gc.FORM_N))
    items, wg = lf.ddc_grid(dc.WALK["nr_inputs"], dc.WALK["nr_out"])
    assert wg < items == wg + 37 and dc.WALK["in_stride"] == 16 * (dc.WALK["nr_out"] - 1) + dc.WALK["T"]


# -------------------------------------------------------------------------------- conditions on the inputs of the new GPU cases

def test_every_width_index_wins_somewhere_and_the_hand_made_cells_are_won_as_stated():
    B, nr_dm, blocks = cc.FORM_SHAPE
    for nw in cc.FORM_NR_WIDTHS:
        snr, peaks = cc.form_planes(nw)
        s, best = collapse(snr, 0, blocks)
        for radii in cc.FORM_RADII:
            rec, _ = find_candidates(snr, peaks, 0, blocks, cc.FORM_THRESHOLD, *radii, 0)
            assert set(rec["width_index"].tolist()) == set(range(nw)), (nw, radii)
            won = {(int(r["dm"]), int(r["block"])): int(r["width_index"]) for r in rec}
            for cell, (_, winner) in cc.hand_cells(nw).items():
                assert won[cell] == winner, (nw, radii, cell)
        pairs = [p for p in cc.TIE_PAIRS if p[1] < nw]
        assert len(pairs) == (0 if nw < 9 else 1 if nw < 13 else 2 if nw < 16 else 3)
        # a collapse that skipped the first width of any call would lose: every chain position is some cell's winner
        _, at = lf.candidate_width_chain(nw)
        assert {at[i] for i in np.unique(best[best != 0xFFFFFFFF]).tolist()} == set(at)


def test_walk_shapes_make_every_wave_take_several_pairs():
    for nw in sc.WALK_NR_WIDTHS:
        widths = sc.walk_widths(nw)
        assert len(widths) == nw and max(w for w in widths if w <= sc.WALK_MAX_WIDTH) <= 64
        batches = (nw - 1) // 8 + 1
        if batches > 1:
            assert widths[8] == 0 and (nw == 9 or widths[-1] == sc.WALK_MAX_WIDTH + 1)  # dropped: second batch, last batch
        for nb in sc.WALK_NB:
            assert lf.boxcar_runs(sc.walk_T(nb), sc.WALK_BLOCK_LEN) == [nb] and sc.walk_T(nb) % sc.WALK_BLOCK_LEN
            walks, b = lf.boxcar_walk(nw, nb)
            assert b == batches and [len(w) for w in walks] == [-(-(b * nb - wave) // 4) if b * nb > wave else 0 for wave in range(4)]
            if b * nb >= 8:  # eight pairs or more: every wave goes round its loop at least twice
                assert min(len(w) for w in walks) >= 2
    # every nb is met with eight pairs or more, and the single block with a wave whose batches are four apart
    for nb in sc.WALK_NB:
        assert any(((nw - 1) // 8 + 1) * nb >= 8 for nw in sc.WALK_NR_WIDTHS)
    assert any(w[1][0] - w[0][0] == 4 for nw in sc.WALK_NR_WIDTHS for w in lf.boxcar_walk(nw, 1)[0] if len(w) > 1)
    assert lf.boxcar_runs(sc.WALK_LONG_T, sc.WALK_BLOCK_LEN) == [64, 2]
