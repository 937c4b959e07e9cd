"""The CPU model of the forms that six kernels and the integrator take (helpers/launch_forms.py; DESIGN.md, "The forms" of
sections 5.4, 5.11, 5.17 to 5.20 and 5.22): its rules against the kernels' source text, worked cases, a census of what the older
tables of the GPU tests present to the launchers (helpers/*_cases.py; printed with pytest -s), and the bar: every form that
can exist is run against its model by the tables as they are now.  The conditions that the new GPU cases rely on -- every
width index wins somewhere, every wave of the boxcar kernel takes several pairs, a reordered float sum differs -- are asserted
here on the numpy models alone: if a builder misses one, the builder is wrong."""
from pathlib import Path

import numpy as np

from helpers import bacc_cases as bc
from helpers import candidates_cases as cc
from helpers import correlator_cases as kc
from helpers import ddc_cases as dc
from helpers import incoherent_cases as ic
from helpers import integrate_cases as gc
from helpers import launch_forms as lf
from helpers import single_pulse_cases as sc
from helpers.bacc_case import plan_of
from helpers.candidates_model import collapse, find_candidates

CSRC = Path(__file__).resolve().parent.parent / "dc_sand_amd" / "csrc"


def text_of(name):
    return (CSRC / name).read_text()


# ------------------------------------------------------------------------------------------------- rules held to the source

ONCE = {
    "bf_beamform_mfma.hip": [
        "constexpr uint32_t kKC = 64; // antennas per staged chunk (16 k-steps of 4)",
        "constexpr int TPR = 4 / NBT;                                  // 16-sample blocks per round",
        "const uint32_t bt = wave % NBT, slot = wave / NBT;",
        "const uint32_t n_chunks = (a.A + kKC - 1u) / kKC;",
        "const uint32_t n_blocks = tt1 > tt0 + slot ? (tt1 - tt0 - slot + TPR - 1u) / TPR : 0u; // this wave's sample blocks",
        "floatx2 *dst = reinterpret_cast<floatx2 *>(a.beams) + ((uint64_t)c * a.nT16 + tt0 + blk * TPR + slot) * a.B * 16u + lm;",
        "const uint32_t A_pad = (A + 3u) & ~3u;",
        "const uint32_t ws = 16u * (uint32_t)nbt + (nbt > 1 ? 16u : 0u);",
        "return (size_t)A_pad * ws * 2u * sizeof(float);",
        "if constexpr (!(Q && P)) // (the launcher has refused that)",
        "}, w != nullptr, q != nullptr, power, cx != nullptr);",
        "if (a.A > 256u) return hipErrorInvalidValue; // not built",
        "const bool chain = a.fp32_chain != 0u;",
        "if ((w || q || power || cx) && chain) return hipErrorInvalidValue;",
        "if (q && power) return hipErrorInvalidValue;",
        "const bool wide = !chain && a.A > 64u;",
        "const bool staged_form = !chain && a.A <= 64u && !BACC_KNOB(a, unstaged);",
        "int nbt = wide ? 1 : (a.B > 32u ? 4 : (a.B > 16u ? 2 : 1));",
        "uint32_t nw = nbt == 8 ? 8u : 4u; // waves per workgroup",
        "while (chain && nbt > 1 && bacc_lds_bytes(nbt, a.A) > 26u * 1024u) nbt >>= 1;",
        "const size_t lds = chain ? bacc_lds_bytes(nbt, a.A) : 0u;",
        "a.nbt_log2 = nbt == 8 ? 3u : (nbt == 4 ? 2u : (nbt == 2 ? 1u : 0u));",
        "a.n_bgroups = (a.B + 16u * (uint32_t)nbt - 1u) / (16u * (uint32_t)nbt);",
        "const uint32_t tpr = split ? 1u : nw / (uint32_t)nbt;",
        "const uint32_t blocks_cap = staged_form && nbt == 4 && a.n_bgroups == 1u ? 8u : 16u;",
        "const uint32_t max_rounds = BACC_KNOB(a, max_rounds) ? BACC_KNOB(a, max_rounds) : (chain ? 16u : (staged_form || wide ? blocks_cap / tpr : 32u));",
        "uint32_t tiles = (a.nT16 + tpr - 1u) / tpr * tpr;",
        "if (tiles > max_rounds * tpr) {",
        "const uint32_t parts = (a.nT16 + max_rounds * tpr - 1u) / (max_rounds * tpr);",
        "tiles = ((a.nT16 + parts - 1u) / parts + tpr - 1u) / tpr * tpr;",
        "const uint64_t enough = chain ? 4096u : 5120u / nw;",
        "while (tiles > tpr && (uint64_t)a.C * a.n_bgroups * ((a.nT16 + tiles - 1u) / tiles) < enough) tiles = ((tiles / tpr + 1u) / 2u) * tpr;",
        "a.tiles_per_wg = tiles;",
        "a.n_tgroups = (a.nT16 + tiles - 1u) / tiles;",
        "a.xcd_group = wide ? a.n_bgroups : (!chain && a.n_bgroups >= 16u ? a.n_bgroups : 1u);",
        "const uint64_t blocks = (uint64_t)a.C * a.n_bgroups * a.n_tgroups;",
        "const dim3 grid((uint32_t)blocks), block(64u * nw);",
        "hipLaunchKernelGGL(bf_beamform_acc_kernel<4>, grid, block, lds, stream, a);",
        "hipLaunchKernelGGL(bf_beamform_acc_kernel<2>, grid, block, lds, stream, a);",
        "hipLaunchKernelGGL(bf_beamform_acc_kernel<1>, grid, block, lds, stream, a);",
        "if (q && a.tiles_per_wg / tpr > 126u) return hipErrorInvalidValue;",
        "const bool full = a.A % 64u == 0u;",
        "size_t stage_bytes = ((size_t)a.tiles_per_wg * a.A * 32u + 1023u) / 1024u * 1024u;",
        "if (tpr > 1u && !BACC_KNOB(a, no_share)) {",
        "stage_bytes += (size_t)nbt * 4u * (cx ? 9u : 6u) * 64u * sizeof(uint32_t);",
        "launch_i8_form<kStaged>(full, grid, block, stage_bytes, stream, a, w, q, power, cx);",
        "const size_t coef_bytes = 4u * (cx ? 9u : 6u) * 64u * 16u + 8u * sizeof(uint32_t) + (q ? 32u : (w ? 16u : 0u)) * sizeof(float);",
        "launch_i8_form<kChain>(full, grid, block, coef_bytes, stream, a, w, q, power, cx);",
    ],
    "bf_beamform_i8_kernel.inc": [
        "const uint32_t nbt_log2 = SPLIT || CHAIN ? 0u : a.nbt_log2;",
        "const uint32_t nbt = 1u << nbt_log2, tpr = SPLIT ? 1u : (uint32_t)NW >> nbt_log2;",
        "const uint32_t bt = SPLIT ? 0u : wave & (nbt - 1u), slot = SPLIT ? 0u : wave >> nbt_log2;",
        "const uint32_t tt0 = tg * a.tiles_per_wg;",
        "const uint32_t tt1 = min(tt0 + a.tiles_per_wg, a.nT16);",
        "const uint32_t n_blocks = tt1 > tt0 + slot ? (tt1 - tt0 - slot + tpr - 1u) / tpr : 0u; // this wave's sample blocks",
    ],
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
    assert (lf.BACC_WAVES, lf.BACC_CHUNK, lf.BACC_FP32_LDS_CAP, lf.BACC_ENOUGH_INT8, lf.BACC_ENOUGH_FP32) == (4, 64, 26 * 1024, 5120, 4096)
    # the product build: every BACC_KNOB is 0 there, and what stands under DCS_PROBES does not exist
    assert text_of("bf_kernels.h").count("#define BACC_KNOB(a, f) 0u") == 1


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


# ------------------------------------------------------------------------------------------- the matrix-core beamformer

def test_the_beamformer_plan_on_cases_worked_out_by_hand():
    # 64 beams at 64 antennas: four tiles fill ONE beam group, so the cap is 8 blocks; 9 blocks are two equal shares of 5 (and
    # 4), 640 x 1 x 2 = 1280 workgroups are enough, nothing is halved; tpr 1: every wave has all the workgroup's blocks
    p = lf.bacc_plan(64, 40, 640, 144)
    assert (p["form"], p["full"], p["nbt"], p["tpr"], p["blocks_cap"], p["tiles_per_wg"], p["n_tgroups"], p["grid"]) == \
        ("staged", True, 4, 1, 8, 5, 2, 1280)
    assert p["blocks_full"] == [5] * 4 and p["blocks_last"] == [4] * 4 and p["lds"] == 5 * 64 * 32 and p["xcd_group"] == 1
    # kChain, four whole chunks: one tile whatever B is, three beam groups; 17 blocks over the cap of 16 are 2 shares of 9,
    # rounded up to rounds of 4: 12 and 5; 216 x 3 x 2 = 1296
    p = lf.bacc_plan(256, 33, 216, 272)
    assert (p["form"], p["full"], p["nbt"], p["tiles_per_wg"], p["n_tgroups"], p["n_bgroups"], p["grid"], p["xcd_group"]) == \
        ("chain", True, 1, 12, 2, 3, 1296, 3)
    assert p["blocks_full"] == [3] * 4 and p["blocks_last"] == [1, 1, 1, 2] and (p["chunks"], p["partial_chunk"]) == (4, False)
    assert p["lds"] == 24 * 1024 + 32 and lf.bacc_plan(256, 33, 216, 272, complex_=True, quant=True)["lds"] == 36 * 1024 + 32 + 128
    assert lf.bacc_plan(256, 33, 216, 272, weighted=True)["lds"] == 24 * 1024 + 32 + 64
    # sixteen beam groups: 40 x 16 = 640 workgroups with all 5 blocks, halved once to 3 (and 2): 1280; grouped on the XCDs
    p = lf.bacc_plan(64, 1024, 40, 80)
    assert (p["tiles_per_wg"], p["n_tgroups"], p["n_bgroups"], p["xcd_group"], p["grid"], p["blocks_cap"]) == (3, 2, 16, 16, 1280, 16)
    # two tiles share the making of the coefficients: 6 (9 complex) operands x 4 registers x 64 lanes x 4 bytes per tile
    p = lf.bacc_plan(37, 21, 640, 144)
    assert (p["nbt"], p["tpr"], p["tiles_per_wg"], p["blocks_full"], p["blocks_last"]) == (2, 2, 6, [3] * 4, [1, 1, 2, 2])
    assert p["lds"] == 7 * 1024 + 2 * 6 * 1024 and lf.bacc_plan(37, 21, 640, 144, complex_=True)["lds"] == 7 * 1024 + 2 * 9 * 1024
    # 33 blocks: three shares of 11, rounded to 12; the last workgroup has 9: waves of 3, 2, 2, 2
    p = lf.bacc_plan(64, 16, 427, 528)
    assert (p["tiles_per_wg"], p["n_tgroups"], p["grid"], p["blocks_last"]) == (12, 3, 1281, [2, 2, 2, 3])
    # the fp32 form: 41 antennas are 44 rows; four tiles are rows of 80 floats, 44 x 80 x 8 = 28 160 bytes > 26 KiB; two tiles
    # rows of 48: 16 896
    p = lf.bacc_plan(41, 33, 16, 16, fp32_chain=True)
    assert (p["form"], p["nbt"], p["lds_of_four_tiles"], p["lds"], p["n_bgroups"]) == ("fp32", 2, 28160, 16896, 2)
    p = lf.bacc_plan(40, 40, 2048, 64, fp32_chain=True)  # 40 rows: 25 600 bytes fit
    assert (p["nbt"], p["lds"], p["tiles_per_wg"], p["blocks_full"], p["grid"]) == (4, 25600, 2, [2] * 4, 4096)
    # 17 blocks in rounds of 4 are 20; 2048 workgroups are under 4096, so the share is halved to 12 (and 5): 4096
    p = lf.bacc_plan(8, 4, 2048, 272, fp32_chain=True)
    assert (p["tiles_per_wg"], p["n_tgroups"], p["grid"], p["blocks_full"], p["blocks_last"], p["lds"]) == (12, 2, 4096, [3] * 4, [1, 1, 1, 2], 1024)
    # ... where the int8 form, whose line is 1280, keeps all 17 blocks in one workgroup of up to 16?  No: 17 > 16 are 2 shares
    assert lf.bacc_plan(8, 4, 2048, 272)["tiles_per_wg"] == 12 and lf.bacc_plan(8, 4, 2048, 256)["tiles_per_wg"] == 16
    # every shape of ACC_SHAPES leaves the fp32 form ONE block per wave: 288 workgroups at the most, 20 / 13 / 2 shapes at 1 / 2 / 4 tiles
    plans = [lf.bacc_plan(*s, fp32_chain=True) for s in bc.ACC_SHAPES]
    assert max(p["grid"] for p in plans) == 288 and all(lf.bacc_depth(p) == 1 for p in plans)
    assert [sum(p["nbt"] == n for p in plans) for n in (1, 2, 4)] == [20, 13, 2]
    # the quantiser's refusal of more than 126 pairs of blocks per wave cannot be reached: rounds are 16 at the most
    assert all(lf.bacc_plan(A, B, 1, 16 * n, quant=True)["tiles_per_wg"] // lf.bacc_plan(A, B, 1, 16 * n, quant=True)["tpr"] <= 16
               for A in (1, 64, 65, 256) for B in (1, 17, 33, 64, 65) for n in (1, 16, 17, 64, 1000))
    assert lf.bacc_instantiation(200, weighted=True, complex_=True) == ("chain", False, True, False, False, True)
    assert lf.bacc_instantiation(64, quant=True) == ("staged", True, False, True, False, False)
    assert len(lf.bacc_instantiations_that_exist()) == 48 and len(lf.BACC_FLAGS) == 12


STAGED_TILES, CHAIN_CHUNKS = (1, 2, 4), (2, 3, 4)
GEOMETRY_CLASSES = ({("staged", n, whole) for n in STAGED_TILES for whole in (True, False)} |
                    {("chain", n, whole) for n in CHAIN_CHUNKS for whole in (True, False)} |
                    {"A = 65", "1 time group", "2 time groups", "3 time groups and more", "waves of one workgroup differ",
                     "XCD-grouped beyond its 8 x group head"})
FP32_CLASSES = {("nbt", 1), ("nbt", 2), ("nbt", 4), "several chunks, the last partial", "several whole chunks"}


def geometry_classes(A, p):
    """The classes of bar (b) that a deep plan of the int8 form stands for."""
    out = {("staged", p["nbt"], p["full"])} if p["form"] == "staged" else {("chain", p["chunks"], not p["partial_chunk"])}
    if A == 65:
        out.add("A = 65")
    out.add(("1 time group", "2 time groups", "3 time groups and more")[min(p["n_tgroups"], 3) - 1])
    if any(len(set(b)) > 1 and b[-1] >= 3 for b in (p["blocks_full"], p["blocks_last"])):
        out.add("waves of one workgroup differ")
    if p["xcd_group"] > 1 and p["grid"] > 8 * p["xcd_group"]:
        out.add("XCD-grouped beyond its 8 x group head")
    return out


def bacc_census(runs):
    """(shallow, deep, float_classes, flag_classes, fp32_classes): the instantiations run with one block per wave and at
    depth; the geometry classes at which the unweighted float call is deep; per flag combination the forms at which it is
    deep (staged by tiles, kChain); the classes at which the fp32 form is deep."""
    shallow, deep, float_classes, fp32_classes = set(), set(), set(), set()
    flag_classes = {f: set() for f in lf.BACC_FLAGS}
    for run in runs:
        for shape in run.shapes:
            for call in run.calls:
                p = plan_of(shape, call)
                if p["form"] == "fp32":
                    if lf.bacc_is_deep(p):
                        fp32_classes.add(("nbt", p["nbt"]))
                        if p["chunks"] > 1:
                            fp32_classes.add("several chunks, the last partial" if p["partial_chunk"] else "several whole chunks")
                    continue
                name, weighted, _ = call
                flags = (weighted,) + bc.KINDS[name]
                inst = lf.bacc_instantiation(shape[0], *flags)
                if lf.bacc_depth(p) == 1:
                    shallow.add(inst)
                if lf.bacc_is_deep(p):
                    deep.add(inst)
                    flag_classes[flags].add(("staged", p["nbt"]) if p["form"] == "staged" else "chain")
                    if call == bc.F:
                        float_classes |= geometry_classes(shape[0], p)
    return shallow, deep, float_classes, flag_classes, fp32_classes


def bar_gaps(runs):
    """What the bar (a) .. (d) misses on ``runs``, as a list of strings; empty when it holds."""
    shallow, deep, float_classes, flag_classes, fp32_classes = bacc_census(runs)
    every = lf.bacc_instantiations_that_exist()
    gaps = [f"(a) never with one block per wave: {i}" for i in sorted(every - shallow)]
    gaps += [f"(a) never deep: {i}" for i in sorted(every - deep)]
    gaps += [f"(b) the float call is never deep at: {c}" for c in sorted(GEOMETRY_CLASSES - float_classes, key=str)]
    want = {("staged", n) for n in STAGED_TILES} | {"chain"}
    gaps += [f"(c) (W, Q, P, C) = {f} is never deep at: {c}" for f in lf.BACC_FLAGS for c in sorted(want - flag_classes[f], key=str)]
    gaps += [f"(d) the fp32 form is never deep at: {c}" for c in sorted(FP32_CLASSES - fp32_classes, key=str)]
    return gaps


def without(runs, table, shape):
    """``runs`` with ``shape`` taken out of every run of ``table``."""
    return [r._replace(shapes=[s for s in r.shapes if s != shape]) if r.table == table else r for r in runs]


def test_the_declared_runs_name_tests_that_exist_and_take_their_parameters_from_the_list():
    tests = Path(__file__).resolve().parent
    for run in bc.RUNS:
        name, func = run.test.split("::")
        text = (tests / name).read_text()
        assert text.count(f"\ndef {func}(") == 1, run.test
        head = text[:text.index(f"\ndef {func}(")].rsplit("\n\n", 1)[-1]  # the decorators
        prefix = {bc.PARITY: "bc.PARITY", bc.EXACT: "bc.EXACT", bc.WEIGHTS: "bc.WEIGHTS", bc.QUANT: "bc.QUANT", bc.POWER: "bc.POWER",
                  bc.COMPLEX: "bc.COMPLEX", bc.CQUANT: "bc.CQUANT"}[name + "::"]
        assert f'bc.shapes_of({prefix} + "{func}"' in head, run.test
        assert all(len(s) == 4 and s[3] % 16 == 0 for s in run.shapes) and run.calls, run.test


def test_census_of_the_older_beamformer_tables():
    """Facts about the tables and tests as they were (bc.older_runs), printed and written into DESIGN.md and the profiles/ note."""
    shallow, deep, float_classes, flag_classes, fp32_classes = bacc_census(bc.older_runs())
    every = lf.bacc_instantiations_that_exist()
    print(f"\nbeamformer, older tables: {len(shallow)} of 48 instantiations with one block per wave, {len(deep)} deep")
    print("never deep (FORM, FULL, W, Q, P, C):", *sorted(every - deep), sep="\n  ")
    print("the float call never deep at:", sorted(GEOMETRY_CLASSES - float_classes, key=str))
    print("flag combinations (W, Q, P, C) not deep everywhere:",
          {f: sorted({("staged", 1), ("staged", 2), ("staged", 4), "chain"} - c, key=str) for f, c in flag_classes.items()
           if len(c) < 4})
    print("fp32 form deep at:", sorted(fp32_classes, key=str))
    assert shallow == every and fp32_classes == set()
    # every instantiation without the complex product was deep; of the 24 with it, these 11 never: all six of kChain with FULL, the
    # four detecting ones of kStaged, and the weighted detecting one of ragged kChain (the detecting call was deep at A = 130
    # alone, without weights)
    never = every - deep
    assert never == ({("chain", True, w, q, p, True) for w, q, p, c in lf.BACC_FLAGS if c} |
                     {("staged", full, w, False, True, True) for full in (False, True) for w in (False, True)} |
                     {("chain", False, True, False, True, True)}) and len(never) == 11
    # (the weighted complex float call counts as deep: the quantised test made it, but held it to no model -- it was the
    # reference of the bytes.  test_several_blocks_per_wave_bit_for_bit holds it to the model now.)
    assert GEOMETRY_CLASSES - float_classes == {("staged", 2, False), ("chain", 3, True), ("chain", 4, False), "A = 65", "3 time groups and more",
                                                "waves of one workgroup differ"}  # (they differed only where none has a third block)
    assert all(("staged", 2) not in c for f, c in flag_classes.items() if f[3]) and all(len(c) == 4 for f, c in flag_classes.items() if not f[3])


def test_every_beamformer_instantiation_and_geometry_class_is_run_shallow_and_deep():
    """The bar (a) .. (d) on the tables as they are, and that it fails when an entry that alone covers a class is taken out."""
    shallow, deep, float_classes, flag_classes, fp32_classes = bacc_census(bc.RUNS)
    print(f"\nbeamformer: {len(shallow)} of 48 instantiations with one block per wave, {len(deep)} deep; the float call deep at "
          f"{len(float_classes & GEOMETRY_CLASSES)} of {len(GEOMETRY_CLASSES)} geometry classes; fp32 form deep at {sorted(fp32_classes, key=str)}")
    for s, call in [(s[:4], bc.F) for s in bc.DEEP_SHAPES] + [(s, bc.F8) for s in bc.FP32_DEEP_SHAPES]:
        p = plan_of(s, call)
        print(f"  {s}: {p['form']}, nbt {p['nbt']}, {p['chunks']} chunk(s){' (partial)' if p['partial_chunk'] else ''}, "
              f"{p['tiles_per_wg']} blocks a workgroup, {p['n_tgroups']} time group(s), grid {p['grid']}, LDS {p['lds']}, "
              f"blocks per wave {p['blocks_full']} / last {p['blocks_last']}")
    assert bar_gaps(bc.RUNS) == []
    assert bar_gaps(bc.older_runs())  # the older tables alone miss it
    # an entry that alone covers a class, taken out
    for table, shape, gap in (("DEEP_SHAPES", (65, 16, 640, 272), "(b) the float call is never deep at: A = 65"),
                              ("DEEP_SHAPES", (64, 16, 427, 528), "(b) the float call is never deep at: 3 time groups and more"),
                              ("DEEP_SHAPES", (37, 21, 640, 144), "(b) the float call is never deep at: ('staged', 2, False)"),
                              ("DEEP_SHAPES", (192, 16, 640, 272), "(b) the float call is never deep at: ('chain', 3, True)"),
                              ("DEEP_SHAPES", (200, 20, 320, 272), "(b) the float call is never deep at: ('chain', 4, False)"),
                              ("COMPLEX_DEEP", (64, 24, 640, 144), "(c) (W, Q, P, C) = (False, False, False, True) is never deep at: ('staged', 2)"),
                              ("FP32_DEEP_SHAPES", (40, 40, 2048, 64), "(d) the fp32 form is never deep at: ('nbt', 4)"),
                              ("FP32_DEEP_SHAPES", (128, 5, 2048, 144), "(d) the fp32 form is never deep at: several whole chunks")):
        gaps = bar_gaps(without(bc.RUNS, table, shape))
        print(f"without {shape} in {table}: {gaps}")
        assert gap in gaps, (table, shape, gaps)
    # the depth the tables ask their launches to prove is the plan's
    for A, B, C, nt, depth in bc.DEEP_SHAPES:
        assert lf.bacc_depth(plan_of((A, B, C, nt), bc.F)) >= depth >= bc.MIN_DEPTH
    assert all(lf.bacc_plan(*s, fp32_chain=True)["grid"] == 4096 for s in bc.FP32_DEEP_SHAPES)
