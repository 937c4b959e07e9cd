"""The beamformers' class words under graph replay (clear_class_words in dc_sand_amd/csrc/bf_capi_beamform.hip).

Both beamformers choose how they make their coefficients from a per-time-step class word that the terms pre-pass leaves
in the context: the highest pair class of the table (low- or full-degree fast path, or the slow path, which also marks
NaN rows).  A table from rand_table is all in the lowest class, so no replay test of a random table ever wrote a word.
Here a table has ONE pair of a higher class -- full degree (fPhase_rad 20000), slow and finite (40000), or NaN
(fDelayRate_sps inf, beam 2) -- each in a beam of its own, and captured calls are replayed on new samples, weights and gains
among other graphs and plain calls of the same context.  Every output is held twice:

 (a) against the CPU oracle, at the bound of the plain-call tests (4e-5 A + 1e-6 for the matrix-core call,
     tests/test_gpu_parity.py; 2e-5 A + 1e-6 for the per-sample fused call, tests/test_gpu_parity_fused.py;
     times s_b with weights), NaN exactly where the
     oracle has NaN.  The quantised and the detected outputs are the numpy models (helpers/beam_quant_model.py,
     helpers/beam_power_model.py) of the float output, byte for byte and bit for bit;
 (b) bit for bit against the same call made plainly on a FRESH context with the same table, samples, weights and gains:
     what a call returns must not depend on what its context did before.

Per (shape, class) the sample sets, the oracle's expectations and the fresh contexts' outputs are made once and shared by
the scenarios (they come in that order; one group is kept at a time).  The per-sample fused call of the matrix-core
scenarios works on the first 32 samples; at the deep shapes the oracle holds the first 8 channels of its output (its
class word is per time step and shared by every channel), (b) the whole tensor."""
from functools import partial

import numpy as np
import pytest

from conftest import rand_table
from helpers import hip_graph
from helpers.bacc_case import DEEP_SHAPES, T_COEFF, Case
from helpers.beam_power_model import block_power, same_bits
from helpers.beam_quant_model import quantise
from helpers.device_buffers import closed_after

pytestmark = pytest.mark.gpu

HIGH_BEAM, NAN_BEAM, SLOW_BEAM = 1, 2, 3
CLASSES = ("high", "slow", "nan")
# kStaged and kChain where every wave has one sample block, and one of DEEP_SHAPES each (the smallest: the stale word is then
# read by waves that go on to several blocks); the fifth number is the depth the launch must prove, 0 for none
STAGED_DEEP, CHAIN_DEEP = DEEP_SHAPES[1], DEEP_SHAPES[6]
MC_SHAPES = [(64, 16, 2, 32, 0), (130, 20, 2, 32, 0), STAGED_DEEP, CHAIN_DEEP]
assert STAGED_DEEP[0] <= 64 < CHAIN_DEEP[0]
TWO_CHUNKS = (129, 255, 1, 256)  # 32895 pairs: the terms table holds 254 time steps, a call of 256 is 240 + 16
FUSED_ORACLE_CHANNELS = 8


def class_table(A, B, cls):
    """(table [b*A + a], the all-low table it was made from, {class: (beam, antenna)} of the pairs that differ)."""
    low = rand_table(A * B, seed=A + B)
    table, where = low.copy(), {}
    if cls in ("high", "all"):
        where["high"] = (HIGH_BEAM, A // 3)
        table["fPhase_rad"][HIGH_BEAM * A + A // 3] = 20000.0
    if cls in ("slow", "all"):
        where["slow"] = (SLOW_BEAM, A // 2)
        table["fPhase_rad"][SLOW_BEAM * A + A // 2] = 40000.0
    if cls in ("nan", "all"):
        where["nan"] = (NAN_BEAM, min(3, A - 1))
        table["fDelayRate_sps"][NAN_BEAM * A + min(3, A - 1)] = np.inf
    assert where, cls
    return table, low, where


def gains_of(v):
    """k_b = 254 / max |v_b| over the finite components: what lies above half a beam's maximum clips, the rest does not;
    1 for a beam without a finite, non-zero component."""
    m = np.where(np.isfinite(v), np.abs(v), 0).max(axis=(0, 1, 3, 4)).astype(np.float64)
    return np.where(m > 0, 254.0 / np.where(m > 0, m, 1.0), 1.0).astype(np.float32)


class RCase(Case):
    """Case plus the quantiser's and the detector's buffers and the fused call on the first ``fnt`` samples, each output
    with a canary behind it; every call can be made on this context or on a fresh one, plainly or into a graph, all on
    one stream."""

    def __init__(self, gpu, oracle, A, B, C, nt, table, fnt=None):
        super().__init__(gpu, oracle, A, B, C, nt, table=table)
        self.qbytes = C * nt * B * 2
        self.d_q = self.out(self.qbytes)
        self.d_k = self.alloc(B * 4)
        self.d_clip = self.alloc(B * 8)
        self.pshape = (C, nt // 16, B)
        self.pbytes = C * (nt // 16) * B * 4
        self.d_p = self.out(self.pbytes)
        self.fnt = min(nt, 32) if fnt is None else fnt
        self.fshape = (C, self.fnt // 16, B, 16, 2)
        self.fbytes = int(np.prod(self.fshape)) * 4
        self.fant_bytes = C * self.fnt * A * 2
        self.d_fant = self.alloc(self.fant_bytes)
        self.d_fbeams = self.out(self.fbytes, 0xFF, 0xFF)
        self.s = gpu.Stream()

    def load(self, ant, w=None):
        self.set_ant(ant)
        self.gpu.memcpy_htod(self.d_fant, np.ascontiguousarray(ant[:, :self.fnt // 16]))
        if w is not None:
            self.gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))

    def set_gains(self, k):
        self.gpu.memcpy_htod(self.d_k, np.ascontiguousarray(k, dtype=np.float32))

    def enqueue(self, kind, g=None, weighted=False, stream=None):
        g = self.g if g is None else g
        w = self.d_w if weighted else None
        if kind == "float":
            if weighted:
                g.beamform_accumulated_weighted(self.d_ant, self.ant.nbytes, w, self.d_beams, self.nbytes, self.nt, t_coeff=T_COEFF,
                                                stream=stream)
            else:
                g.beamform_accumulated(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, self.nt, t_coeff=T_COEFF, stream=stream)
        elif kind == "q8":
            g.beamform_accumulated_q8(self.d_ant, self.ant.nbytes, self.d_k, self.d_q, self.qbytes, self.nt, t_coeff=T_COEFF,
                                      d_weights=w, d_clip_count=self.d_clip, stream=stream)
        elif kind == "power":
            g.beamform_accumulated_power(self.d_ant, self.ant.nbytes, self.d_p, self.pbytes, self.nt, t_coeff=T_COEFF, d_weights=w,
                                         stream=stream)
        elif weighted:
            assert kind == "fused"
            g.generate_and_beamform_weighted(self.d_fant, self.fant_bytes, w, self.d_fbeams, self.fbytes, t0=0, nt=self.fnt, stream=stream)
        else:
            assert kind == "fused"
            g.generate_and_beamform(self.d_fant, self.fant_bytes, self.d_fbeams, self.fbytes, t0=0, nt=self.fnt, stream=stream)

    def clean(self, kind):
        gpu, s = self.gpu, self.s.handle
        if kind == "float":
            self.refill(self.d_beams, stream=s)
        elif kind == "q8":
            self.refill(self.d_q, stream=s)
            gpu.memset(self.d_clip, 0, self.B * 8, stream=s)
        elif kind == "power":
            self.refill(self.d_p, stream=s)
        else:
            self.refill(self.d_fbeams, stream=s)

    def fetch(self, kind):
        if kind == "float":
            return self.read_beams()
        if kind == "q8":
            n = np.empty(self.B, dtype=np.uint64)
            self.gpu.memcpy_dtoh(n, self.d_clip)
            return self.read(self.d_q, self.qbytes, np.int8, self.shape), n
        if kind == "power":
            return self.read(self.d_p, self.pbytes, np.float32, self.pshape)
        return self.read(self.d_fbeams, self.fbytes, np.float32, self.fshape)

    def plain(self, kind, weighted=False, g=None):
        self.clean(kind)
        self.enqueue(kind, g, weighted, self.s.handle)
        self.s.synchronize()
        return self.fetch(kind)

    def fresh(self, kind, weighted=False):
        """The call made plainly on a context that has done nothing else."""
        from dc_sand_amd.generator import SteeringCoefficientGenerator

        g = SteeringCoefficientGenerator(self.bp)
        try:
            g.upload_delays(self.table, stream=self.s.handle)  # on the stream of the call: it is a non-blocking one
            return self.plain(kind, weighted, g)
        finally:
            g.close()

    def capture(self, kind, weighted=False):
        with hip_graph.capture(self.s) as graph:
            self.enqueue(kind, None, weighted, self.s.handle)
        return graph

    def replay(self, graph, kind):
        self.clean(kind)
        graph.launch(self.s)
        self.s.synchronize()
        return self.fetch(kind)


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(RCase, gpu, oracle))


class Refs:
    """What the scenarios of one (shape, class) share: sample sets, weights, the oracle's expectations (with the sanity
    conditions on the inputs) and the outputs of fresh contexts.  Everything is made once and not changed."""

    def __init__(self, oracle, A, B, C, nt, cls, fnt=None):
        from dc_sand_amd import BeamformerParameters
        from dc_sand_amd.generator import delta_times

        self.oracle, self.A, self.B, self.C, self.nt, self.cls = oracle, A, B, C, nt, cls
        self.fnt = min(nt, 32) if fnt is None else fnt
        self.table, self.low, self.where = class_table(A, B, cls)
        self.bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        self.op = oracle.params_from(self.bp)
        self.dt = delta_times(self.bp, T_COEFF, 1)[0]
        self.fnc = min(C, FUSED_ORACLE_CHANNELS)
        self.memo = {}
        special = {a for _, a in self.where.values()}
        self.flag_antenna = next(iter(special)) if len(special) == 1 else None  # "flagged": the one special pair's antenna
        self.taper_antenna = A - 1  # "taper": 2^k per beam, this antenna flagged
        assert self.taper_antenna not in special or A == 1
        self.taper = (2.0 ** (np.arange(B) % 5 - 2)).astype(np.float32)

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def ant(self, i):
        return self.once(("ant", i), lambda: np.random.default_rng(1000 * (i + 1) + self.A + self.B).integers(
            -128, 128, size=(self.C, self.nt // 16, self.A, 16, 2), dtype=np.int8))

    def weights(self, wl):
        w = np.ones((self.B, self.A), np.float32)
        if wl == "flagged":
            w[:, self.flag_antenna] = 0.0
        elif wl == "taper":
            w *= self.taper[:, None]
            w[:, self.taper_antenna] = 0.0
        else:
            assert wl == "ones", wl
        return w

    def scale(self, wl):
        """s_b of the weights: what the bound against the oracle is multiplied by."""
        return self.taper.astype(np.float64) if wl == "taper" else np.ones(self.B)

    def _inputs(self, i, wl):
        """(table, samples) the unweighted oracle gives the weighted expectation from: a flagged antenna (weight 0 in
        every beam) contributes nothing whatever its delay values are -- its samples zeroed and its pairs finite."""
        ant = self.ant(i)
        if wl in (None, "ones"):
            return self.table, ant
        a = self.flag_antenna if wl == "flagged" else self.taper_antenna
        z = ant.copy()
        z[:, :, a] = 0
        t = self.table.copy().reshape(self.B, self.A)
        t[:, a] = self.low.reshape(self.B, self.A)[:, a]
        return t.ravel(), z

    def _sane(self, exp, exp_low, weighted_away):
        """The oracle's expectation has NaN in beam 2 and nowhere else for a NaN pair and none otherwise; (sample set 0,
        first channels) the beam of every pair of a higher class differs from that of the all-low table, the other beams
        do not."""
        nan = np.isnan(exp)
        has_nan = "nan" in self.where and not weighted_away
        others = [b for b in range(self.B) if b != NAN_BEAM]
        assert not nan[:, :, others].any() and nan[:, :, NAN_BEAM].all() == has_nan and nan[:, :, NAN_BEAM].any() == has_nan
        if exp_low is None:
            return
        assert not np.isnan(exp_low).any()
        changed = set() if weighted_away else {b for b, _ in self.where.values()}
        nc = exp_low.shape[0]
        for b in range(self.B):
            same = np.array_equal(exp[:nc, :, b], exp_low[:, :, b])
            assert same != (b in changed), (b, sorted(changed))

    def exp(self, i, wl=None):
        """The oracle's matrix-core beams of sample set i (unscaled by s_b: no weighted scenario of that call scales)."""
        assert wl != "taper"

        def make():
            o, nc = self.oracle, min(self.C, 4)
            table, ant = self._inputs(i, wl)
            exp = o.beamform_accumulated(self.op, table, self.dt, self.nt, ant)
            exp_low = o.beamform_accumulated_slab(self.op, self.low, self.dt, self.nt, 0, nc, ant[:nc]) if i == 0 else None
            self._sane(exp, exp_low, wl == "flagged")
            return exp
        return self.once(("exp", i, "ones" if wl is None else wl), make)

    def fexp(self, i, wl=None):
        """The oracle's per-sample beams of the first fnt samples and fnc channels of sample set i, every time step its own
        coefficients (and with them its own class)."""
        def make():
            o, nc, nb = self.oracle, self.fnc, self.fnt // 16
            table, ant = self._inputs(i, wl)
            exp = o.beamform_slab(self.op, table, self.fnt, 0, nc, ant[:nc, :nb])
            exp_low = o.beamform_slab(self.op, self.low, self.fnt, 0, min(nc, 2), ant[:min(nc, 2), :nb]) if i == 0 else None
            self._sane(exp, exp_low, wl == "flagged")
            if wl == "taper":
                exp = (exp * self.taper[None, None, :, None, None]).astype(np.float32)  # powers of two: exact
            return exp
        return self.once(("fexp", i, "ones" if wl is None else wl), make)


_GROUP = {}


def refs_of(oracle, A, B, C, nt, cls, fnt=None):
    key = (A, B, C, nt, cls, fnt)
    if _GROUP.get("key") != key:
        _GROUP.clear()
        _GROUP.update(key=key, refs=Refs(oracle, A, B, C, nt, cls, fnt))
    return _GROUP["refs"]


def within(got, exp, bound, what):
    """(a): NaN exactly where the oracle has NaN, elsewhere within ``bound`` (a number or one per beam) of it."""
    nan = np.isnan(exp)
    bad = np.flatnonzero((np.isnan(got) != nan).ravel())
    assert bad.size == 0, (f"{what}: NaN in {int(np.isnan(got).sum())} places, the oracle in {int(nan.sum())}; first difference at "
                           f"{np.unravel_index(int(bad[0]), exp.shape)}: got {got.ravel()[bad[0]]!r}, oracle {exp.ravel()[bad[0]]!r}")
    err = np.abs(np.where(nan, 0, got.astype(np.float64) - exp))
    over = err - np.broadcast_to(np.asarray(bound, dtype=np.float64).reshape(-1)[None, None, :, None, None], err.shape)
    i = np.unravel_index(int(np.argmax(over)), err.shape)
    print(f"{what}: max |got - oracle| {err.max():.3e}, bound {np.max(bound):.3e}")
    assert over[i] <= 0, f"{what}: |got - oracle| {err[i]:.3e} at {i} (got {got[i]!r}, oracle {exp[i]!r})"


def reference(c, r, kind, i, wl=None):
    """The output of ``kind`` on sample set i (loaded in c, with its weights) from a fresh context, held to (a)."""
    weighted = wl is not None

    def make():
        tag = f"fresh context, {kind}, sample set {i}, weights {wl}"
        if kind == "float":
            v = c.fresh("float", weighted)
            within(v, r.exp(i, wl), 4e-5 * c.A + 1e-6, tag)
            return v
        if kind == "fused":
            f = c.fresh("fused", weighted)
            within(f[:r.fnc], r.fexp(i, wl), (2e-5 * c.A) * r.scale(wl) + 1e-6, tag)
            return f
        v = reference(c, r, "float", i, wl)
        if kind == "power":
            p = c.fresh("power", weighted)
            assert same_bits(p, block_power(v)) is None, (tag, same_bits(p, block_power(v)))
            return p
        assert kind == "q8"
        k = gains_of(v)
        c.set_gains(k)
        q, n = c.fresh("q8", weighted)
        q_exp, n_exp = quantise(v, k)
        finite = [b for b in range(c.B) if not np.isnan(v[:, :, b]).any()]
        assert np.all(n_exp[finite] > 0) and np.all(n_exp[finite] < v[:, :, 0].size), n_exp  # some clip, most do not
        assert np.array_equal(q, q_exp) and np.array_equal(n, n_exp), (tag, first_byte(q, q_exp), n, n_exp)
        return k, q, n
    return r.once((kind, i, wl), make)


def first_byte(got, exp):
    bad = np.flatnonzero(got.ravel() != exp.ravel())
    if bad.size == 0:
        return None
    i = np.unravel_index(int(bad[0]), got.shape)
    return f"{bad.size} of {got.size} bytes differ; first at {i}: got {got[i]}, expected {exp[i]}"


def step(c, r, i, kind, run, wl=None, what=""):
    """One call on sample set i (and the weights ``wl``): ``run()`` makes it and returns its output, which must be the
    fresh context's (b) -- itself held to the oracle (a), so the output is too, at the same bound."""
    c.load(r.ant(i), None if wl is None else r.weights(wl))
    ref = reference(c, r, kind, i, wl)
    what = f"{what}: {kind}, sample set {i}, weights {wl}"
    if kind == "q8":
        k, q_ref, n_ref = ref
        c.set_gains(k)
        q, n = run()
        assert np.array_equal(q, q_ref), (what, first_byte(q, q_ref))
        assert np.array_equal(n, n_ref), (what, "clip counters", n, n_ref)
        return
    got = run()
    if kind == "float":  # (a) on the output itself as well: the NaN places and the figure are then in the failure
        within(got, r.exp(i, wl), 4e-5 * c.A + 1e-6, what)
    elif kind == "fused":
        within(got[:r.fnc], r.fexp(i, wl), (2e-5 * c.A) * r.scale(wl) + 1e-6, what)
    assert same_bits(got, ref) is None, (what, same_bits(got, ref))


def alternate(c, r, first, second):
    """Two graphs on one context, ``first`` captured before ``second`` (after one plain call, which allocates), replayed
    younger, older, younger, older on new samples (and gains)."""
    c.load(r.ant(0))
    c.plain("float")
    graphs = {first: c.capture(first)}
    graphs[second] = c.capture(second)
    for i, kind in enumerate((second, first, second, first)):
        step(c, r, i, kind, lambda: c.replay(graphs[kind], kind), what=f"replay {i + 1} ({first} captured before {second})")
    for g in graphs.values():
        g.close()


def graph_plain_graph(c, r):
    c.load(r.ant(0))
    c.plain("float")
    graph = c.capture("float")
    step(c, r, 0, "float", lambda: c.replay(graph, "float"), what="first replay")
    for i, kind in ((1, "q8"), (1, "fused"), (2, "float")):
        step(c, r, i, kind, lambda: c.plain(kind), what="plain call after a replay")
    step(c, r, 3, "float", lambda: c.replay(graph, "float"), what="replay after plain calls")
    graph.close()


def weights_change_the_class(c, r):
    """The higher-class pair's antenna is flagged (weight 0 in every beam) at capture, so every pair is of the lowest
    class; unflagged on the next replay, so the pair counts (a NaN pair: its beam NaN); then flagged again."""
    c.load(r.ant(0), r.weights("flagged"))
    c.plain("float", weighted=True)
    graph = c.capture("float", weighted=True)
    for i, wl in enumerate(("flagged", "ones", "flagged", "ones")):
        step(c, r, i, "float", lambda: c.replay(graph, "float"), wl=wl, what=f"weighted replay {i + 1}")
    graph.close()


SCENARIOS = {
    "float then q8": lambda c, r: alternate(c, r, "float", "q8"),
    "q8 then float": lambda c, r: alternate(c, r, "q8", "float"),
    "float then power": lambda c, r: alternate(c, r, "float", "power"),
    "power then float": lambda c, r: alternate(c, r, "power", "float"),
    "graph, plain calls, graph": graph_plain_graph,
    "weights change the class": weights_change_the_class,
    "fused then float": lambda c, r: alternate(c, r, "fused", "float"),  # they share the word of time step 0
    "float then fused": lambda c, r: alternate(c, r, "float", "fused"),
}


@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("A,B,C,nt,depth", MC_SHAPES)
def test_matrix_core_calls_replayed_among_other_calls_of_their_context(gpu, oracle, case, A, B, C, nt, depth, cls, scenario):
    r = refs_of(oracle, A, B, C, nt, cls)
    c = case(A, B, C, nt, r.table)
    SCENARIOS[scenario](c, r)
    if depth:  # (last: it captures, which the context remembers)
        c.prove_depth(depth, lambda s: c.enqueue("float", stream=s))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cls", CLASSES + ("all",))
def test_fused_call_of_two_chunks_replayed(gpu, oracle, case, cls, weighted):
    """One graph is enough here: with more than 32768 pairs the terms table holds fewer than 256 time steps, so a call of
    256 is two chunks, each with its terms launch and its beamformer launch on the SAME class words.  The captured graph
    itself must show the 240 + 16 split (the terms launches have one row of workgroups per time step, one more with
    weights; the beamformer launches 16 beam groups per 16-sample block)."""
    A, B, C, nt = TWO_CHUNKS
    wl = "taper" if weighted else None
    r = refs_of(oracle, A, B, C, nt, cls, fnt=nt)
    c = case(A, B, C, nt, r.table, fnt=nt)
    c.load(r.ant(0), r.weights(wl) if weighted else None)
    c.plain("fused", weighted)
    others = []
    nodes = hip_graph.launches(c.s, lambda: c.enqueue("fused", weighted=weighted, stream=c.s.handle), others)
    c.s.synchronize()
    grids = sorted(g for g, _ in nodes)
    terms = [g for g in grids if g[1] > 1]
    clearing = [g for g in grids if g == (1, 1, 1)]  # at most one workgroup in front of each chunk: its words
    assert [g[1] for g in terms] == [16 + weighted, 240 + weighted], grids
    assert [g for g in grids if g[1] == 1 and g != (1, 1, 1)] == [(16, 1, 1), (16 * 15, 1, 1)], grids
    assert len(grids) == 4 + len(clearing) and len(clearing) in (0, 2) and others == [], (grids, others)
    graph = c.capture("fused", weighted)
    for i in range(3):
        step(c, r, i, "fused", lambda: c.replay(graph, "fused"), wl=wl, what=f"replay {i + 1} of the two-chunk call")
    graph.close()


@pytest.mark.parametrize("A,B", [(64, 16), (130, 20)])
def test_a_captured_call_is_its_two_kernels_and_the_clearing_of_its_words(gpu, oracle, case, A, B):
    """What capturing costs: the first captured call of a context is the two kernel launches of the plain call and one
    workgroup in front that clears the class words of its time steps, and so is every later one; no other node."""
    table, _, _ = class_table(A, B, "slow")
    c = case(A, B, 2, 32, table)
    c.load(c.ant, np.ones((B, A), np.float32))
    plain = {}
    for kind, weighted in (("float", False), ("float", True), ("q8", False), ("power", True), ("fused", False), ("fused", True)):
        plain[kind, weighted] = c.plain(kind, weighted)  # before anything is captured
    for (kind, weighted), ref in plain.items():
        others = []
        nodes = hip_graph.launches(c.s, lambda: c.enqueue(kind, weighted=weighted, stream=c.s.handle), others)
        c.s.synchronize()
        grids = sorted(g for g, _ in nodes)
        assert len(grids) == 3 and grids[0] == (1, 1, 1) and others == [], (kind, weighted, grids, others)
        got = c.plain(kind, weighted)  # after: the same bits
        for g, r in zip(got if kind == "q8" else (got,), ref if kind == "q8" else (ref,)):
            assert np.array_equal(g.view(np.uint8), r.view(np.uint8)), (kind, weighted)
