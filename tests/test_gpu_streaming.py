"""GPU parity of the streaming path (BASELINE configs[4]): the hipGraph replayed per tick, one node and TWO nodes (terms
pre-pass + generator, what slabs of >= 2 GiB and ``form = 3`` build -- the path ``bench.py``'s full-tensor
``streaming_cfg5`` figure runs on), ticks by time index, by fDeltaTime and by (current, reference), a new delay table
landing between ticks from the host or from DEVICE memory (``dcs_bf_stream_tick_*_from_global``: a gather node in the
replayed graph; configs[3] + configs[4] composed).

Everything is compared with the CPU oracle evaluated at the tick's own fDeltaTime and table -- never with another GPU
launch.  Bar as in test_gpu_parity.py: fp32 within 1 ULP, binary16 within one binary16 ulp of RN-even(oracle).  Contexts,
streams and buffers belong to a StreamCase that the fixture closes; every slab has a guard behind it.
"""
from functools import partial

import numpy as np
import pytest

from conftest import rand_table
from helpers.device_buffers import closed_after
from helpers.parity_case import GeneratorCase, check_1ulp, ordered_distance

pytestmark = pytest.mark.gpu


class StreamCase(GeneratorCase):
    """A generator, the stream its ticks run on and the CoefficientStreams begun on it: close() ends them before the
    generator and the buffers go."""

    def __init__(self, gpu, bp, table=None, tuning=None):
        super().__init__(gpu, bp, table, tuning)
        self.stream, self.begun = gpu.Stream(), []

    def begin(self, out, c0, nc, bitwidth=1):
        """stream_begin into the Tensor ``out``, whose fill (made on the null stream) is complete first."""
        self.gpu.synchronize()
        self.begun.append(self.g.stream_begin(out.ptr, out.nbytes, c0, nc, self.stream, bitwidth=bitwidth))
        return self.begun[-1]

    def close(self):
        try:
            self.stream.synchronize()
            for st in self.begun:
                st.end()
        finally:
            super().close()


@pytest.fixture
def streaming(gpu):
    yield from closed_after(partial(StreamCase, gpu))


def _check_slab(oracle, got, exp, tag):
    """got: floats or halves off the device; exp: the oracle's fp32 slab; NaN exactly where the verifier has NaN, the rest
    within the bar."""
    fin = ~np.isnan(exp)
    assert np.array_equal(np.isnan(got), ~fin), tag
    if got.dtype == np.float32:
        check_1ulp(oracle, np.where(fin, got, 0).astype(np.float32), np.where(fin, exp, 0).astype(np.float32), tol=None, tag=tag)
    else:
        assert ordered_distance(np.where(fin, got, 0).astype(np.float16), np.where(fin, exp, 0).astype(np.float16)) <= 1, tag


def _rows(gpu, out, first, shape):
    """Rows of a slab too large to come back whole: ``shape`` floats from row ``first`` of the Tensor ``out``."""
    host = np.empty(shape, dtype=np.float32)
    gpu.memcpy_dtoh(host, out.ptr + first * int(np.prod(out.shape[2:])) * 4)
    return host


def _tables(n_pairs, seeds, slow_in=()):
    """Seeded tables; those listed in ``slow_in`` carry slow-class pairs (|fRotation| far beyond 32000, a rate of
    1e38, an infinity, a NaN): with the terms table it is the PRE-PASS node that writes those tiles into d_out."""
    out = []
    for i, s in enumerate(seeds):
        t = rand_table(n_pairs, seed=s)
        if i in slow_in:
            t["fDelayRate_sps"][5 % n_pairs] = 1e-2
            t["fDelayRate_sps"][(n_pairs // 2 + 3) % n_pairs] = 1e38
            t["fPhase_rad"][(n_pairs - 2) % n_pairs] = np.inf
            t["fDelay_s"][(n_pairs // 3) % n_pairs] = np.nan
        out.append(t)
    return out


@pytest.mark.parametrize("bitwidth,math_mode", [(1, 0), (0, 0), (0, 4)])
def test_two_node_streaming_graph_every_tick_against_the_oracle(streaming, oracle, bitwidth, math_mode):
    """``form = 3`` before ``stream_begin`` builds the two-node graph (bf_terms_kernel -> tiled generator reading the
    terms table) at a small shape.  Ticks by time index, by fDeltaTime and by (current, reference); a new HOST table
    on some ticks (one of them with slow-class pairs, so the pre-pass node's own stores into d_out happen inside the
    graph) and a new DEVICE table on others; the whole slab after every tick against the oracle."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times

    bp = BeamformerParameters(NR_CHANNELS=96, NR_STATIONS=8, NR_BEAMS=40)
    op = oracle.params_from(bp)
    c0, nc = 16, 64
    tables = _tables(bp.n_pairs, (131, 132, 133, 134), slow_in=(1, 3))
    c = streaming(bp, tuning=dict(form=3, math_mode=math_mode))
    d_tables = [c.upload(t) for t in tables]
    c.g.upload_delays(tables[0], stream=c.stream)
    out = c.tensor(1, nc, bitwidth)
    st = c.begin(out, c0, nc, bitwidth)
    cur = 0
    ref = (41, 999_800_000)
    #        kind  time                      table source
    plan = [("t", 0, None), ("t", 9, ("host", 1)), ("dt", 200e-6, None), ("at", (42, 100), ("dev", 2)), ("dt", 0.37, ("dev", 3)),
            ("t", 255, None), ("at", (41, 999_900_000), ("host", 0)), ("dt", -2e-4, ("dev", 1)), ("t", 1000, ("host", 2)),
            ("dt", 1.5, ("dev", 0)), ("dt", 400e-6, ("dev", 3)), ("t", 18, ("host", 1)), ("t", 7, None)]
    for tick, (kind, when, src) in enumerate(plan):
        host_tbl = None
        if src is not None:
            cur = src[1]
            host_tbl = tables[cur] if src[0] == "host" else None
        dev = src is not None and src[0] == "dev"
        out.refill(stream=c.stream)
        if kind == "t":
            dt = delta_times(bp, when, 1)[0]
            st.tick_from_global(when, d_tables[cur]) if dev else st.tick(when, host_tbl)
        elif kind == "dt":
            dt = np.float32(when)
            st.tick_dt_from_global(when, d_tables[cur]) if dev else st.tick_dt(when, host_tbl)
        else:
            dt = oracle.ts_diff(ref, when)
            st.tick_at_from_global(when, ref, d_tables[cur]) if dev else st.tick_at(when, ref, host_tbl)
        c.stream.synchronize()
        _check_slab(oracle, out.read(), oracle.generate_dt(op, tables[cur], [dt], c0, nc), (tick, kind, when, src))


def test_streaming_from_a_global_device_table_changing_every_tick(streaming, oracle):
    """configs[3] + configs[4] composed: the context owns beams [off, off + B_loc) of a GLOBAL [A][B_total] table that
    sits in device memory (where an RCCL broadcast lands it) and CHANGES ON EVERY TICK; the tick gathers its slice
    inside the replayed graph.  Both graph shapes (one node / two nodes behind the gather), both widths; each tick's
    slab against the oracle on that tick's slice.  Ticks are queued back to back in bursts (no host
    synchronisation between them) into separate output slabs, so the double-buffered table is exercised while
    earlier replays are still in flight."""
    from dc_sand_amd import BeamformerParameters, _lib

    A, B_total, C = 6, 50, 40
    rng = np.random.default_rng(77)
    n_ticks = 9
    globs = [rand_table(A * B_total, seed=900 + k) for k in range(n_ticks)]
    globs[4]["fDelayRate_sps"][3 * B_total + 20] = 2e-2  # a slow-class pair inside the second shard below
    for (off, bl), form, bw in (((0, 16), 0, 1), ((16, 34), 3, 1), ((7, 9), 3, 0), ((49, 1), 0, 0)):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=bl)
        op = oracle.params_from(bp)
        c = streaming(bp, tuning=dict(form=form) if form else None)
        d_globs = [c.upload(t) for t in globs]
        c.g.set_delays_from_global(d_globs[0], B_total, off, stream=c.stream)
        c0, nc = 3, 30
        outs = [c.tensor(1, nc, bw) for k in range(n_ticks)]
        streams = [c.begin(outs[k], c0, nc, bw) for k in range(n_ticks)]
        dts = [np.float32(k * 200e-6 + rng.uniform(0, 1e-5)) for k in range(n_ticks)]
        for k in range(n_ticks):  # one burst: nine graph launches, nine different tables, no synchronisation
            streams[k].tick_dt_from_global(float(dts[k]), d_globs[k], B_total, off)
        c.stream.synchronize()
        for k in range(n_ticks):
            local = np.ascontiguousarray(globs[k].reshape(A, B_total)[:, off:off + bl]).ravel()
            _check_slab(oracle, outs[k].read(), oracle.generate_dt(op, local, [dts[k]], c0, nc), (off, bl, form, bw, k))
        # the argument checks of the device-table ticks
        with pytest.raises(_lib.DcsError) as e:
            streams[0].tick_dt_from_global(0.0, d_globs[0], B_total, B_total - bl + 1)  # slice runs past the table
        assert e.value.status == _lib.DCS_ERR_OUT_OF_RANGE
        with pytest.raises(_lib.DcsError) as e:
            streams[0].tick_dt_from_global(0.0, int(d_globs[0]) + 4, B_total, off)  # not 16-byte aligned
        assert e.value.status == _lib.DCS_ERR_INVALID_ARGUMENT


def test_host_table_on_every_tick_never_reuses_a_staging_buffer_in_flight(gpu, streaming, oracle):
    """A new HOST table with every tick, twelve ticks queued back to back (more than the ring of four pinned staging
    buffers): the caller's array may be overwritten as soon as the tick call returns, and every slab still shows
    its own tick's table."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=48, NR_STATIONS=4, NR_BEAMS=96)
    op = oracle.params_from(bp)
    n_ticks = 12
    tables = [rand_table(bp.n_pairs, seed=500 + k) for k in range(n_ticks)]
    c = streaming(bp)
    c.g.upload_delays(tables[0], stream=c.stream)
    out, keep = c.tensor(1), c.tensor(n_ticks)  # every tick's slab is copied aside on the same stream
    st = c.begin(out, 0, bp.NR_CHANNELS)
    scratch = np.empty_like(tables[0])
    for k in range(n_ticks):
        scratch[:] = tables[k]
        out.refill(stream=c.stream)
        st.tick_dt(k * 200e-6, scratch)
        scratch["fDelay_s"][:] = np.nan  # the call has copied it: the caller's buffer is free again
        gpu.memcpy_dtod(keep.ptr + k * out.nbytes, out.ptr, out.nbytes, c.stream)
    c.stream.synchronize()
    out.guard_untouched()
    kept = keep.read()
    for k in range(n_ticks):
        _check_slab(oracle, kept[k:k + 1], oracle.generate_dt(op, tables[k], [np.float32(k * 200e-6)]), k)


def test_config5_full_tensor_two_node_graph_every_element(gpu, streaming, oracle, record_property):
    """BASELINE configs[4] at FULL size: ``stream_begin`` over the whole 64 x 1024 x 32768 tensor (16 GiB >= 2 GiB: the
    two-node graph, the code ``bench.py``'s ``streaming_cfg5.full_tensor_period_us`` times), three ticks at a 200 us
    model cadence -- the second with a new host table, the third with a new DEVICE table --, then EVERY one of the 2^32
    floats of the last tick against the verifier (<= 1 ULP, both readings of cos(float))."""
    import time

    from dc_sand_amd import BeamformerParameters
    from helpers.every_element import compare_every_element

    bp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=64, NR_BEAMS=1024)
    op = oracle.params_from(bp)
    tables = [rand_table(bp.n_pairs, seed=s) for s in (71, 72, 73)]
    c = streaming(bp)
    d_tab = c.upload(tables[2])
    c.g.upload_delays(tables[0], stream=c.stream)
    out = c.tensor(1)
    assert out.nbytes == c.g.output_bytes(1, 1) == 16 * 2 ** 30
    st = c.begin(out, 0, bp.NR_CHANNELS)
    row = (1, 1) + out.shape[2:]
    dts = [np.float32(k * 200e-6) for k in (1, 2, 3)]
    st.tick_dt(float(dts[0]))
    c.stream.synchronize()
    for ch in (0, 12345, 32767):  # sampled rows of the earlier ticks, everything of the last
        _check_slab(oracle, _rows(gpu, out, ch, row), oracle.generate_dt(op, tables[0], [dts[0]], ch, 1), ch)
    out.refill(stream=c.stream)
    st.tick_dt(float(dts[1]), tables[1])
    c.stream.synchronize()
    for ch in (1, 20000, 32766):
        _check_slab(oracle, _rows(gpu, out, ch, row), oracle.generate_dt(op, tables[1], [dts[1]], ch, 1), ch)
    out.refill(stream=c.stream)
    st.tick_dt_from_global(float(dts[2]), d_tab)
    c.stream.synchronize()
    out.guard_untouched()
    t0 = time.perf_counter()
    res = compare_every_element(gpu, oracle, out.ptr, op, tables[2], dts[2], bp.NR_CHANNELS, bp.n_pairs)
    wall = time.perf_counter() - t0
    n = bp.NR_CHANNELS * bp.n_pairs * 2
    for r in (0, 1):
        h = res[r]["hist"]
        assert sum(h) == n == 2 ** 32
        assert h[2] == 0 and h[3] == 0 and res[r]["max_ulp"] <= 1, (r, res[r])
    summary = (f"config 5, full tensor through the two-node streaming graph, third tick (device table), all {n} floats: "
               f"{res[0]['hist'][1]} at 1 ULP, 0 beyond (float-libm reading: {res[1]['hist'][1]}, 0 beyond); {wall:.1f} s wall")
    print(summary)
    record_property("config5_full_compare", summary)


def test_streaming_graph_ticks_with_table_updates(streaming, oracle):
    """BASELINE configs[4] plumbing: hipGraph-captured launch replayed per tick
    with a new time index, and a new delay table landing between ticks
    (double-buffered); every tick's slab equals the oracle's."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=96, NR_STATIONS=8, NR_BEAMS=40)
    op = oracle.params_from(bp)
    c0, nc = 16, 64
    tables = [rand_table(bp.n_pairs, seed=s) for s in (31, 32, 33)]
    c = streaming(bp, tables[0])
    out = c.tensor(1, nc)
    st = c.begin(out, c0, nc)
    cur = 0
    for tick, t in enumerate([0, 1, 5, 7, 9, 18, 255, 256, 1000]):
        new = None
        if tick in (3, 4, 7):
            cur = (cur + 1) % 3
            new = tables[cur]
        out.refill(stream=c.stream)
        st.tick(t, new)
        c.stream.synchronize()
        _check_slab(oracle, out.read(), oracle.generate(op, tables[cur], t, 1, c0, nc), (tick, t))


def test_config5_streaming_at_the_200us_slab(gpu, streaming, oracle):
    """BASELINE configs[4] at size: 64 x 1024 pairs x the 2560-channel slab that sustains the 200 us cadence
    (1.34 GB per tick), hipGraph replay, MODEL time advancing 200 us per tick (dcs_bf_stream_tick_dt, and
    dcs_bf_stream_tick_at across a seconds boundary), a new delay table landing between ticks; sampled rows of
    every tick against the oracle evaluated at the same fDeltaTime."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=64, NR_BEAMS=1024)
    op = oracle.params_from(bp)
    c0, nc = 4096, 2560
    tables = [rand_table(bp.n_pairs, seed=s) for s in (61, 62)]
    c = streaming(bp, tables[0])
    out = c.tensor(1, nc)
    st = c.begin(out, c0, nc)
    row = (1, 1) + out.shape[2:]
    cur = 0
    ref = (777, 999_500_000)  # 0.5 ms before a seconds boundary: ticks 3.. lie beyond it
    for tick in range(1, 7):
        new = None
        if tick == 3:
            cur, new = 1, tables[1]
        out.refill(stream=c.stream)
        if tick % 2:
            dt = np.float32(tick * 200e-6)
            st.tick_dt(dt, new)
        else:
            ns = ref[1] + tick * 200_000
            now = (ref[0] + ns // 10 ** 9, ns % 10 ** 9)  # a normalised wall-clock reading
            dt = oracle.ts_diff(ref, now)
            assert abs(float(dt) - tick * 200e-6) < 1e-7
            st.tick_at(now, ref, new)
        c.stream.synchronize()
        out.guard_untouched()
        for cl in (0, 1279, nc - 1):
            _check_slab(oracle, _rows(gpu, out, cl, row), oracle.generate_dt(op, tables[cur], [dt], c0 + cl, 1), (tick, cl))
    out.refill(stream=c.stream)
    st.tick(300)  # the time-index form still works on the same stream object
    c.stream.synchronize()
    out.guard_untouched()
    _check_slab(oracle, _rows(gpu, out, 0, row), oracle.generate(op, tables[cur], 300, 1, c0, 1), 300)


def test_streaming_seeded_fuzz_of_tick_kinds_slabs_and_table_updates(streaming, oracle):
    """12 seeded streams (hipGraph replay, BASELINE configs[4]'s plumbing) x 8 ticks each: a random channel slab and
    output width per stream, every tick by time index, by fDeltaTime or by a (current, reference) pair, a new delay table
    landing with some of the ticks (double-buffered), the slab read back after every tick: fp32 within 1 ULP of the
    verifier at that tick's time and table, fp16 within one binary16 ulp of its RN-even image."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times

    rng = np.random.default_rng(20261009)
    for n in range(12):
        A, B, C = int(rng.integers(1, 7)), int(rng.integers(1, 40)), int(rng.integers(2, 60))
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        op = oracle.params_from(bp)
        table = rand_table(bp.n_pairs, seed=11000 + n)
        c0 = int(rng.integers(0, C))
        nc = int(rng.integers(1, C - c0 + 1))
        bw = int(rng.integers(0, 2))
        c = streaming(bp)
        c.g.upload_delays(table, stream=c.stream)
        out = c.tensor(1, nc, bw)
        s_ = c.begin(out, c0, nc, bw)
        for tick in range(8):
            new = None
            if rng.integers(0, 3) == 0:
                table = rand_table(bp.n_pairs, seed=12000 + 10 * n + tick)
                new = table
            kind = int(rng.integers(0, 3))
            out.refill(stream=c.stream)
            if kind == 0:
                t = int(rng.integers(0, 5000))
                s_.tick(t, new_table=new)
                dt = delta_times(bp, t, 1)[0]
            elif kind == 1:
                dt = np.float32(rng.uniform(-2.0, 2.0))
                s_.tick_dt(float(dt), new_table=new)
            else:
                ref = (int(rng.integers(0, 10 ** 6)), int(rng.integers(0, 10 ** 9)))
                cur = (ref[0] + int(rng.integers(0, 3)), int(rng.integers(0, 10 ** 9)))
                s_.tick_at(cur, ref, new_table=new)
                dt = oracle.ts_diff(ref, cur)
            c.stream.synchronize()
            _check_slab(oracle, out.read(), oracle.generate_dt(op, table, [dt], c0, nc), (n, tick, kind, A, B, C, c0, nc, bw, float(dt)))
