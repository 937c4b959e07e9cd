"""GPU tests of staged delay tables (``dcs_bf_stream_stage_table*``): the next tick's table lands on an internal stream
while the current tick runs, and the next tick without a table of its own makes it current.

Every slab is compared with the CPU oracle evaluated at that tick's own fDeltaTime and table -- never with another GPU
launch.  Bar as in test_gpu_parity.py: fp32 within 1 ULP, binary16 within one binary16 ulp of RN-even(oracle), NaN
exactly where the oracle has NaN.
"""
import time

import numpy as np
import pytest

from conftest import rand_table

pytestmark = pytest.mark.gpu


def _ordered16(u):
    return np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)


def _check_slab(oracle, gpu, buf, exp, bitwidth, tag):
    fin = ~np.isnan(exp)
    if bitwidth == 1:
        got = np.empty(exp.shape, dtype=np.float32)
        gpu.memcpy_dtoh(got, buf)
        assert np.array_equal(np.isnan(got), ~fin), tag
        mx, n_over, first = oracle.max_ulp(np.where(fin, got, 0).astype(np.float32), np.where(fin, exp, 0).astype(np.float32), 1)
        assert n_over == 0, (tag, mx, n_over, first)
    else:
        h16 = np.empty(exp.shape, dtype=np.float16)
        gpu.memcpy_dtoh(h16, buf)
        assert np.array_equal(np.isnan(h16), ~fin), tag
        have = np.where(fin, h16, 0).astype(np.float16).view(np.uint16).astype(np.int32)
        want = np.where(fin, exp, 0).astype(np.float16).view(np.uint16).astype(np.int32)
        assert np.abs(_ordered16(have) - _ordered16(want)).max() <= 1, tag


def _with_slow_pairs(t):
    """Slow-class pairs (|fRotation| far beyond 32000, a rate of 1e38, an infinity, a NaN)."""
    n = t.size
    t["fDelayRate_sps"][5 % n] = 1e-2
    t["fDelayRate_sps"][(n // 2 + 3) % n] = 1e38
    t["fPhase_rad"][(n - 2) % n] = np.inf
    t["fDelay_s"][(n // 3) % n] = np.nan
    return t


def _small_setup(gpu, bp, bitwidth, form=0, math_mode=0):
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    g = SteeringCoefficientGenerator(bp)
    if form or math_mode:
        g.set_tuning(form=form, math_mode=math_mode)
    stream = gpu.Stream()
    slab = bp.NR_CHANNELS * bp.n_pairs * (8 if bitwidth == 1 else 4)
    buf = gpu.mem_alloc(slab)
    return g, stream, slab, buf


@pytest.mark.parametrize("form", [0, 3])
@pytest.mark.parametrize("bitwidth,math_mode", [(1, 0), (0, 0), (0, 4)])
def test_back_to_back_staged_host_ticks(gpu, oracle, bitwidth, math_mode, form):
    """Thirteen ticks queued without synchronisation; after enqueuing tick k the table of tick k + 1 is staged from a
    host array that is scribbled over as soon as the call returns (twelve stagings: three times round the ring of four
    pinned buffers).  Each slab is copied aside on the same stream and must show its own tick's table.  ``form = 3``
    builds the two-node graph (terms pre-pass + generator); one staged table carries slow-class pairs."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=48, NR_STATIONS=4, NR_BEAMS=96)
    op = oracle.params_from(bp)
    n_ticks = 13
    tables = [rand_table(bp.n_pairs, seed=1300 + k) for k in range(n_ticks)]
    _with_slow_pairs(tables[6])
    g, stream, slab, buf = _small_setup(gpu, bp, bitwidth, form, math_mode)
    keep = gpu.mem_alloc(slab * n_ticks)
    g.upload_delays(tables[0], stream=stream)
    st = g.stream_begin(buf, slab, 0, bp.NR_CHANNELS, stream, bitwidth=bitwidth)
    scratch = np.empty_like(tables[0])
    dts = [np.float32(k * 200e-6 + 3e-6) for k in range(n_ticks)]
    for k in range(n_ticks):
        st.tick_dt(float(dts[k]))  # ticks 1.. consume the table staged after the previous tick
        gpu.memcpy_dtod(int(keep) + k * slab, buf, slab, stream)
        if k + 1 < n_ticks:
            scratch[:] = tables[k + 1]
            st.stage_table(scratch)
            scratch["fDelay_s"][:] = np.nan  # copied into the ring: the caller's array is free again
            scratch["fPhase_rad"][:] = 1e30
    stream.synchronize()
    for k in range(n_ticks):
        exp = oracle.generate_dt(op, tables[k], [dts[k]])
        _check_slab(oracle, gpu, int(keep) + k * slab, exp, bitwidth, (form, bitwidth, math_mode, k))
    st.end()
    g.close()
    buf.free()
    keep.free()


def test_back_to_back_staged_pinned_ticks(gpu, oracle):
    """The same with ``pinned=True``: twelve distinct ``pagelocked_empty`` tables, copied from where they are."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.device import pagelocked_empty
    from dc_sand_amd.parameters import delay_vals_dtype

    bp = BeamformerParameters(NR_CHANNELS=40, NR_STATIONS=8, NR_BEAMS=24)
    op = oracle.params_from(bp)
    n_ticks = 13
    tables = [rand_table(bp.n_pairs, seed=1400 + k) for k in range(n_ticks)]
    _with_slow_pairs(tables[3])
    pinned = []
    for t in tables:
        p = pagelocked_empty(bp.n_pairs, delay_vals_dtype)
        p[:] = t
        pinned.append(p)
    g, stream, slab, buf = _small_setup(gpu, bp, 1)
    keep = gpu.mem_alloc(slab * n_ticks)
    g.upload_delays(tables[0], stream=stream)
    st = g.stream_begin(buf, slab, 0, bp.NR_CHANNELS, stream)
    dts = [np.float32(k * 200e-6) for k in range(n_ticks)]
    for k in range(n_ticks):
        st.tick_dt(float(dts[k]))
        gpu.memcpy_dtod(int(keep) + k * slab, buf, slab, stream)
        if k + 1 < n_ticks:
            st.stage_table(pinned[k + 1], pinned=True)
    stream.synchronize()
    for k in range(n_ticks):
        _check_slab(oracle, gpu, int(keep) + k * slab, oracle.generate_dt(op, tables[k], [dts[k]]), 1, k)
    st.end()
    g.close()
    buf.free()
    keep.free()


def _busy(gpu, stream, ms):
    """Queue at least ``ms`` of generator work on ``stream``; returns (start, stop) events around it and what to free."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import SteeringCoefficientGenerator, simulate_input

    bp = BeamformerParameters(NR_CHANNELS=512, NR_STATIONS=64, NR_BEAMS=1024)
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(simulate_input(bp), stream=stream)
    nbytes = g.output_bytes(1, 4)
    out = gpu.mem_alloc(nbytes)
    # calibrate on warm launches: the fastest of three, so that the queue is long enough whatever the first one cost
    g.generate(out, nbytes, t0=1, nt=4, stream=stream)
    e0, e1 = gpu.Event(), gpu.Event()
    per = []
    for _ in range(3):
        e0.record(stream)
        g.generate(out, nbytes, t0=1, nt=4, stream=stream)
        e1.record(stream)
        e1.synchronize()
        per.append(e1.elapsed_ms_since(e0))
    n = int(np.ceil(1.5 * ms / max(min(per), 1e-3))) + 1
    e0.record(stream)
    for i in range(n):
        g.generate(out, nbytes, t0=1 + i, nt=4, stream=stream)
    e1.record(stream)
    return e0, e1, (g, out)


@pytest.mark.parametrize("bitwidth", [1, 0])
def test_staging_from_a_global_table_waits_for_its_ready_event(gpu, oracle, bitwidth):
    """A beam-sharded global table (``nr_beams_total = 3 * nr_beams``, non-zero ``beam_offset``) is WRITTEN on another
    stream behind >= 10 ms of queued work, and the producer records ``ready_event`` there.  The buffer held another
    table before, so a gather that ignored the event would stage stale beams.  The consuming ticks show the new table;
    a second staging without an event (the table already complete) works too."""
    from dc_sand_amd import BeamformerParameters

    A, nb = 6, 20
    B_total, off = 3 * nb, nb + 3
    bp = BeamformerParameters(NR_CHANNELS=36, NR_STATIONS=A, NR_BEAMS=nb)
    op = oracle.params_from(bp)
    stale, fresh, second = (rand_table(A * B_total, seed=s) for s in (1501, 1502, 1503))
    _with_slow_pairs(fresh)
    d_glob = gpu.mem_alloc(stale.nbytes)
    d_fresh = gpu.mem_alloc(fresh.nbytes)
    d_second = gpu.mem_alloc(second.nbytes)
    gpu.memcpy_htod(d_glob, stale)
    gpu.memcpy_htod(d_fresh, fresh)
    gpu.memcpy_htod(d_second, second)
    local = lambda t: np.ascontiguousarray(t.reshape(A, B_total)[:, off:off + nb]).ravel()  # noqa: E731

    g, stream, slab, buf = _small_setup(gpu, bp, bitwidth)
    keep = gpu.mem_alloc(slab * 3)
    g.set_delays_from_global(d_glob, B_total, off, stream=stream)
    st = g.stream_begin(buf, slab, 0, bp.NR_CHANNELS, stream, bitwidth=bitwidth)
    stream.synchronize()

    producer = gpu.Stream()
    b0, b1, busy_keep = _busy(gpu, producer, 10.0)
    gpu.memcpy_dtod(d_glob, d_fresh, fresh.nbytes, producer)  # the new table lands only after the busy work
    ready = gpu.Event().record(producer)
    dts = [np.float32(1e-4), np.float32(3e-4), np.float32(5e-4)]
    st.tick_dt(float(dts[0]))  # the table set before staging
    gpu.memcpy_dtod(int(keep), buf, slab, stream)
    st.stage_table_from_global(d_glob, B_total, off, ready_event=ready)
    st.tick_dt(float(dts[1]))
    gpu.memcpy_dtod(int(keep) + slab, buf, slab, stream)
    stream.synchronize()
    producer.synchronize()
    assert b1.elapsed_ms_since(b0) >= 10.0  # the event really was recorded behind >= 10 ms of work
    st.stage_table_from_global(int(d_second), B_total, off)  # no event: the table is already complete
    st.tick_dt(float(dts[2]))
    gpu.memcpy_dtod(int(keep) + 2 * slab, buf, slab, stream)
    stream.synchronize()
    for k, tbl in enumerate((stale, fresh, second)):
        _check_slab(oracle, gpu, int(keep) + k * slab, oracle.generate_dt(op, local(tbl), [dts[k]]), bitwidth, (bitwidth, k))
    st.end()
    g.close()
    for d in (buf, keep, d_glob, d_fresh, d_second, busy_keep[1]):
        d.free()
    busy_keep[0].close()


def test_staging_semantics(gpu, oracle):
    """A tick with its own table while one is staged is refused (status -1) and enqueues nothing, and the next plain
    tick takes the staged table; a tick that fails its own checks consumes nothing; the last table staged wins;
    generate on the context between staging and tick sees the old table, after the tick the new one; ``end()`` with a
    table staged but never consumed leaves the context on its table."""
    from dc_sand_amd import BeamformerParameters, _lib

    bp = BeamformerParameters(NR_CHANNELS=24, NR_STATIONS=5, NR_BEAMS=12)
    op = oracle.params_from(bp)
    T = [rand_table(bp.n_pairs, seed=1600 + k) for k in range(8)]
    g, stream, slab, buf = _small_setup(gpu, bp, 1)
    full = gpu.mem_alloc(slab)
    d_t = gpu.mem_alloc(T[7].nbytes)
    gpu.memcpy_htod(d_t, T[7])
    g.upload_delays(T[0], stream=stream)
    st = g.stream_begin(buf, slab, 0, bp.NR_CHANNELS, stream)

    def tick_shows(dt, table, tag):
        st.tick_dt(dt)
        stream.synchronize()
        _check_slab(oracle, gpu, buf, oracle.generate_dt(op, table, [np.float32(dt)]), 1, tag)

    def context_shows(dt, table, tag):
        g.generate_dt(full, slab, [dt], stream=stream)
        stream.synchronize()
        _check_slab(oracle, gpu, full, oracle.generate_dt(op, table, [np.float32(dt)]), 1, tag)

    tick_shows(1e-4, T[0], "before any staging")
    st.stage_table(T[1])
    for refused in (lambda: st.tick_dt(2e-4, T[2]), lambda: st.tick(3, T[2]), lambda: st.tick_at((1, 0), (0, 0), T[2]),
                    lambda: st.tick_dt_from_global(2e-4, d_t), lambda: st.tick_from_global(3, d_t),
                    lambda: st.tick_at_from_global((1, 0), (0, 0), d_t)):
        with pytest.raises(_lib.DcsError) as e:
            refused()
        assert e.value.status == _lib.DCS_ERR_INVALID_ARGUMENT == -1
    tick_shows(2e-4, T[1], "staged table after refused ticks")

    st.stage_table(T[2])
    with pytest.raises(_lib.DcsError):
        st.tick(2**64 - 1)  # out of range for dcs_bf_delta_times: nothing consumed
    tick_shows(3e-4, T[2], "staged table after a failed tick")

    st.stage_table(T[3])
    st.stage_table(T[4])
    tick_shows(4e-4, T[4], "last staged wins")

    st.stage_table(T[5])
    context_shows(5e-4, T[4], "context before the consuming tick")
    tick_shows(6e-4, T[5], "consuming tick")
    context_shows(7e-4, T[5], "context after the consuming tick")

    st.stage_table_from_global(d_t, bp.NR_BEAMS, 0)
    st.stage_table(T[6])
    st.end()  # T[6] staged, never consumed: dropped
    context_shows(8e-4, T[5], "context after end() with a pending table")
    g.close()
    for d in (buf, full, d_t):
        d.free()


def test_staging_and_ticking_never_wait_on_the_host(gpu, oracle):
    """>= 20 ms of generate work queued on the caller's stream (timed with device events), then twelve pinned stage +
    tick calls: their host wall time is under half the queued time -- no call waits for the running tick or the queue
    -- and every slab still matches the oracle afterwards."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.device import pagelocked_empty
    from dc_sand_amd.parameters import delay_vals_dtype

    bp = BeamformerParameters(NR_CHANNELS=32, NR_STATIONS=16, NR_BEAMS=16)
    op = oracle.params_from(bp)
    n = 12
    tables = [rand_table(bp.n_pairs, seed=1700 + k) for k in range(n + 1)]
    pinned = []
    for t in tables:
        p = pagelocked_empty(bp.n_pairs, delay_vals_dtype)
        p[:] = t
        pinned.append(p)
    g, stream, slab, buf = _small_setup(gpu, bp, 1)
    keep = gpu.mem_alloc(slab * n)
    g.upload_delays(tables[0], stream=stream)
    st = g.stream_begin(buf, slab, 0, bp.NR_CHANNELS, stream)
    st.stage_table(pinned[0], pinned=True)  # the first staging creates the internal stream: outside the timed part
    st.tick_dt(0.0)
    stream.synchronize()

    b0, b1, busy_keep = _busy(gpu, stream, 20.0)
    dts = [np.float32((k + 1) * 200e-6) for k in range(n)]
    t0 = time.perf_counter()
    for k in range(n):
        st.stage_table(pinned[k + 1], pinned=True)
        st.tick_dt(float(dts[k]))
        gpu.memcpy_dtod(int(keep) + k * slab, buf, slab, stream)
    host_ms = (time.perf_counter() - t0) * 1e3
    stream.synchronize()
    queued_ms = b1.elapsed_ms_since(b0)
    assert queued_ms >= 20.0
    assert host_ms < 0.5 * queued_ms, (host_ms, queued_ms)
    for k in range(n):
        _check_slab(oracle, gpu, int(keep) + k * slab, oracle.generate_dt(op, tables[k + 1], [dts[k]]), 1, k)
    st.end()
    g.close()
    buf.free()
    keep.free()
    busy_keep[1].free()
    busy_keep[0].close()


def test_staged_host_ticks_at_the_cadence_slab(gpu, oracle):
    """64 ant x 1024 beams x 2560 channels (the 200 us cadence slab of BASELINE configs[4], 1.34 GB per tick), fp32:
    twelve staged host-table ticks back to back; rows 0, the middle and the last of every tick copied aside on the
    stream and compared with the oracle."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    bp = BeamformerParameters(NR_CHANNELS=2560, NR_STATIONS=64, NR_BEAMS=1024)
    op = oracle.params_from(bp)
    n = 12
    rows = (0, bp.NR_CHANNELS // 2, bp.NR_CHANNELS - 1)
    tables = [rand_table(bp.n_pairs, seed=1800 + k) for k in range(n + 1)]
    g = SteeringCoefficientGenerator(bp)
    stream = gpu.Stream()
    row = bp.n_pairs * 8
    slab = bp.NR_CHANNELS * row
    buf = gpu.mem_alloc(slab)
    keep = gpu.mem_alloc(row * len(rows) * n)
    g.upload_delays(tables[0], stream=stream)
    st = g.stream_begin(buf, slab, 0, bp.NR_CHANNELS, stream)
    st.stage_table(tables[1])
    dts = [np.float32((k + 1) * 200e-6) for k in range(n)]
    for k in range(n):
        st.tick_dt(float(dts[k]))
        for j, r in enumerate(rows):
            gpu.memcpy_dtod(int(keep) + (k * len(rows) + j) * row, int(buf) + r * row, row, stream)
        if k + 1 < n:
            st.stage_table(tables[k + 2])
    stream.synchronize()
    for k in range(n):
        for j, r in enumerate(rows):
            exp = oracle.generate_dt(op, tables[k + 1], [dts[k]], r, 1)
            _check_slab(oracle, gpu, int(keep) + (k * len(rows) + j) * row, exp, 1, (k, r))
    st.end()
    g.close()
    buf.free()
    keep.free()
