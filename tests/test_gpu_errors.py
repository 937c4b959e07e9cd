"""Error paths of the C-ABI on the GPU: a call that cannot be part of a stream capture says so
with a status BEFORE it enqueues anything -- the capture stays valid --, and a failure in the middle of a per-time-step
launch loop leaves the side streams joined and the caller's stream usable."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import rand_table
from helpers import hip_graph

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_non_capturable_calls_are_refused_up_front_and_the_capture_survives(gpu, oracle):
    """On a capturing stream: ``generate_dt`` of 300 time steps (their fDeltaTime values would be staged through pinned
    memory behind an event wait), the rows form with > 1 time step, a first-ever ``beamform_accumulated`` and
    ``generate_and_beamform`` (their terms table would be allocated), ``autotune`` and ``stream_begin`` all return
    DCS_ERR_UNSUPPORTED; capturable calls made in the SAME capture afterwards are recorded, the capture ends cleanly
    and its replay writes what the oracle says."""
    from dc_sand_amd import BeamformerParameters, _lib
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    bp = BeamformerParameters(NR_CHANNELS=24, NR_STATIONS=5, NR_BEAMS=13)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs, seed=31)
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(table)
    g_rows = SteeringCoefficientGenerator(bp)
    g_rows.set_tuning(form=2)
    g_rows.upload_delays(table)
    gpu.synchronize()
    nbytes = g.output_bytes(1, 300)
    buf = gpu.mem_alloc(nbytes)
    ant = gpu.mem_alloc(bp.NR_STATIONS * bp.NR_CHANNELS * 16 * 2)
    beams = gpu.mem_alloc(bp.NR_BEAMS * bp.NR_CHANNELS * 16 * 8)
    gpu.memset(ant, 1, ant.nbytes)
    s = gpu.Stream()
    dts = np.linspace(0.0, 0.3, 300).astype(np.float32)
    with hip_graph.capture(s) as graph:
        refused = [
            lambda: g.generate_dt(buf, nbytes, dts, stream=s),
            lambda: g.generate(buf, nbytes, t0=0, nt=300, stream=s),
            lambda: g_rows.generate(buf, nbytes, t0=0, nt=2, stream=s),
            lambda: g.beamform_accumulated(ant, ant.nbytes, beams, beams.nbytes, 16, t_coeff=1, stream=s),
            lambda: g.generate_and_beamform(ant, ant.nbytes, beams, beams.nbytes, 0, 16, stream=s),
            lambda: g.autotune(buf, nbytes, stream=s),
            lambda: g.stream_begin(buf, nbytes, 0, bp.NR_CHANNELS, s),
        ]
        for i, call in enumerate(refused):
            with pytest.raises(_lib.DcsError) as e:
                call()
            assert e.value.status == _lib.DCS_ERR_UNSUPPORTED, (i, e.value.status)
        # the capture is still alive: these ARE capturable (up to 256 time steps ride in the kernel arguments)
        g.generate(buf, nbytes, t0=7, nt=256, stream=s)
    gpu.memset(buf, 0xFF, nbytes, stream=s)
    graph.launch(s)
    s.synchronize()
    exp = oracle.generate(op, table, 7, 256)
    got = np.empty(exp.shape, dtype=np.float32)
    gpu.memcpy_dtoh(got, buf)
    assert oracle.max_ulp(got, exp, 1)[1] == 0
    graph.close()
    # outside a capture every one of the refused calls works (and the beamformers become capturable after their first call)
    g.generate_dt(buf, nbytes, dts, stream=s)
    s.synchronize()
    gpu.memcpy_dtoh(got, buf, nbytes=got.nbytes)
    assert oracle.max_ulp(got, oracle.generate_dt(op, table, dts[:256]), 1)[1] == 0
    g.beamform_accumulated(ant, ant.nbytes, beams, beams.nbytes, 16, t_coeff=1, stream=s)
    s.synchronize()
    hip_graph.begin(s)
    g.beamform_accumulated(ant, ant.nbytes, beams, beams.nbytes, 16, t_coeff=1, stream=s)
    hip_graph.destroy(hip_graph.end(s))
    g.close()
    g_rows.close()
    for b in (buf, ant, beams):
        b.free()


def _first_failing_time_index(bp):
    """The first time index whose nanosecond step (BCT.cu:299: t * 1e-7f * 1e9f * 8192 in fp32) no longer fits a long."""
    from dc_sand_amd import _lib
    from dc_sand_amd.generator import delta_times

    def valid(t):
        try:
            delta_times(bp, t, 1)
            return True
        except _lib.DcsError as e:
            assert e.status == _lib.DCS_ERR_OUT_OF_RANGE
            return False

    t_edge = int(9.2e18 / (1e-7 * 1e9 * 8192))
    while not valid(t_edge):
        t_edge -= 1 << 20
    lo, hi = t_edge, t_edge + (1 << 22)
    while valid(hi):
        hi += 1 << 22
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if valid(mid):
            lo = mid
        else:
            hi = mid
    assert valid(hi - 1) and not valid(hi)
    return hi


@pytest.mark.parametrize("kernel", [0, 1, 2, "slab", "fused", "fused_weighted"])
def test_time_index_out_of_range_mid_loop_launches_nothing(gpu, kernel):
    """A multi-launch call whose LATER time indices overflow the verifier's nanosecond step (BCT.cu:299: the fp32
    product no longer fits a long) returns DCS_ERR_OUT_OF_RANGE before the first launch (and before the fork of the
    per-time-step loops): the output buffer is untouched and the stream carries on.  Kernels 0 and 1 launch per time step
    (steps 0 .. 4 valid); kernel 2, generate_slab and the fused beamformer (weighted or not) launch per chunk of 4096 time
    steps at this shape: 4096 + 32 steps whose first chunk is valid and whose second is not."""
    from dc_sand_amd import BeamformerParameters, _lib
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    bp = BeamformerParameters(NR_CHANNELS=8, NR_STATIONS=2, NR_BEAMS=3)
    A, B, C = 2, 3, 8
    hi = _first_failing_time_index(bp)
    per_step = kernel in (0, 1)
    nt = 16 if per_step else 4096 + 32
    # per-step loops: steps 0..4 are valid, 5.. are not; chunked loops: t0 a multiple of 16 (the beamformers' rule), the first
    # invalid step among the 32 of the second chunk
    t0 = hi - 5 if per_step else (hi - 4097) // 16 * 16
    assert t0 < hi and (per_step or 4096 < hi - t0 < nt)
    g = SteeringCoefficientGenerator(bp)
    g.upload_delays(rand_table(bp.n_pairs))
    s = gpu.Stream()
    extra = []
    if kernel in ("fused", "fused_weighted"):
        d_ant = gpu.mem_alloc(C * nt * A * 2)
        gpu.memset(d_ant, 1, d_ant.nbytes)
        d_w = gpu.mem_alloc(B * A * 4)
        gpu.memcpy_htod(d_w, np.ones((B, A), np.float32))
        extra = [d_ant, d_w]
        nbytes = C * nt * B * 8
        if kernel == "fused":
            call = lambda buf, t: g.generate_and_beamform(d_ant, d_ant.nbytes, buf, nbytes, t0=t, nt=nt, stream=s)
        else:
            call = lambda buf, t: g.generate_and_beamform_weighted(d_ant, d_ant.nbytes, d_w, buf, nbytes, t0=t, nt=nt, stream=s)
    elif kernel == "slab":
        nbytes = nt * 3 * bp.n_pairs * 8
        call = lambda buf, t: g.generate_slab(buf, nbytes, 2, 3, t0=t, nt=nt, stream=s)
    else:
        nbytes = g.output_bytes(1, nt)
        call = lambda buf, t: g.generate(buf, nbytes, t0=t, nt=nt, kernel=kernel, stream=s)
    buf = gpu.mem_alloc(nbytes)
    gpu.memset(buf, 0xFF, nbytes, stream=s)
    with pytest.raises(_lib.DcsError) as e:
        call(buf, t0)
    assert e.value.status == _lib.DCS_ERR_OUT_OF_RANGE
    s.synchronize()
    host = np.empty(nbytes, dtype=np.uint8)
    gpu.memcpy_dtoh(host, buf)
    assert np.all(host == 0xFF), f"a launch was made before the range check: {int(np.count_nonzero(host != 0xFF))} of {nbytes} bytes written"
    call(buf, 0)  # the stream is fine
    s.synchronize()
    gpu.memcpy_dtoh(host, buf)
    assert not np.all(host == 0xFF)
    g.close()
    for b in [buf] + extra:
        b.free()


def test_launch_failure_in_the_fan_out_loop_joins_the_side_streams(gpu):
    """The injected-failure rehearsal (tests/helpers/fanout_failure.py) in a child process that loads the -DDCS_PROBES
    build of the SAME sources behind the ordinary wrappers: status returned, side streams joined, capture endable,
    stream usable afterwards."""
    from probes import build as pb

    env = dict(os.environ, DCS_LIB_PATH=str(pb.build()))
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "helpers" / "fanout_failure.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:] + res.stderr[-4000:]
