"""GPU parity of the per-sample fused kernel (dcs_bf_generate_and_beamform and _dt: coefficient generation and beamforming
in one launch) against the CPU oracle's restatement of the verifier (BeamformerCoefficientTest.cu:363-414).
The generator's own parity is tests/test_gpu_parity.py; the bound is helpers.parity_case.fused_bound.  Samples, table and
the guarded beams tensor are a helpers.bacc_case.Case, closed by the fixture."""
from functools import partial

import numpy as np
import pytest

from conftest import rand_table
from helpers import hip_graph
from helpers.bacc_case import Case
from helpers.device_buffers import closed_after
from helpers.parity_case import fused_bound

pytestmark = pytest.mark.gpu


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(Case, gpu, oracle))


@pytest.mark.parametrize("A,B,C,nt,seeded", [(64, 16, 64, 256, False), (64, 16, 64, 32, True), (8, 4, 5, 16, True),
                                             (37, 21, 9, 48, True), (130, 3, 4, 16, True), (4, 40, 7, 32, True),
                                             (9, 5, 3, 16, True), (129, 2, 2, 16, True), (258, 2, 5, 16, True),
                                             (1, 1, 1, 16, True), (3, 17, 2, 32, True)])
def test_fused_coefficient_generation_and_beamforming(case, oracle, A, B, C, nt, seeded):
    """beams = sum over antennas (in order) of the element-wise product of
    coefficient and int8 sample, against the verifier restatement
    (BeamformerCoefficientTest.cu:363-414), at fused_bound(A) and at the reference's 1e-1
    (runBeamformerTests.cpp:15).  Seeded: the Case's own table (seed A + B) and samples (seed A);
    otherwise the reference's ramps."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import simulate_input

    if seeded:
        c = case(A, B, C, nt)  # table indexed [b*A + a] by this kernel
    else:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        c = case(A, B, C, nt, table=simulate_input(bp), ant=oracle.simulate_antenna_data(oracle.params_from(bp), nt))
    exp = oracle.beamform(c.op, c.table, nt, c.ant)
    got = c.run("fused")
    diff = np.abs(got - exp)
    assert np.all(np.isfinite(got))
    assert diff.max() <= fused_bound(A), diff.max()
    assert oracle.compare(got, exp, 1e-1) == -1


def test_fused_seeded_fuzz(case, oracle):
    """40 seeded random cases of the per-sample fused kernel: antennas 1..300 (several 128-antenna LDS chunks), beams
    1..70 (partial 16-beam groups), channels (odd counts: the two-channels-per-pass loop's tail), 1..6 sample blocks,
    a time offset, times by index or by value -- each within fused_bound(A) of the verifier, nothing written outside
    the tensor."""
    rng = np.random.default_rng(20261006)
    for n in range(40):
        A = int(rng.choice([1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 300])) if n % 2 else int(rng.integers(1, 200))
        B = int(rng.integers(1, 71))
        C = int(rng.integers(1, 8))
        nblk = int(rng.integers(1, 7))
        while A * B * C * nblk * 16 > 400000 and nblk > 1:
            nblk -= 1
        while A * B * C * nblk * 16 > 400000 and C > 1:
            C -= 1
        nt = 16 * nblk
        table = rand_table(A * B, seed=5000 + n)
        ant = rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8)
        by_value = bool(rng.integers(0, 2))
        c = case(A, B, C, nt, table=table, ant=ant)
        if by_value:
            dts = rng.uniform(0.0, 0.3, size=nt).astype(np.float32)
            exp = oracle.beamform_dt(c.op, table, dts, ant)
            c.enqueue_fused(False, None, dts)
            got = c.read_beams()
        else:
            exp = oracle.beamform(c.op, table, nt, ant)
            got = c.run("fused")
        tag = (n, A, B, C, nt, by_value)
        assert np.all(np.isfinite(got)), tag
        assert np.abs(got - exp).max() <= fused_bound(A), (tag, float(np.abs(got - exp).max()))


def test_fused_more_steps_than_ride_in_the_kernel_arguments_and_under_capture(gpu, case, oracle):
    """The per-sample fused kernel with 288 > 256 time steps (their fDeltaTime table is staged through pinned memory, two
    terms launches) and, with 256, captured into a hipGraph after a first plain call and replayed on new samples."""
    A, B, C = 9, 20, 3
    rng = np.random.default_rng(11)
    for nt in (288, 256):
        table = rand_table(A * B, seed=62)
        ant = rng.integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
        c = case(A, B, C, nt, table=table, ant=ant)
        gpu.synchronize()
        s = gpu.Stream()
        c.enqueue_fused(False, s.handle)
        s.synchronize()
        assert np.abs(c.read_beams() - oracle.beamform(c.op, table, nt, ant)).max() <= fused_bound(A)
        if nt == 256:
            with hip_graph.capture(s) as graph:
                c.enqueue_fused(False, s.handle)
            try:
                for rep in range(2):
                    ant2 = rng.integers(-128, 128, size=ant.shape, dtype=np.int8)
                    gpu.memcpy_htod(c.d_ant, ant2, stream=s.handle)
                    c.refill(c.d_beams, stream=s.handle)
                    graph.launch(s)
                    s.synchronize()
                    assert np.abs(c.read_beams() - oracle.beamform(c.op, table, nt, ant2)).max() <= fused_bound(A)
            finally:
                s.synchronize()
                graph.close()


def test_fused_harness_and_slow_path(case, oracle):
    from dc_sand_amd.beamformer_coeff_test import BeamformerCoeffTest, SteeringCoefficientBitWidth as BW, SteeringCoefficientKernel as K

    def beam_verifier(bp, delays, nt, ant):
        return oracle.beamform(oracle.params_from(bp), np.asarray(delays), nt, ant)

    t = BeamformerCoeffTest(1e-1, K.COMBINED_COEFF_GEN_AND_BEAMFORMER_SINGLE_CHANNEL, BW.b32, beam_verifier=beam_verifier, verbose=False)
    t.run_test()
    assert t.get_result() == 1 and t.max_abs_diff < 2e-3
    assert t.get_time() > 0
    with pytest.raises(ValueError):
        BeamformerCoeffTest(1e-1, K.COMBINED_COEFF_GEN_AND_BEAMFORMER_SINGLE_CHANNEL, BW.b16)
    # a pair outside the fast path's range sends its 16-sample blocks down the slow branch
    table = rand_table(9 * 5, seed=77)
    table["fDelayRate_sps"][11] = 1e-2
    table["fDelayRate_sps"][12] = 1e-30
    ant = np.random.default_rng(3).integers(-128, 128, size=(6, 2, 9, 16, 2), dtype=np.int8)
    c = case(9, 5, 6, 32, table=table, ant=ant)
    assert np.abs(c.run("fused") - oracle.beamform(c.op, table, 32, ant)).max() <= 2e-4 * 9


@pytest.mark.parametrize("A,B,C", [(9, 16, 16384), (130, 16, 4096)])
def test_fused_slow_path_with_several_channels_per_pass(case, oracle, A, B, C):
    """The fused kernel's slow branch when a pass covers 4 channels (<= 64 antennas) or 2 (more: the
    antennas also cross the 128-antenna LDS chunk): enough channels that the launcher keeps 4 per
    workgroup, and slow-class pairs so that every 16-sample block takes the branch.  The samples are the Case's own
    (seed A)."""
    nt = 16
    table = rand_table(A * B, seed=A)
    table["fDelayRate_sps"][5] = 1e-2    # |fRotation| far beyond the fast path's range
    table["fDelayRate_sps"][A + 1] = 1e-30  # rate term outside the divide's proven range
    c = case(A, B, C, nt, table=table)
    got = c.run("fused")
    assert np.all(np.isfinite(got))
    assert np.abs(got - oracle.beamform(c.op, table, nt, c.ant)).max() <= 2e-4 * A


def test_fused_with_time_offset(case, oracle):
    """generate_and_beamform(t0 = 32, nt = 32) equals the last two 16-sample blocks of the
    verifier's 64-sample tensor (the time index is absolute)."""
    A, B, C = 12, 20, 6
    table = rand_table(A * B, seed=17)
    ant_full = np.random.default_rng(9).integers(-128, 128, size=(C, 4, A, 16, 2), dtype=np.int8)
    c = case(A, B, C, 32, table=table, ant=np.ascontiguousarray(ant_full[:, 2:4]), NR_SAMPLES_PER_CHANNEL=64)
    exp = oracle.beamform(c.op, table, 64, ant_full)[:, 2:4]
    c.g.generate_and_beamform(c.d_ant, c.ant.nbytes, c.d_beams, c.nbytes, t0=32, nt=32)
    assert np.abs(c.read_beams() - np.ascontiguousarray(exp)).max() <= fused_bound(A)


def test_fused_generate_and_beamform_dt(case, oracle):
    """dcs_bf_generate_and_beamform_dt: 32 samples 200 us apart."""
    A, B, C, nt = 12, 20, 6, 32
    table = rand_table(A * B, seed=74)
    ant = np.random.default_rng(10).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    dts = (np.arange(nt, dtype=np.float64) * 200e-6 + 0.25).astype(np.float32)
    c = case(A, B, C, nt, table=table, ant=ant)
    c.enqueue_fused(False, None, dts)
    assert np.abs(c.read_beams() - oracle.beamform_dt(c.op, table, dts, ant)).max() <= fused_bound(A)
