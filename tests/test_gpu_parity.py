"""GPU parity: the HIP path, called through the C-ABI, against the CPU oracle.  This file holds the coefficient generator
and, at its end, the beamformer with coefficient reuse on the matrix cores (dcs_bf_beamform_accumulated); the per-sample fused
kernel is held to the same oracle in tests/test_gpu_parity_fused.py, the streaming ticks in tests/test_gpu_streaming.py, the
examples and the C++ host in tests/test_gpu_examples.py.

Bar: every fp32 element within 1 ULP of the oracle (ordered-integer distance of
the bit patterns), and the reference's own rule |gpu - cpu| <= 1e-4
(runBeamformerTests.cpp:30,61).  The oracle's canonical reading of ``cos(float)`` is
double-then-round; configs 1-2 and the reference's default tensor are also held to
1 ULP of its float-libm reading (``check_float_reading``).  Time indices 5, 7, 9, 18 are those where the
reference's three dt derivations disagree.

Every context and every buffer comes from a fixture that closes it whatever the test's end; every output has a guard
behind it (helpers/parity_case.py, helpers/bacc_case.py).
"""
import time
from functools import partial

import numpy as np
import pytest

from conftest import rand_table
from helpers import hip_graph
from helpers import bacc_cases as bc
from helpers import launch_forms as lf
from helpers.bacc_case import T_COEFF, Case, plan_of
from helpers.device_buffers import DeviceBuffers, closed_after
from helpers.every_element import compare_every_element
from helpers.parity_case import (GeneratorCase, Tensor, accumulated_bound, check_1ulp, check_exact_sum, check_float_reading, fused_bound,
                                 ordered_distance)

pytestmark = pytest.mark.gpu

PARITY_T = [0, 1, 5, 7, 9, 18, 255]


@pytest.fixture
def generator(gpu):
    yield from closed_after(partial(GeneratorCase, gpu))


@pytest.fixture
def buffers(gpu):
    yield from closed_after(partial(DeviceBuffers, gpu))


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(Case, gpu, oracle))


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_config1_4ant_2beam_1024chan(generator, oracle, kernel):
    """BASELINE configs[0]: 4 ant x 2 beam x 1024 chan, reference ramp input."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import simulate_input

    bp = BeamformerParameters(NR_CHANNELS=1024, NR_STATIONS=4, NR_BEAMS=2)
    table = simulate_input(bp)
    op = oracle.params_from(bp)
    assert np.array_equal(table.view(np.uint32), oracle.simulate_input(op).view(np.uint32))
    c = generator(bp, table)
    for t in PARITY_T:
        got = c.generate(t, 1, kernel=kernel)
        check_1ulp(oracle, got, oracle.generate(op, table, t, 1))
        check_float_reading(oracle, got, op, table, t, 1)


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_reference_default_shape_all_256_time_steps(generator, oracle, kernel):
    """BeamformerParameters.h defaults (64 chan, 64 ant, 16 beams, 256 samples):
    the tensor runBeamformerTests verifies, every element."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import simulate_input

    bp = BeamformerParameters()
    table = simulate_input(bp)
    op = oracle.params_from(bp)
    got = generator(bp, table).generate(0, 256, kernel=kernel)
    check_1ulp(oracle, got, oracle.generate(op, table, 0, 256))
    check_float_reading(oracle, got, op, table, 0, 256)


@pytest.mark.parametrize("seeded", [False, True])
def test_config2_64ant_64beam_4096chan(generator, oracle, seeded):
    """BASELINE configs[1]: single launch, every element compared."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import simulate_input

    bp = BeamformerParameters(NR_CHANNELS=4096, NR_STATIONS=64, NR_BEAMS=64)
    table = rand_table(bp.n_pairs) if seeded else simulate_input(bp)
    op = oracle.params_from(bp)
    c = generator(bp, table)
    for t in (1, 9):
        got = c.generate(t, 1)
        check_1ulp(oracle, got, oracle.generate(op, table, t, 1))
        check_float_reading(oracle, got, op, table, t, 1)


TUNINGS = [
    dict(form=1, tiles_per_block=1, nontemporal=1),
    dict(form=1, tiles_per_block=2, nontemporal=0),
    dict(form=1, tiles_per_block=4, chan_per_block=8, nontemporal=1),
    dict(form=1, tiles_per_block=1, chan_per_block=3),
    dict(form=1, tiles_per_block=4, chan_per_block=1000),
    dict(form=1, tiles_per_block=1, chan_per_block=13, xcd_remap=1),
    dict(form=1, tiles_per_block=1, chan_per_block=12, wg_per_cu=-1),
    dict(form=1, tiles_per_block=2, chan_per_block=5, wg_per_cu=2),
    dict(form=1, tiles_per_block=4, chan_per_block=9, wg_per_cu=7),
    dict(form=3),
    dict(form=3, tiles_per_block=2, chan_per_block=5, wg_per_cu=-1),
    dict(form=3, tiles_per_block=4, chan_per_block=3, wg_per_cu=7),
    dict(form=3, tiles_per_block=1, chan_per_block=16, nontemporal=0),
    dict(form=2),
    dict(form=2, waves_per_block=4, rows_per_wave=1, rows_same_tile=0),
    dict(form=2, waves_per_block=4, rows_per_wave=2, nontemporal=1, rows_same_tile=0),
    dict(form=2, waves_per_block=8, rows_per_wave=4, xcd_remap=1, rows_same_tile=0),
    dict(form=2, waves_per_block=16, rows_per_wave=1, xcd_remap=1, nontemporal=1, rows_same_tile=0),
    dict(form=2, waves_per_block=16, rows_per_wave=4, rows_same_tile=0),
    dict(form=2, waves_per_block=4, rows_per_wave=3, rows_same_tile=1),
    dict(form=2, waves_per_block=4, rows_per_wave=3, rows_same_tile=1, wg_per_cu=4),
    dict(form=2, waves_per_block=8, rows_per_wave=1, rows_same_tile=1, xcd_remap=0),
]


@pytest.mark.parametrize("tuning", TUNINGS, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
@pytest.mark.parametrize("bitwidth", [1, 0])
def test_tunings_agree(generator, oracle, tuning, bitwidth):
    """Every form and launch geometry gives the same bits (ragged channel
    blocks, partial tiles and odd row groups included)."""
    from dc_sand_amd import BeamformerParameters

    for (A, B, C) in ((7, 38, 301), (3, 5, 17), (64, 16, 64)):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        table = rand_table(bp.n_pairs, seed=7)
        got = generator(bp, table, tuning).generate(3, 3, bitwidth=bitwidth)
        if bitwidth == 1:
            check_1ulp(oracle, got, oracle.generate(oracle.params_from(bp), table, 3, 3))
        else:
            base = generator(bp, table).generate(3, 3, bitwidth=0)
            assert np.array_equal(got.view(np.uint16), base.view(np.uint16))


@pytest.mark.parametrize("A,B,C", [(1, 1, 1), (3, 5, 17), (5, 3, 64), (1, 129, 33), (64, 1, 5), (2, 257, 9)])
@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_ragged_and_odd_shapes(generator, oracle, A, B, C, kernel):
    """Odd pair counts (8-byte stores), partial tiles, single elements; the
    three kernel options cover the naive, tiled and rows forms."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
    table = rand_table(bp.n_pairs, seed=A * 1000 + B)
    got = generator(bp, table).generate(7, 3, kernel=kernel)
    check_1ulp(oracle, got, oracle.generate(oracle.params_from(bp), table, 7, 3))


def test_channel_slab(generator, oracle):
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=4, NR_BEAMS=32)
    table = rand_table(bp.n_pairs, seed=11)
    op = oracle.params_from(bp)
    c = generator(bp, table)
    for c0, nc in ((0, 5), (32000, 768), (16383, 2)):
        check_1ulp(oracle, c.generate_slab(c0, nc, 18, 2), oracle.generate(op, table, 18, 2, c0, nc))


def test_slow_path_large_rotation_and_extreme_rates(generator, oracle):
    """Pairs outside the fast path's proven range (|rotation| >= 32000, tiny or
    huge rate terms, zero rate) take the IEEE-divide + fp64-sincos branch."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=512, NR_STATIONS=2, NR_BEAMS=128)
    table = rand_table(bp.n_pairs, seed=3)
    table["fDelayRate_sps"][5] = 1e-2      # rotation up to ~3e5 rad
    table["fDelayRate_sps"][6] = 1e-30     # below dcs_div_const's range
    table["fDelayRate_sps"][7] = 0.0
    table["fPhase_rad"][130] = 5e4
    table["fDelayRate_sps"][200] = -3.0    # huge
    table["fDelay_s"][201] = 1.0
    op = oracle.params_from(bp)
    forms = {form: generator(bp, table, dict(form=form)) for form in (1, 2, 3)}
    for t in (0, 9):
        for form in (1, 2, 3):
            check_1ulp(oracle, forms[form].generate(t, 1), oracle.generate(op, table, t, 1), tol=1e-4)


def test_fp16_output(generator, oracle):
    """b16: packed half2, RN-even of the fp32 coefficient.  The reference never
    verifies this mode (BeamformerCoefficientTest.cu:282-287): parity unpinned;
    the expectation is RN-even(oracle fp32), tolerance 1 half-ULP."""
    from dc_sand_amd import BeamformerParameters

    for (A, B, C) in ((64, 16, 64), (3, 5, 17), (2, 130, 9)):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        table = rand_table(bp.n_pairs, seed=5)
        c = generator(bp, table)
        got = c.generate(5, 2, kernel=2, bitwidth=0)
        exp = oracle.generate(oracle.params_from(bp), table, 5, 2).astype(np.float16)
        assert ordered_distance(got, exp) <= 1
        # MULTIPLE_CHANNELS supports b16 as well (reference kernel a2)
        got2 = c.generate(5, 2, kernel=1, bitwidth=0)
        assert np.array_equal(got.view(np.uint16), got2.view(np.uint16))


def test_error_behaviour(generator):
    """NAIVE + b16 and COMBINED are refused like the reference's ctor throws
    (BeamformerCoefficientTest.cu:40-50); generate before upload is NOT_READY."""
    from dc_sand_amd import BeamformerParameters, _lib

    c = generator(BeamformerParameters(NR_CHANNELS=8, NR_STATIONS=2, NR_BEAMS=2))
    g, buf = c.g, c.tensor(1)
    assert buf.nbytes == g.output_bytes(1, 1)
    with pytest.raises(_lib.DcsError) as e:
        g.generate(buf.ptr, buf.nbytes)
    assert e.value.status == _lib.DCS_ERR_NOT_READY
    g.upload_delays(rand_table(4))
    with pytest.raises(_lib.DcsError) as e:
        g.generate(buf.ptr, buf.nbytes, kernel=0, bitwidth=0)
    assert e.value.status == _lib.DCS_ERR_UNSUPPORTED
    with pytest.raises(_lib.DcsError) as e:
        g.generate(buf.ptr, buf.nbytes, kernel=3)  # the fused kernel has its own entry point
    assert e.value.status == _lib.DCS_ERR_UNSUPPORTED
    with pytest.raises(_lib.DcsError) as e:
        g.generate_and_beamform(buf.ptr, 8, buf.ptr, 8, t0=0, nt=8)  # not a multiple of 16
    assert e.value.status == _lib.DCS_ERR_INVALID_ARGUMENT
    with pytest.raises(_lib.DcsError) as e:
        g.generate(buf.ptr, buf.nbytes - 1)
    assert e.value.status == _lib.DCS_ERR_INVALID_ARGUMENT
    for bad in (dict(wg_per_cu=1), dict(wg_per_cu=8), dict(wg_per_cu=-2), dict(tiles_per_block=3), dict(form=4), dict(math_mode=-1)):
        with pytest.raises(_lib.DcsError) as e:
            g.set_tuning(**bad)
        assert e.value.status == _lib.DCS_ERR_INVALID_ARGUMENT, bad
    for probe_only in (dict(probe_pace=3), dict(probe_nomath=True)):  # ABI 2's measurement fields are gone from the struct (ABI 3)
        with pytest.raises(TypeError):
            g.set_tuning(**probe_only)
    assert np.all(buf.read().view(np.uint32) == 0xFFFFFFFF)  # no refused call wrote anything


def test_beam_shard_gather(generator, buffers, oracle):
    """set_delays_from_global: a context holding beams [off, off+B_loc) of a
    global [A][B_total] device table produces that column slab of the global
    tensor."""
    from dc_sand_amd import BeamformerParameters

    A, B_total, C = 6, 40, 33
    glob = rand_table(A * B_total, seed=9)
    opg = oracle.params(C, A, B_total)
    full = oracle.generate(opg, glob, 2, 2)
    d_glob = buffers().upload(glob)
    for off, bl in ((0, 10), (10, 10), (30, 10), (7, 33)):
        c = generator(BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=bl))
        c.g.set_delays_from_global(d_glob, B_total, off)
        check_1ulp(oracle, c.generate(2, 2), np.ascontiguousarray(full[:, :, :, off:off + bl, :]))


def test_unit_test_harness_five_phases(gpu, oracle, capsys):
    """The BeamformerCoeffTest mirror: run_test() -> result 1, three timed
    phases, utilisation model; get_result() before run_test() is 0."""
    from dc_sand_amd.beamformer_coeff_test import BeamformerCoeffTest, SteeringCoefficientBitWidth as BW, SteeringCoefficientKernel as K

    def verifier(bp, delays, nt):
        return oracle.generate(oracle.params_from(bp), np.asarray(delays), 0, nt)

    for kern in (K.MULTIPLE_CHANNELS_AND_TIMESTAMPS, K.NAIVE):
        t = BeamformerCoeffTest(1e-4, kern, BW.b32, verifier=verifier, verbose=False)
        assert t.get_result() == 0
        t.run_test()
        assert t.get_result() == 1
        assert t.max_ulp is not None and t.max_ulp <= 1
        total = t.get_time()
        assert total > 0 and t.m_fKernelElapsedTime_ms > 0
        assert t.get_gpu_utilisation_per_single_time_unit() > 0
    with pytest.raises(ValueError):
        BeamformerCoeffTest(1e-4, K.NAIVE, BW.b16)


def test_sincos_probe_fast_path_matches_host_sweep(gpu, buffers, oracle, probes):
    """The device evaluates dcs_sincos_fast to the same bits as the host build
    swept exhaustively in test_numerics.py (sampled: 4M arguments)."""
    rng = np.random.default_rng(1)
    x = np.concatenate([
        rng.uniform(-100, 100, 1 << 21).astype(np.float32),
        rng.uniform(-32000, 32000, 1 << 20).astype(np.float32),
        (np.arange(1, 1 << 20, dtype=np.float32) * np.float32(np.pi / 2)),  # near multiples of pi/2
    ])
    n = x.size
    b = buffers()
    dx, ds, dc = b.upload(x), b.out(4 * n, 0xFF, 0xFF), b.out(4 * n, 0xFF, 0xFF)  # unwritten: NaN
    es = np.sin(x.astype(np.float64)).astype(np.float32)
    ec = np.cos(x.astype(np.float64)).astype(np.float32)
    for which, limit in ((0, 1), (2, 1), (3, 1)):
        b.refill(ds)
        b.refill(dc)
        probes.sincos(which, dx, n, ds, dc)
        gpu.synchronize()
        s = b.read(ds, dtype=np.float32)
        c = b.read(dc, dtype=np.float32)
        # the fast path is only used (and only proven) below DCS_SINCOS_FAST_LIMIT
        sel = np.abs(x) < 32768.0 if which == 0 else (np.abs(x) < 512.0 if which == 3 else np.ones(n, dtype=bool))
        assert oracle.max_ulp(s[sel], es[sel], limit)[1] == 0
        assert oracle.max_ulp(c[sel], ec[sel], limit)[1] == 0


def test_against_committed_golden_fixtures(generator):
    """HIP path vs tests/golden/*.npz (written by tests/golden/make_golden.py):
    inputs and expected outputs come from the files alone."""
    import json
    from pathlib import Path

    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.parameters import delay_vals_dtype

    gold = Path(__file__).resolve().parent / "golden"
    man = json.loads((gold / "manifest.json").read_text())
    for entry in man["cases"]:
        z = np.load(gold / entry["file"], allow_pickle=False)
        bp = BeamformerParameters(NR_CHANNELS=entry["C"], NR_STATIONS=entry["A"], NR_BEAMS=entry["B"])
        c = generator(bp, np.ascontiguousarray(z["delays"]).view(delay_vals_dtype).ravel())
        for t, c0, nc, key in entry["slabs"]:
            assert ordered_distance(c.generate_slab(c0, nc, t, 1), z[key]) <= 1, (entry["file"], key)


def test_config3_full_size_every_element(gpu, generator, oracle, probes, record_property):
    """BASELINE configs[2] at FULL size (64 x 1024 x 32768, 16 GiB on the GPU): EVERY one of the 2^32 floats is
    compared with the verifier, as the reference's verify_output does (BeamformerCoefficientTest.cu:348-357) --
    <= 1 ULP under the canonical reading of cos(float), and <= 1 ULP under the float-libm reading too
    (|fRotation| < 100 here, inside the range proven in tests/test_numerics.py), whose count of 1-ULP elements is
    reported.  Then the size-independent properties on the device copy: unit modulus everywhere and the two
    independent forms (tiled / rows) writing bit-identical tensors."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times

    bp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=64, NR_BEAMS=1024)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs)
    c = generator(bp, table)
    out = c.tensor(1)
    nbytes = out.nbytes
    assert nbytes == c.g.output_bytes(1, 1) == 16 * 2 ** 30
    t = 9
    c.g.generate(out.ptr, nbytes, t0=t, nt=1)
    gpu.synchronize()
    out.guard_untouched()
    t0 = time.perf_counter()
    res = compare_every_element(gpu, oracle, out.ptr, op, table, delta_times(bp, t, 1)[0], bp.NR_CHANNELS, bp.n_pairs)
    wall = time.perf_counter() - t0
    n = bp.NR_CHANNELS * bp.n_pairs * 2
    for r in (0, 1):
        h = res[r]["hist"]
        assert sum(h) == n == 2 ** 32, "sampled fraction must be 1.0"
        assert h[2] == 0 and h[3] == 0 and res[r]["max_ulp"] <= 1, (r, res[r])
    summary = (f"config 3, all {n} floats: reading 0 (double-then-round) {res[0]['hist'][1]} at 1 ULP, 0 beyond; reading 1 (float libm) "
               f"{res[1]['hist'][1]} at 1 ULP, 0 beyond; {wall:.1f} s wall on {res['threads']} threads (D2H {res['copy_seconds']:.1f} s)")
    print(summary)
    record_property("config3_full_compare", summary)
    # whole-tensor properties on the device: unit modulus everywhere, and the two
    # independent forms (tiled / rows: different grids and index arithmetic, both
    # 64-bit) write bit-identical 16 GiB tensors
    ck1, dev1 = probes.tensor_properties(out.ptr, nbytes)
    assert dev1 < 4e-7
    c.g.set_tuning(form=2)
    out.refill()
    c.g.generate(out.ptr, nbytes, t0=t, nt=1)
    ck2, dev2 = probes.tensor_properties(out.ptr, nbytes)
    assert ck2 == ck1 and dev2 == dev1
    out.guard_untouched()
    # small-case anchor of the checksum itself
    small = np.empty((4, bp.NR_STATIONS, bp.NR_BEAMS, 2), dtype=np.float32)
    gpu.memcpy_dtoh(small, out.ptr)
    cks, _ = probes.tensor_properties(out.ptr, small.nbytes)
    assert cks == oracle.checksum_of(small)


@pytest.mark.parametrize("math_mode", [0, 4])
def test_config3_full_size_fp16_every_element(gpu, generator, oracle, record_property, math_mode):
    """The packed binary16 output of config 3 at FULL size (2^32 halves, 8 GiB), EVERY element against
    RN-even(verifier's fp32) -- the check the reference never makes (BeamformerCoefficientTest.cu:282-287 skip the b16
    case).  Default arithmetic (the <= 1 ULP fp32 pair rounded once): a half differs from the expectation only where the
    fp32 value sits within its own last place of a binary16 rounding boundary -- at most 1 binary16 ulp, and rarely.  The
    opt-in b16 arithmetic form (math_mode 4): within 1 binary16 ulp everywhere (tests/test_numerics.py proves that per
    argument; this is the whole tensor)."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd._lib import B16
    from dc_sand_amd.generator import delta_times

    bp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=64, NR_BEAMS=1024)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs)
    c = generator(bp, table, dict(math_mode=math_mode) if math_mode else None)
    out = c.tensor(1, bitwidth=B16)
    assert out.nbytes == c.g.output_bytes(B16, 1) == 8 * 2 ** 30
    t = 9
    c.g.generate(out.ptr, out.nbytes, t0=t, nt=1, bitwidth=B16)
    gpu.synchronize()
    out.guard_untouched()
    t0 = time.perf_counter()
    res = compare_every_element(gpu, oracle, out.ptr, op, table, delta_times(bp, t, 1)[0], bp.NR_CHANNELS, bp.n_pairs, readings=(0,), half=True)
    wall = time.perf_counter() - t0
    n = bp.NR_CHANNELS * bp.n_pairs * 2
    h = res[0]["hist"]
    assert sum(h) == n == 2 ** 32, "sampled fraction must be 1.0"
    assert h[2] == 0 and h[3] == 0 and res[0]["max_ulp"] <= 1, res[0]
    if math_mode == 0:
        assert h[1] < n // 1000  # double rounding only: a few in 10^4
    summary = (f"config 3 fp16 (math_mode {math_mode}), all {n} halves: {h[1]} at 1 binary16 ulp of RN16(verifier), 0 beyond; "
               f"{wall:.1f} s wall on {res['threads']} threads (D2H {res['copy_seconds']:.1f} s)")
    print(summary)
    record_property("config3_fp16_full_compare", summary)


def test_config4_one_rank_shard_at_full_size_every_element(gpu, generator, buffers, oracle, probes, record_property):
    """BASELINE configs[3]: 256 ant x 4096 beam x 32768 chan beam-sharded over 8 GPUs.  One rank's share at FULL size
    on this GPU (rank 3: beams [1536, 2048), 2^32 coefficients, 32 GiB): the slice is gathered on the device from the
    16 MiB global table, and EVERY one of its 2^33 floats is compared with the verifier's column slab (canonical
    reading; byte offsets beyond 2^32); the tiled and rows forms must agree on the whole tensor."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times
    from dc_sand_amd.sharding import beam_range, local_parameters, slice_table

    gp = BeamformerParameters(NR_CHANNELS=32768, NR_STATIONS=256, NR_BEAMS=4096)
    sh = beam_range(gp.NR_BEAMS, 8, 3)
    assert (sh.beam_lo, sh.beam_hi) == (1536, 2048)
    lp = local_parameters(gp, sh)
    glob = rand_table(gp.n_pairs, seed=44)
    assert glob.nbytes == 16 * 2 ** 20
    c = generator(lp)
    c.g.set_delays_from_global(buffers().upload(glob), gp.NR_BEAMS, sh.beam_lo)
    out = c.tensor(1)
    nbytes = out.nbytes
    assert nbytes == c.g.output_bytes(1, 1) == 32 * 2 ** 30
    t = 18
    c.g.generate(out.ptr, nbytes, t0=t, nt=1)
    gpu.synchronize()
    out.guard_untouched()
    local = slice_table(glob, gp, sh)
    op = oracle.params_from(lp)
    t0 = time.perf_counter()
    res = compare_every_element(gpu, oracle, out.ptr, op, local, delta_times(lp, t, 1)[0], lp.NR_CHANNELS, lp.n_pairs, readings=(0,))
    wall = time.perf_counter() - t0
    h = res[0]["hist"]
    assert sum(h) == 2 ** 33 and h[2] == 0 and h[3] == 0 and res[0]["max_ulp"] <= 1, res[0]
    summary = f"config 4 rank-3 shard, all {sum(h)} floats: {h[1]} at 1 ULP, 0 beyond; {wall:.1f} s wall on {res['threads']} threads"
    print(summary)
    record_property("config4_shard_full_compare", summary)
    ck, dev = probes.tensor_properties(out.ptr, nbytes)
    assert dev < 4e-7
    c.g.set_tuning(form=2)
    out.refill()
    c.g.generate(out.ptr, nbytes, t0=t, nt=1)
    ck2, dev2 = probes.tensor_properties(out.ptr, nbytes)
    assert (ck2, dev2) == (ck, dev)
    out.guard_untouched()


@pytest.mark.parametrize("form", [1, 2, 3])
def test_arithmetic_forms_agree_and_class_boundaries(generator, oracle, form):
    """The fast path has four arithmetic forms (3-op / 5-op divide x low- / full-degree
    polynomials), chosen per wave from a bound on |fRotation|; all must give the
    oracle's bits (<= 1 ULP) and each other's bits.  The table mixes pairs below 500 rad,
    between 500 and 32000 rad and beyond (slow path), so every class occurs, also
    inside one wave."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=200, NR_STATIONS=3, NR_BEAMS=200)
    table = rand_table(bp.n_pairs, seed=13)
    table["fDelayRate_sps"][100:140] = 2.0e-5    # ~630 rad at the top channel: full-degree class
    table["fDelayRate_sps"][300:310] = -4.0e-4   # ~12600 rad
    table["fDelayRate_sps"][470] = 1.5e-3        # > 32000 rad: slow path
    table["fPhase_rad"][520:530] = 499.0         # just below / above the class boundary
    table["fPhase_rad"][530:540] = 501.0
    exp = oracle.generate(oracle.params_from(bp), table, 9, 2)
    outs = []
    for mode in (0, 1, 2, 3):
        outs.append(generator(bp, table, dict(form=form, math_mode=mode)).generate(9, 2))
        check_1ulp(oracle, outs[-1], exp)
    for o in outs[1:]:
        # the forms are all within 1 ULP of the oracle; between each other they may
        # differ by the same 1 ULP only where the polynomial degree differs
        assert oracle.max_ulp(o, outs[0], 2)[1] == 0
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))  # divide form never changes a bit
    assert np.array_equal(outs[2].view(np.uint32), outs[3].view(np.uint32))


def test_autotune_keeps_results(generator, oracle):
    """dcs_bf_autotune picks a launch geometry by measurement; whatever it picks, the
    bits are the oracle's."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=300, NR_STATIONS=16, NR_BEAMS=40)
    table = rand_table(bp.n_pairs, seed=55)
    exp = oracle.generate(oracle.params_from(bp), table, 5, 2)
    for bw in (1, 0):
        c = generator(bp, table)
        out = c.tensor(2, bitwidth=bw)
        assert out.nbytes == c.g.output_bytes(bw, 2)
        t0 = time.perf_counter()
        chosen = c.g.autotune(out.ptr, out.nbytes, bitwidth=bw)
        t_first = time.perf_counter() - t0
        assert chosen["form"] == 0 and chosen["tiles_per_block"] in (1, 2, 4) and chosen["chan_per_block"] >= 1
        t0 = time.perf_counter()
        again = c.g.autotune(out.ptr, out.nbytes, bitwidth=bw)  # cached in the context per output width
        assert again == chosen and time.perf_counter() - t0 < max(0.05, 0.25 * t_first)
        out.read()  # the measuring launches stayed inside the tensor
        got = c.generate(5, 2, bitwidth=bw)
        if bw == 1:
            check_1ulp(oracle, got, exp)
        else:
            assert np.max(np.abs(got.astype(np.float32) - exp)) < 1e-3


def test_fp16_is_exactly_rne_of_the_fp32_output(generator):
    """b16 output == RN-even(b32 output), bit for bit (the reference's
    __floats2half2_rn of the same fp32 value, BeamformerKernels.cu:113,182): the fp16
    mode adds one correctly rounded conversion and nothing else."""
    from dc_sand_amd import BeamformerParameters

    for (A, B, C) in ((64, 16, 64), (5, 7, 33), (2, 300, 40)):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        c = generator(bp, rand_table(bp.n_pairs, seed=C))
        f32 = c.generate(9, 3, bitwidth=1)
        f16 = c.generate(9, 3, bitwidth=0)
        assert np.array_equal(f16.view(np.uint16), f32.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("form", [1, 2])
def test_many_time_steps_cross_the_internal_chunking(generator, oracle, form):
    """nt = 5000 > the 4096 fDeltaTime values staged per launch: the call is split into
    several launches internally; every time step must still be the oracle's."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=3, NR_BEAMS=6)
    table = rand_table(bp.n_pairs, seed=99)
    got = generator(bp, table, dict(form=form)).generate(250, 5000)
    check_1ulp(oracle, got, oracle.generate(oracle.params_from(bp), table, 250, 5000))


@pytest.mark.parametrize("form", [1, 2, 3])
@pytest.mark.parametrize("bitwidth", [1, 0])
def test_output_pointer_not_16_byte_aligned(generator, oracle, form, bitwidth):
    """An output tensor that starts 8 (fp32) or 4 (fp16) bytes off a 16-byte boundary
    takes the per-pair store path; the bytes before and after it stay untouched."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=19, NR_STATIONS=4, NR_BEAMS=34)
    table = rand_table(bp.n_pairs, seed=5)
    got = generator(bp, table, dict(form=form)).generate(3, 2, bitwidth=bitwidth, offset=8 if bitwidth == 1 else 4)
    exp = oracle.generate(oracle.params_from(bp), table, 3, 2)
    if bitwidth == 1:
        check_1ulp(oracle, got, exp)
    else:
        assert np.max(np.abs(got.astype(np.float32) - exp)) < 1e-3


def test_seeded_fuzz_of_shapes_slabs_time_ranges_and_geometries(generator, oracle):
    """80 seeded random cases: shape (ragged tiles, odd pair counts), channel slab, time range (1..300 time
    steps: both sides of the 256 that travel in the kernel arguments), kernel selection, output width,
    launch geometry of either form (incl. wg_per_cu) and an output pointer 0 / 8 / 16 bytes off alignment --
    every fp32 case within 1 ULP of the oracle, every fp16 case the RN-even image of the fp32 run,
    canaries before and after the tensor intact."""
    from dc_sand_amd import BeamformerParameters

    rng = np.random.default_rng(20261004)
    for n in range(80):
        A, B = int(rng.integers(1, 9)), int(rng.integers(1, 70))
        C = int(rng.integers(1, 80))
        nt = int(rng.choice([1, 2, 3, 17, 255, 256, 257, 300])) if n % 4 == 0 else int(rng.integers(1, 6))
        if nt > 16:
            A, B, C = min(A, 3), min(B, 9), min(C, 7)  # keep the oracle's work small
        t0 = int(rng.integers(0, 1000))
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        table = rand_table(bp.n_pairs, seed=1000 + n)
        bitwidth = int(rng.integers(0, 2))
        form = int(rng.integers(1, 4))
        if form != 2:
            tuning = dict(form=form if n % 3 else 0, tiles_per_block=int(rng.choice([1, 2, 4])), chan_per_block=int(rng.integers(1, 40)),
                          nontemporal=int(rng.integers(0, 2)), wg_per_cu=int(rng.choice([-1, 0, 2, 5, 6, 7])))
        else:
            tuning = dict(form=2, waves_per_block=int(rng.choice([4, 8, 16])), rows_per_wave=int(rng.integers(1, 5)),
                          rows_same_tile=int(rng.integers(0, 2)), wg_per_cu=int(rng.choice([0, 3, 6])))
        use_slab = bool(rng.integers(0, 2))
        c0 = int(rng.integers(0, C)) if use_slab else 0
        nc = int(rng.integers(1, C - c0 + 1)) if use_slab else C
        kernel = 2 if (use_slab or form == 2) else int(rng.choice([1, 2]))  # (MULTIPLE_CHANNELS: the tiled form, one launch per time step)
        off = int(rng.choice([0, 8 if bitwidth == 1 else 4, 16]))
        tag = f"case {n}: {A}x{B}x{C} nt={nt} t0={t0} slab=({c0},{nc}) kernel={kernel} b{bitwidth} off={off} {tuning}"
        c = generator(bp, table, tuning)
        if use_slab:
            got = c.generate_slab(c0, nc, t0, nt, bitwidth=bitwidth, offset=off)
        else:
            got = c.generate(t0, nt, kernel=kernel, bitwidth=bitwidth, offset=off)
        if bitwidth == 1:
            check_1ulp(oracle, got, oracle.generate(oracle.params_from(bp), table, t0, nt, c0, nc), tol=None, tag=tag)
        else:
            c.g.set_tuning()
            f32 = c.generate_slab(c0, nc, t0, nt) if use_slab else c.generate(t0, nt, kernel=2)
            assert np.array_equal(got.view(np.uint16), oracle.f32_to_f16_bits(f32)), tag


@pytest.mark.parametrize("nt,kernel", [(1, 2), (256, 2), (16, 1), (3, 1), (16, 0)])
def test_generate_under_stream_capture(gpu, generator, oracle, nt, kernel):
    """include/dcs_beamformer.h: "all device work is enqueued on the caller's stream so the calls can be
    captured in a hipGraph".  dcs_bf_generate under a stream capture (helpers/hip_graph.py; up to 256 time steps:
    their fDeltaTime values are kernel arguments; longer launches stage a table through pinned memory and
    are not capturable), instantiated and replayed twice: the replays write what a direct launch writes."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=24, NR_STATIONS=5, NR_BEAMS=13)
    table = rand_table(bp.n_pairs, seed=31)
    c = generator(bp, table)
    out = c.tensor(nt)
    assert out.nbytes == c.g.output_bytes(1, nt)
    gpu.synchronize()
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:  # hipStreamCaptureModeGlobal
        c.g.generate(out.ptr, out.nbytes, t0=7, nt=nt, stream=s.handle, kernel=kernel)  # (kernel 1 from 8 time steps on: a fork and a join over side streams)
    try:
        exp = oracle.generate(oracle.params_from(bp), table, 7, nt)
        for _ in range(2):
            out.refill(stream=s.handle)  # nothing was generated yet by the capture itself
            graph.launch(s)
            s.synchronize()
            check_1ulp(oracle, out.read(), exp)
    finally:
        s.synchronize()
        graph.close()


# ---- arbitrary-time entry points (the reference kernels take struct timespec sCurrentTime, sRefTime:
# ---- BeamformerKernels.cuh:38-42, 81-86; the verifier's fDeltaTime is ts_diff, BeamformerCoefficientTest.cu:12-18, :320)
OFF_GRID_DT = [0.0, 200e-6, 400e-6, 1e-3 + 3e-7, 0.123456, 1.5, -2e-4, 86400.0]  # not multiples of 819.2 us; before the reference; a day


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_generate_dt_off_grid_times(generator, oracle, kernel):
    """dcs_bf_generate_dt: fDeltaTime by value, every launch shape, against the verifier at the same fDeltaTime."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=24, NR_STATIONS=5, NR_BEAMS=13)
    table = rand_table(bp.n_pairs, seed=71)
    c = generator(bp, table)
    dts = np.array(OFF_GRID_DT, dtype=np.float32)
    got = c.generate_dt(dts, kernel=kernel)
    exp = oracle.generate_dt(oracle.params_from(bp), table, dts)
    check_1ulp(oracle, got, exp)
    assert not np.array_equal(got[1], got[2])
    if kernel != 0:  # b16 (NAIVE has no b16: BeamformerCoefficientTest.cu:40-44)
        h16 = c.generate_dt(dts, kernel=kernel, bitwidth=0)
        assert np.array_equal(h16.view(np.uint16), got.astype(np.float16).view(np.uint16))
    # a channel slab through dcs_bf_generate_slab_dt
    c0, nc = 7, 9
    gs = c.generate_slab_dt(c0, nc, dts)
    check_1ulp(oracle, gs, np.ascontiguousarray(exp[:, c0:c0 + nc]))  # (NAIVE picks its polynomial degree per pair, the tiled form per wave: not bit-equal)


@pytest.mark.parametrize("form", [1, 2])
def test_generate_dt_more_steps_than_ride_in_the_kernel_arguments(generator, oracle, form):
    """300 > 256 time steps 200 us apart (the staged fDeltaTime table), both forms; and 4100 > 4096 (two launches)."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=3, NR_BEAMS=6)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs, seed=72)
    c = generator(bp, table, dict(form=form))
    for nt in (300, 4100):
        dts = (np.arange(nt, dtype=np.float64) * 200e-6).astype(np.float32)
        check_1ulp(oracle, c.generate_dt(dts), oracle.generate_dt(op, table, dts))


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_non_finite_delay_values_give_the_verifiers_nans(generator, oracle, kernel):
    """Infinities and NaNs in the delay table (and a rate of 1e38): the coefficients of those pairs are NaN exactly where
    the verifier's are (cos(inf) = NaN, inf * 0 = NaN at channel 0 ...), every other element is within 1 ULP, nothing
    hangs.  The reference does not test this; the slow class (IEEE divide, fp64 sincos) is what these pairs fall into."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=6, NR_STATIONS=3, NR_BEAMS=7)
    table = rand_table(bp.n_pairs, seed=5)
    table["fDelayRate_sps"][2] = np.inf
    table["fDelay_s"][5] = np.nan
    table["fPhase_rad"][9] = -np.inf
    table["fPhaseRate_radps"][13] = np.nan
    table["fDelayRate_sps"][17] = 1e38
    c = generator(bp, table)
    dts = np.array([0.0, 0.37], dtype=np.float32)
    got = c.generate_dt(dts, kernel=kernel)
    exp = oracle.generate_dt(oracle.params_from(bp), table, dts)
    assert np.isnan(exp).sum() > 50
    assert np.array_equal(np.isnan(exp), np.isnan(got))
    fin = ~np.isnan(exp)
    check_1ulp(oracle, np.where(fin, got, 0).astype(np.float32), np.where(fin, exp, 0).astype(np.float32), tol=None)
    if kernel != 0:  # the packed binary16 output, both arithmetic forms: NaN in the same places, the rest RN-even / within 1 ulp
        for math_mode in (0, 4):
            c.g.set_tuning(math_mode=math_mode) if math_mode else c.g.set_tuning()
            h16 = c.generate_dt(dts, kernel=kernel, bitwidth=0)
            assert np.array_equal(np.isnan(h16), np.isnan(exp)), math_mode
            assert ordered_distance(np.where(fin, h16, 0).astype(np.float16), np.where(fin, exp, 0).astype(np.float16)) <= 1, math_mode


def test_seeded_fuzz_of_the_sampling_period_fft_size_and_channel_count(generator, oracle):
    """40 seeded random PARAMETER sets -- SAMPLING_PERIOD from 1e-9 to 1e-5 s, FFT_SIZE 256 .. 65536, channel counts that
    are not powers of two -- i.e. forty different divisors Ts * C for the divide by the launch constant (whose 3-operation
    form dcs_bf_create verifies per divisor) and forty different time grids: every launch shape by time index, fp32 within
    1 ULP of the verifier, fp16 the RN-even image of it."""
    from dc_sand_amd import BeamformerParameters

    rng = np.random.default_rng(20261008)
    for n in range(40):
        Ts = float(10.0 ** rng.uniform(-9, -5))
        fft = int(2 ** rng.integers(8, 17))
        A, B = int(rng.integers(1, 6)), int(rng.integers(1, 30))
        C = int(rng.choice([1, 2, 3, 7, 48, 100, 257, 1000, 1023, 1025])) if n % 2 else int(rng.integers(1, 300))
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, SAMPLING_PERIOD=Ts, FFT_SIZE=fft)
        table = rand_table(bp.n_pairs, seed=9000 + n, Ts=Ts)
        nt = int(rng.integers(1, 4))
        t0 = int(rng.integers(0, 3000))
        kernel = int(rng.integers(0, 3))
        tag = (n, Ts, fft, A, B, C, nt, t0, kernel)
        c = generator(bp, table)
        got = c.generate(t0, nt, kernel=kernel)
        check_1ulp(oracle, got, oracle.generate(oracle.params_from(bp), table, t0, nt), tol=None, tag=tag)
        if kernel != 0:
            h16 = c.generate(t0, nt, kernel=kernel, bitwidth=0)
            assert np.array_equal(h16.view(np.uint16), got.astype(np.float16).view(np.uint16)), tag


def test_two_contexts_on_two_streams_at_once(gpu, generator, oracle):
    """The one-stream-at-a-time rule is per CONTEXT (include/dcs_beamformer.h, dcs_bf_create): two contexts, each on its
    own stream, enqueue launches of every kind turn by turn -- generators in both widths, a streaming graph, both
    beamformers -- without a host synchronisation in between, and each gets its own results."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times

    shapes = [BeamformerParameters(NR_CHANNELS=300, NR_STATIONS=8, NR_BEAMS=40, NR_SAMPLES_PER_CHANNEL=32),
              BeamformerParameters(NR_CHANNELS=77, NR_STATIONS=66, NR_BEAMS=24, NR_SAMPLES_PER_CHANNEL=32)]
    nt = 3
    ctx = []
    for i, bp in enumerate(shapes):
        c = generator(bp)
        c.st = gpu.Stream()
        c.table = rand_table(bp.n_pairs, seed=400 + i)
        c.g.upload_delays(c.table, stream=c.st)
        c.ant = np.random.default_rng(i).integers(-128, 128, size=(bp.NR_CHANNELS, 2, bp.NR_STATIONS, 16, 2), dtype=np.int8)
        c.d_ant = c.upload(c.ant)
        beams = (bp.NR_CHANNELS, 2, bp.NR_BEAMS, 16, 2)
        c.out32, c.out16, c.acc, c.fused = c.tensor(nt), c.tensor(nt, bitwidth=0), Tensor(c, beams), Tensor(c, beams)
        assert c.out32.nbytes == c.g.output_bytes(1, nt)
        ctx.append(c)
    gpu.synchronize()
    for rep in range(3):  # turn by turn, nothing waits
        for c in ctx:
            for t in (c.out32, c.out16, c.acc, c.fused):
                t.refill(stream=c.st)
        for c in ctx:
            c.g.generate(c.out32.ptr, c.out32.nbytes, t0=5, nt=nt, stream=c.st)
        for c in ctx:
            c.g.generate(c.out16.ptr, c.out16.nbytes, t0=5, nt=nt, bitwidth=0, stream=c.st)
        for c in ctx:
            c.g.beamform_accumulated(c.d_ant, c.ant.nbytes, c.acc.ptr, c.acc.nbytes, 32, t_coeff=9, stream=c.st)
        for c in ctx:
            c.g.generate_and_beamform(c.d_ant, c.ant.nbytes, c.fused.ptr, c.fused.nbytes, t0=0, nt=32, stream=c.st)
    for c in ctx:
        c.st.synchronize()
        bp, op = c.bp, oracle.params_from(c.bp)
        got = c.out32.read()
        check_1ulp(oracle, got, oracle.generate(op, c.table, 5, nt))
        assert np.array_equal(c.out16.read().view(np.uint16), got.astype(np.float16).view(np.uint16))
        exp_acc = oracle.beamform_accumulated(op, c.table, delta_times(bp, 9, 1)[0], 32, c.ant)
        assert np.abs(c.acc.read() - exp_acc).max() <= accumulated_bound(bp.NR_STATIONS)
        exp_f = oracle.beamform(op, c.table, 32, c.ant)
        assert np.abs(c.fused.read() - exp_f).max() <= fused_bound(bp.NR_STATIONS)


def test_generate_dt_seeded_fuzz_over_the_whole_time_and_rate_range(generator, oracle):
    """50 seeded random cases of dcs_bf_generate_dt: fDeltaTime from 1e-7 s to 1e4 s of either sign (and 0), delay
    tables whose rates span nine decades on top of the usual ones -- so that waves land in every class (low-degree,
    full, slow: |fRotation| from 1e-3 to far beyond 32000) -- every launch shape, several time steps at once, fp32 within
    1 ULP of the verifier (the tolerance rule applies only where |fRotation| is small enough for 1e-4 to mean anything)
    and fp16 the RN-even image of the fp32 run."""
    from dc_sand_amd import BeamformerParameters

    rng = np.random.default_rng(20261007)
    for n in range(50):
        A, B, C = int(rng.integers(1, 7)), int(rng.integers(1, 40)), int(rng.integers(1, 50))
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        table = rand_table(bp.n_pairs, seed=7000 + n)
        if n % 3 == 0:  # a few pairs with rates far outside the usual range
            k = rng.integers(0, bp.n_pairs, size=max(1, bp.n_pairs // 5))
            table["fDelayRate_sps"][k] = (10.0 ** rng.uniform(-12, -3, size=k.size)) * rng.choice([-1.0, 1.0], size=k.size)
            table["fPhaseRate_radps"][k] = (10.0 ** rng.uniform(-9, 2, size=k.size)) * rng.choice([-1.0, 1.0], size=k.size)
        nt = int(rng.integers(1, 6))
        dts = ((10.0 ** rng.uniform(-7, 4, size=nt)) * rng.choice([-1.0, 1.0], size=nt)).astype(np.float32)
        if n % 7 == 0:
            dts[0] = 0.0
        kernel = int(rng.integers(0, 3))
        tag = (n, A, B, C, nt, kernel, dts.tolist())
        c = generator(bp, table)
        got = c.generate_dt(dts, kernel=kernel)
        check_1ulp(oracle, got, oracle.generate_dt(oracle.params_from(bp), table, dts), tol=None, tag=tag)
        if kernel != 0:
            h16 = c.generate_dt(dts, kernel=kernel, bitwidth=0)
            assert np.array_equal(h16.view(np.uint16), got.astype(np.float16).view(np.uint16)), tag


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_generate_at_timespec_pairs_across_a_seconds_boundary(generator, oracle, kernel):
    """dcs_bf_generate_at: (current, reference) as the reference's kernels take them.  Times 200 us apart that cross a
    seconds boundary, given normalised (tv_sec + 1, small tv_nsec: a negative nanosecond difference) and
    un-normalised (tv_nsec >= 1e9, as the reference's own launch loop builds them, BeamformerCoefficientTest.cu:232-236)."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=17, NR_STATIONS=4, NR_BEAMS=9)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs, seed=73)
    c = generator(bp, table)
    ref = (4242, 999_700_000)
    steps = [k * 200_000 for k in range(8)]  # ns; the boundary falls between k = 1 and k = 2
    unnorm = [(ref[0], ref[1] + st) for st in steps]
    norm = [(ref[0] + (ref[1] + st) // 10 ** 9, (ref[1] + st) % 10 ** 9) for st in steps]
    assert norm[2][0] == ref[0] + 1
    outs = []
    for cur in (unnorm, norm):
        outs.append(c.generate_at(cur, ref, kernel=kernel))
        check_1ulp(oracle, outs[-1], oracle.generate_at(op, table, cur, ref))
    # the two spellings of the same instants give fDeltaTime values that agree to an fp32 rounding, not always bit for bit
    assert np.max(np.abs(outs[0] - outs[1])) < 1e-3


def test_b16_arithmetic_form_device_equals_host_sweep(gpu, buffers, probes):
    """The device evaluates dcs_sincos_half2 (math_mode bit 2) to the same bits as the host build swept exhaustively
    in tests/test_numerics.py -- including the compiler's v_fma_mix{lo,hi}_f16 fusion of the last fma with the
    conversion, which must round like fmaf-then-convert (8M arguments: a single-rounding fma would differ on ~2^-13
    of them)."""
    import ctypes
    import subprocess
    from pathlib import Path

    lab_dir = Path(__file__).resolve().parent / "numerics"
    assert subprocess.run(["make", "-C", str(lab_dir)], capture_output=True).returncode == 0
    L = ctypes.CDLL(str(lab_dir / "libnumerics_lab.so"))
    L.lab_sincos_half2.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    rng = np.random.default_rng(2)
    x = np.concatenate([
        rng.uniform(-100, 100, 1 << 22).astype(np.float32),
        rng.uniform(-500, 500, 1 << 21).astype(np.float32),
        rng.uniform(-32000, 32000, 1 << 21).astype(np.float32),
        (np.arange(1, 20000, dtype=np.float32) * np.float32(np.pi / 2)),
        np.arange(0x3F800000, 0x3F800000 + (1 << 21), dtype=np.uint32).view(np.float32),  # a dense run of [1, 1.25)
    ])
    n = x.size
    b = buffers()
    dx, dw = b.upload(x), b.out(4 * n, 0xFF, 0xFF)
    probes.sincos(4, dx, n, dw, dw)
    gpu.synchronize()
    got = b.read(dw, dtype=np.uint32)
    exp = np.empty(n, np.uint32)
    L.lab_sincos_half2(x.ctypes.data, n, exp.ctypes.data)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (bad.size, x[bad[:4]], got[bad[:4]], exp[bad[:4]])


@pytest.mark.parametrize("kernel", [1, 2])
def test_b16_arithmetic_form_in_the_generator(generator, oracle, kernel):
    """math_mode = 4: b16 output from the binary16-sized arithmetic.  Every half within one binary16 ulp of
    RN16(oracle fp32) (the bar the default b16 form is held to) -- also for pairs between 500 and 32000 rad; workgroups
    holding a slow-class pair (|fRotation| >= 32000) keep the fp64 path and so reproduce the default output bit for bit;
    fp32 output is unaffected."""
    from dc_sand_amd import BeamformerParameters

    for (A, B, C) in ((64, 16, 64), (3, 5, 17), (2, 600, 40)):
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B)
        table = rand_table(bp.n_pairs, seed=C + 1)
        if A == 2:
            table["fPhase_rad"][0:100] = 2000.0     # full-degree class, still the b16 form
            table["fPhase_rad"][600] = 40000.0      # slow class: the 256-pair tile 512..767 keeps the fp64 path
        exp = oracle.generate(oracle.params_from(bp), table, 5, 3).astype(np.float16)
        plain, mode4 = generator(bp, table), generator(bp, table, dict(math_mode=4))
        dflt = plain.generate(5, 3, kernel=kernel, bitwidth=0)
        fast = mode4.generate(5, 3, kernel=kernel, bitwidth=0)
        fast_tt = generator(bp, table, dict(math_mode=4, form=3)).generate(5, 3, kernel=kernel, bitwidth=0)  # terms from the pre-pass table
        assert np.array_equal(fast.view(np.uint16), fast_tt.view(np.uint16))
        assert ordered_distance(fast, exp) <= 1
        assert ordered_distance(dflt, exp) <= 1
        differ = np.mean(fast.view(np.uint16) != dflt.view(np.uint16))
        assert differ < 0.02, differ  # ~0.5 % of halves
        if A == 2:
            f = fast.reshape(3, C, bp.n_pairs, 2).view(np.uint16)
            d = dflt.reshape(3, C, bp.n_pairs, 2).view(np.uint16)
            assert np.array_equal(f[:, :, 512:768], d[:, :, 512:768])
            assert not np.array_equal(f[:, :, 0:256], d[:, :, 0:256])
        f32a = plain.generate(5, 3, kernel=kernel, bitwidth=1)
        f32b = mode4.generate(5, 3, kernel=kernel, bitwidth=1)
        assert np.array_equal(f32a.view(np.uint32), f32b.view(np.uint32))


def test_autotune_measures_a_large_shape_once(gpu, generator, oracle):
    """dcs_bf_autotune on a tensor large enough to be tuned (2 GiB: 64 x 256 x 16384): the first call measures (~1 s), the
    second returns the cached choice at once, dcs_bf_set_tuning(NULL) forgets it; whatever was chosen, sampled rows are
    the oracle's."""
    from dc_sand_amd import BeamformerParameters

    bp = BeamformerParameters(NR_CHANNELS=16384, NR_STATIONS=64, NR_BEAMS=256)
    op = oracle.params_from(bp)
    table = rand_table(bp.n_pairs, seed=91)
    c = generator(bp, table)
    g, out = c.g, c.tensor(1)
    buf, nbytes = out.ptr, out.nbytes
    assert nbytes == g.output_bytes(1, 1)
    t0 = time.perf_counter()
    chosen = g.autotune(buf, nbytes)
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert g.autotune(buf, nbytes) == chosen
    t_second = time.perf_counter() - t0
    assert t_first > 0.2 and t_second < 0.02, (t_first, t_second)
    out.refill()
    g.generate(buf, nbytes, t0=9, nt=1)
    row = bp.n_pairs * 8
    host = np.empty((bp.NR_STATIONS, bp.NR_BEAMS, 2), dtype=np.float32)
    for ch in (0, 4097, 16383):
        gpu.memcpy_dtoh(host, buf + ch * row)
        assert oracle.max_ulp(host, oracle.generate(op, table, 9, 1, ch, 1), 1)[1] == 0
    out.guard_untouched()
    # a 1 GiB slab of the same shape takes the OTHER kernel variant (terms computed per workgroup, not read from the pre-pass
    # table): its geometry is measured and cached separately, and the full tensor's stays cached beside it
    t0 = time.perf_counter()
    slab_choice = g.autotune(buf, nbytes // 2)
    assert time.perf_counter() - t0 > 0.2
    t0 = time.perf_counter()
    assert g.autotune(buf, nbytes) == chosen and g.autotune(buf, nbytes // 2) == slab_choice
    assert time.perf_counter() - t0 < 0.02
    out.refill()
    g.generate_slab(buf, nbytes // 2, 100, bp.NR_CHANNELS // 2, t0=9, nt=1)
    gpu.memcpy_dtoh(host, buf + 17 * row)
    assert oracle.max_ulp(host, oracle.generate(op, table, 9, 1, 117, 1), 1)[1] == 0
    gpu.memcpy_dtoh(host, buf + nbytes // 2)
    assert np.all(host.view(np.uint32) == 0xFFFFFFFF)  # the row behind the slab: nothing written
    out.guard_untouched()
    g.set_tuning()  # forgets the cached choices
    t0 = time.perf_counter()
    g.autotune(buf, nbytes)
    assert time.perf_counter() - t0 > 0.2
    out.guard_untouched()


# ---- beamformer with coefficient reuse on the matrix cores ("general version"): the verifier's beamformer with
# ---- the coefficient of ONE time held (BeamformerCoefficientTest.cu:363-414); bounds: accumulated_bound, check_exact_sum
@pytest.mark.parametrize("math_mode", bc.math_modes_of(bc.PARITY + "test_beamform_accumulated_on_the_matrix_cores"))
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.PARITY + "test_beamform_accumulated_on_the_matrix_cores"))
def test_beamform_accumulated_on_the_matrix_cores(case, oracle, A, B, C, nt, math_mode):
    """dcs_bf_beamform_accumulated: the coefficients of ONE time applied to nt samples as two real contractions over the
    antennas on the matrix cores, against the verifier's beamformer with the coefficient held.  Both forms: the default
    exact fixed-point contraction on the int8 pipe (24-bit coefficients as three signed digits; sums exact) and
    (math_mode 8) the fp32 fma chain on v_mfma_f32_16x16x4_f32, at accumulated_bound(A) and at the reference's own 1e-1
    (runBeamformerTests.cpp:15); the fixed-point form also at its own, much tighter, bound (check_exact_sum).
    ACC_SHAPES cover every beam-tile count (1, 2, 4 per workgroup: coefficients shared by 4, 2, 1 waves), ragged antennas /
    beams / sample blocks, odd block counts and several workgroups per (channel, beam group) -- at these channel counts the
    launcher splits the blocks until every wave has ONE, whatever their number: what a wave does with several is held, bit
    for bit, at the DEEP_SHAPES of helpers/bacc_cases.py (tests/test_gpu_beamformer_exact.py, _beam_quant.py, _beam_power.py), and for
    the fp32 form by test_fp32_chain_form_with_several_blocks_per_wave below --, 1-4
    64-antenna chunks (whole and partial) and the 256-antenna limit -- above 64 antennas the kChain form (round 3: the
    coefficients in LDS, the integer sums chained through the chunks by the matrix instruction's accumulator), with fewer
    sample blocks than waves (waves that only make their chunk's coefficients), odd pair counts and several workgroups
    per channel.  The first shape takes the reference's ramps, the others the Case's own table (seed A + B) and samples
    (seed A)."""
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import delta_times, simulate_input

    if (A, B, C, nt) != (64, 16, 64, 256):
        c = case(A, B, C, nt)  # table indexed [b*A + a]
    else:
        bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        c = case(A, B, C, nt, table=simulate_input(bp), ant=oracle.simulate_antenna_data(oracle.params_from(bp), nt))
    dt = delta_times(c.bp, T_COEFF, 1)[0]
    exp = oracle.beamform_accumulated(c.op, c.table, dt, nt, c.ant)
    if math_mode:
        c.g.set_tuning(math_mode=math_mode)
    got = c.floats()
    assert np.all(np.isfinite(got))
    diff = np.abs(got - exp)
    assert diff.max() <= accumulated_bound(A), diff.max()
    assert oracle.compare(got, exp, 1e-1) == -1
    if math_mode == 0:
        check_exact_sum(c, got, dt)
    # fDeltaTime by value gives the same bits
    assert np.array_equal(c.floats(dt=float(dt)).view(np.uint32), got.view(np.uint32))


def test_beamform_accumulated_seeded_fuzz(case, oracle):
    """60 seeded random cases of the coefficient-reuse beamformer: antennas 1..256 (every form: staged, K-split with
    2-4 chunks, whole and partial), beams 1..90 (1, 2, 4 tiles per workgroup, partial tiles), channels, 1..40 sample
    blocks (odd counts, several workgroups per channel), either arithmetic form, time by index or by value -- each
    within accumulated_bound(A) of the verifier's loop with the coefficient held, the fixed-point form also within its own
    bound of the exact sum, nothing written outside the tensor."""
    from dc_sand_amd.generator import delta_times

    rng = np.random.default_rng(20261005)
    for n in range(60):
        A = int(rng.choice([1, 3, 17, 63, 64, 65, 100, 128, 129, 191, 192, 200, 255, 256])) if n % 2 else int(rng.integers(1, 257))
        B = int(rng.integers(1, 91))
        C = int(rng.integers(1, 5))
        nblk = int(rng.integers(1, 41))
        if A * B * C * nblk > 600000:  # keep the oracle's work small
            nblk = max(1, 600000 // (A * B * C))
        nt = 16 * nblk
        math_mode = 8 if n % 5 == 0 else 0
        table = rand_table(A * B, seed=3000 + n)  # indexed [b*A + a]
        ant = rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8)
        by_value = bool(rng.integers(0, 2))
        t_coeff = int(rng.integers(0, 2000))
        c = case(A, B, C, nt, table=table, ant=ant)
        dt = np.float32(rng.uniform(0.0, 1.5)) if by_value else delta_times(c.bp, t_coeff, 1)[0]
        exp = oracle.beamform_accumulated(c.op, table, dt, nt, ant)
        if math_mode:
            c.g.set_tuning(math_mode=math_mode)
        got = c.floats(dt=float(dt)) if by_value else c.floats(t_coeff=t_coeff)
        tag = (n, A, B, C, nt, math_mode, by_value)
        assert np.all(np.isfinite(got)), tag
        assert np.abs(got - exp).max() <= accumulated_bound(A), (tag, float(np.abs(got - exp).max()))
        if math_mode == 0:
            check_exact_sum(c, got, dt, tag)


@pytest.mark.parametrize("math_mode", bc.math_modes_of(bc.PARITY + "test_beamform_accumulated_non_finite_coefficients"))
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.PARITY + "test_beamform_accumulated_non_finite_coefficients"))
def test_beamform_accumulated_non_finite_coefficients(case, oracle, A, B, C, nt, math_mode):
    """An infinite or NaN delay value makes that pair's coefficient NaN and, with it, every sample of its beam (the plane
    concerned) in the verifier's sum: NaN * 0 = NaN.  Both forms give NaN in exactly those places -- the fixed-point form,
    whose digits cannot hold a NaN, by marking the rows -- and the other beams are unaffected."""
    table = rand_table(A * B, seed=5)  # [b*A + a]
    table["fDelayRate_sps"][2 * A + min(3, A - 1)] = np.inf       # beam 2
    table["fPhase_rad"][(B - 1) * A + A - 1] = np.nan              # the last beam, the last antenna
    ant = np.random.default_rng(1).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    c = case(A, B, C, nt, table=table, ant=ant)
    dt = np.float32(0.25)
    exp = oracle.beamform_accumulated(c.op, table, dt, nt, ant)
    assert np.isnan(exp).any() and not np.isnan(exp).all()
    if math_mode:
        c.g.set_tuning(math_mode=math_mode)
    got = c.floats(dt=float(dt))
    assert np.array_equal(np.isnan(exp), np.isnan(got))
    fin = ~np.isnan(exp)
    assert np.abs(np.where(fin, got - exp, 0)).max() <= accumulated_bound(A)


@pytest.mark.parametrize("A,B,C,nt,depth",
                         bc.shapes_of(bc.PARITY + "test_beamform_accumulated_non_finite_coefficients_in_every_pair_of_blocks", raw=True))
def test_beamform_accumulated_non_finite_coefficients_in_every_pair_of_blocks(case, oracle, record_property, A, B, C, nt, depth):
    """The shapes above give every wave one sample block.  Here the launch fills the chip, so a wave has four blocks (the
    launch geometry, read from a captured graph, must prove it): the NaN rows are marked in the first pair of blocks and
    in the later ones, kStaged (64 antennas) and kChain (130), exactly where the verifier's NaNs are."""
    table = rand_table(A * B, seed=5)  # [b*A + a]
    table["fDelayRate_sps"][2 * A + 3] = np.inf        # beam 2
    table["fPhase_rad"][(B - 1) * A + A - 1] = np.nan  # the last beam, the last antenna
    c = case(A, B, C, nt, seed=1, table=table)
    dt = np.float32(0.25)
    exp = oracle.beamform_accumulated(c.op, table, dt, nt, c.ant)
    nan = np.isnan(exp)
    assert nan[:, :, 2].all() and nan[:, :, B - 1].any() and not nan[:, :, [b for b in range(B) if b not in (2, B - 1)]].any()
    got = c.floats(dt=float(dt))
    assert np.array_equal(nan, np.isnan(got)), np.argwhere(nan != np.isnan(got))[:4]
    assert np.abs(np.where(nan, 0, got - exp)).max() <= accumulated_bound(A)
    record_property("gridDim.x, blockDim.x, blocks proven on some wave", c.prove_depth(depth, lambda s: c.enqueue_floats(False, s), kind=bc.F))


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.PARITY + "test_fp32_chain_form_with_several_blocks_per_wave"))
def test_fp32_chain_form_with_several_blocks_per_wave(case, oracle, record_property, A, B, C, nt):
    """The fp32 fma chain (math_mode 8) where a wave takes a second sample block.  Its launcher splits a workgroup's blocks
    until 4096 workgroups are launched, not 1280, so every other shape of this file leaves its waves ONE block: the stores of
    a later block (tt0 + blk * TPR + slot), the accumulators zeroed behind a block's store and the samples requested one
    stage ahead across a block boundary run here alone -- with 1, 2 and 4 beam tiles, one chunk of antennas, three with a
    partial last one and two whole ones (helpers/bacc_cases.py: FP32_DEEP_SHAPES; tests/test_launch_forms.py holds the list
    to these classes).  Against the verifier's beamformer with the coefficient held, at accumulated_bound(A) and at the
    reference's own 1e-1, every output finite, the canary behind the tensor untouched (read_beams).  The captured launch must
    prove two blocks on some wave and be the plan's.  Then samples in which every block of a channel repeats block 0: every
    block's floats must be block 0's, bit for bit -- and block 0's those of the first call -- which is sharp where the
    bound is not: a sum that starts from the previous block's, or a register set of the wrong stage."""
    from dc_sand_amd.generator import delta_times

    plan = plan_of((A, B, C, nt), bc.F8)
    assert lf.bacc_is_deep(plan), plan
    c = case(A, B, C, nt)
    dt = delta_times(c.bp, T_COEFF, 1)[0]
    exp = oracle.beamform_accumulated(c.op, c.table, dt, nt, c.ant)
    c.g.set_tuning(math_mode=8)
    got = c.floats()
    assert np.all(np.isfinite(got))
    diff = np.abs(got - exp)
    print(f"(A, B, C, nt) = {(A, B, C, nt)}: max |got - oracle| {diff.max():.3e}, bound {accumulated_bound(A):.3e}")
    assert diff.max() <= accumulated_bound(A), diff.max()
    assert oracle.compare(got, exp, 1e-1) == -1
    record_property("gridDim.x, blockDim.x, blocks proven on some wave", c.prove_depth(2, lambda s: c.enqueue_floats(False, s), kind=bc.F8))
    c.set_ant(np.ascontiguousarray(np.broadcast_to(c.ant[:, :1], c.ant.shape)))
    rep = c.floats().view(np.uint32)
    assert np.array_equal(rep[:, 0], got.view(np.uint32)[:, 0])
    bad = np.argwhere(rep != rep[:, :1])
    assert bad.size == 0, f"{bad.shape[0]} words differ from block 0's; first at [c][block][beam][sample][re, im] = {bad[0]}"


@pytest.mark.parametrize("A,B", [(64, 16), (130, 20)])
def test_beamform_accumulated_under_stream_capture(gpu, case, oracle, A, B):
    """dcs_bf_beamform_accumulated is two kernel launches and nothing else once the context's terms table exists (its one
    fDeltaTime travels in the kernel arguments): captured into a hipGraph after a first, plain, call and replayed -- a
    real-time beamformer re-launching one graph per block of samples."""
    C, nt = 5, 48
    table = rand_table(A * B, seed=61)
    rng = np.random.default_rng(7)
    ant = rng.integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
    dt = np.float32(0.0421)
    c = case(A, B, C, nt, table=table, ant=ant)
    gpu.synchronize()
    s = gpu.Stream()

    def call():
        c.g.beamform_accumulated(c.d_ant, ant.nbytes, c.d_beams, c.nbytes, nt, dt_coeff=float(dt), stream=s.handle)

    call()  # allocates the terms table
    s.synchronize()
    assert np.abs(c.read_beams() - oracle.beamform_accumulated(c.op, table, dt, nt, ant)).max() <= accumulated_bound(A)
    with hip_graph.capture(s) as graph:
        call()
    try:
        for rep in range(3):
            ant2 = rng.integers(-128, 128, size=ant.shape, dtype=np.int8)  # new samples, same coefficients: what a replay is for
            gpu.memcpy_htod(c.d_ant, ant2, stream=s.handle)
            c.refill(c.d_beams, stream=s.handle)
            graph.launch(s)
            s.synchronize()
            assert np.abs(c.read_beams() - oracle.beamform_accumulated(c.op, table, dt, nt, ant2)).max() <= accumulated_bound(A)
    finally:
        s.synchronize()
        graph.close()


def test_beamform_accumulated_slow_class_and_limits(case, generator, oracle):
    """A pair outside the fast path's range sends the coefficient generation down the slow branch (IEEE divide, fp64
    sincos); more than 256 antennas and sample counts that are not whole 16-sample blocks are refused."""
    from dc_sand_amd import BeamformerParameters, _lib

    table = rand_table(9 * 5, seed=77)
    table["fDelayRate_sps"][11] = 1e-2
    table["fDelayRate_sps"][12] = 1e-30
    ant = np.random.default_rng(3).integers(-128, 128, size=(6, 2, 9, 16, 2), dtype=np.int8)
    c = case(9, 5, 6, 32, table=table, ant=ant)
    dt = np.float32(0.25)
    exp = oracle.beamform_accumulated(c.op, table, dt, 32, ant)
    for math_mode in (0, 8):  # the fixed-point form and the fp32 chain
        c.g.set_tuning(math_mode=math_mode)
        assert np.abs(c.floats(dt=float(dt)) - exp).max() <= 2e-4 * 9
    c.g.set_tuning()
    c.refill(c.d_beams)
    with pytest.raises(_lib.DcsError) as e:
        c.g.beamform_accumulated(c.d_ant, ant.nbytes, c.d_beams, c.nbytes, 24, t_coeff=0)
    assert e.value.status == _lib.DCS_ERR_INVALID_ARGUMENT
    big = generator(BeamformerParameters(NR_CHANNELS=1, NR_STATIONS=257, NR_BEAMS=1), rand_table(257))
    with pytest.raises(_lib.DcsError) as e:
        big.g.beamform_accumulated(c.d_ant, 257 * 32, c.d_beams, 16 * 8, 16, t_coeff=0)
    assert e.value.status == _lib.DCS_ERR_UNSUPPORTED
    assert np.all(np.isnan(c.read_beams()))  # neither refused call wrote anything
