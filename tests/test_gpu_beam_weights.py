"""Per-input beam weights on the GPU (include/dcs_beam_weights.h): both beamformers against the
numerical contract -- unit weights bit-identical to the unweighted calls, 2^k weights exactly scaled, flagged antennas
(weight 0) contributing nothing even with non-finite delay values, all-zero beams 0, a non-finite weight poisoning its
own beam only, random weights within the derived bounds -- and the calls' plumbing: the fp32-chain refusal, capture
with weights changed between replays, beam shards.  Every weighted call writes into a buffer with a canary behind the
output tensor, which must stay untouched."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import bacc_cases as bc
from helpers.bacc_case import FUSED_SHAPES, T_COEFF, Case, random_weights
from helpers.beamformer_model import fused_model, normalise
from helpers.device_buffers import closed_after

pytestmark = pytest.mark.gpu


@pytest.fixture
def case(gpu, oracle):
    yield from closed_after(partial(Case, gpu, oracle))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def acc_bound_check(case, w, got):
    """Fixed-point form: within 3.7e-7 * s_b * sum_a |x_a| + 3e-7 * |exact| of the fp64 sum of g * c * x over the
    oracle's fp32 coefficients."""
    from dc_sand_amd.generator import delta_times

    A, B, C, nt = case.A, case.B, case.C, case.nt
    s, _ = normalise(w)
    coef = case.coefficients(delta_times(case.bp, T_COEFF, 1)[0])[0].astype(np.float64)  # [c][a][b][2]
    x = case.ant.astype(np.float64)
    gw = np.asarray(w, dtype=np.float64).T  # [a][b]
    exact = np.einsum("cabk,ctaik->ctbik", coef * gw[None, :, :, None], x)
    mag = np.abs(x).sum(axis=2)[:, :, None, :, :] * s.astype(np.float64)[None, None, :, None, None]
    err = np.abs(got.astype(np.float64) - exact)
    assert np.all(err <= 3.7e-7 * mag + 3e-7 * np.abs(exact) + 1e-30), float((err - 3.7e-7 * mag - 3e-7 * np.abs(exact)).max())


def fused_expected(case, w):
    """The per-sample rule restated in fp32 (helpers/beamformer_model.py: fused_model) over the oracle's coefficients."""
    from dc_sand_amd.generator import delta_times

    s, gh = normalise(w)
    return fused_model(case.coefficients(delta_times(case.bp, 0, case.nt)), case.ant, ghat=gh, scale=s)


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.WEIGHTS + "test_unit_and_power_of_two_weights_on_the_matrix_cores"))
def test_unit_and_power_of_two_weights_on_the_matrix_cores(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    base = c.run("acc")
    ones = c.run("acc", np.ones((B, A), np.float32))
    assert np.array_equal(bits(ones), bits(base))
    for k in (0.25, 8.0):
        got = c.run("acc", np.full((B, A), k, np.float32))
        assert np.array_equal(bits(got), bits((base * np.float32(k)).astype(np.float32))), k


@pytest.mark.parametrize("A,B,C,nt", FUSED_SHAPES)
def test_unit_and_power_of_two_weights_in_the_fused_kernel(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    base = c.run("fused")
    ones = c.run("fused", np.ones((B, A), np.float32))
    assert np.array_equal(bits(ones), bits(base))
    for k in (0.25, 8.0):
        got = c.run("fused", np.full((B, A), k, np.float32))
        assert np.array_equal(bits(got), bits((base * np.float32(k)).astype(np.float32))), k
    # per beam: beam b weighted 2^(b % 5 - 2)
    kb = (2.0 ** (np.arange(B) % 5 - 2)).astype(np.float32)
    got = c.run("fused", np.repeat(kb[:, None], A, axis=1))
    assert np.array_equal(bits(got), bits((base * kb[None, None, :, None, None]).astype(np.float32)))


@pytest.mark.parametrize("kind", ["acc", "fused"])
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.WEIGHTS + "test_flagged_antennas_contribute_nothing"))
def test_flagged_antennas_contribute_nothing(gpu, oracle, case, kind, A, B, C, nt):
    rng = np.random.default_rng(A * B)
    c = case(A, B, C, nt)
    w = (rng.random((B, A)) < 0.7).astype(np.float32)
    w[0, :] = 0.0   # an all-zero beam
    w[-1, :] = 1.0  # a beam with every antenna
    if A > 1:
        w[min(1, B - 1), 0] = -0.0
    got = c.run(kind, w)
    assert np.all(got[:, :, 0] == 0)
    ant = c.ant.copy()
    for b in range(B):  # per beam, the samples with that beam's flagged antennas zeroed
        z = ant.copy()
        z[:, :, w[b] == 0] = 0
        c.set_ant(z)
        ref = c.run(kind)
        assert np.all(got[:, :, b] == ref[:, :, b]), b
        if b >= 3:
            break
    c.set_ant(ant)
    # a flagged antenna (all beams) whose delay values are NaN or infinite: the beams stay finite and are the bits of the
    # same call with finite delay values there
    flag = A // 2
    w2 = np.ones((B, A), np.float32)
    w2[:, flag] = 0.0
    finite = c.run(kind, w2)
    assert np.all(np.isfinite(finite))
    bad = c.table.copy().reshape(B, A)
    bad["fDelay_s"][:, flag] = np.nan
    bad["fDelayRate_sps"][:, flag] = np.inf
    bad["fPhase_rad"][:, flag] = np.nan
    c.set_table(bad.ravel())
    got = c.run(kind, w2)
    assert np.array_equal(bits(got), bits(finite))
    # ... while unflagged, such an antenna turns every beam to NaN (what the weights are there to prevent)
    assert np.all(np.isnan(c.run(kind, np.ones((B, A), np.float32))))


@pytest.mark.parametrize("kind", ["acc", "fused"])
def test_a_non_finite_weight_poisons_its_beam_only(gpu, oracle, case, kind):
    A, B, C, nt = 70, 20, 3, 32
    c = case(A, B, C, nt)
    w = random_weights(np.random.default_rng(5), B, A, zero_beam=False)
    ref = c.run(kind, w)
    assert np.all(np.isfinite(ref))
    for b, v in ((3, np.inf), (17, np.nan), (0, -np.inf)):
        w2 = w.copy()
        w2[b, A // 3] = v
        got = c.run(kind, w2)
        assert np.all(np.isnan(got[:, :, b])), (b, v)
        others = [i for i in range(B) if i != b]
        assert np.array_equal(bits(got[:, :, others]), bits(ref[:, :, others]))


@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.WEIGHTS + "test_random_weights_on_the_matrix_cores_within_the_bound"))
def test_random_weights_on_the_matrix_cores_within_the_bound(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    w = random_weights(np.random.default_rng(A + 7 * B), B, A, zero_beam=B > 1)
    got = c.run("acc", w)
    assert np.all(np.isfinite(got))
    acc_bound_check(c, w, got)


@pytest.mark.parametrize("A,B,C,nt", [(64, 16, 3, 32), (37, 21, 2, 48), (130, 3, 2, 16), (258, 2, 2, 16), (1, 1, 1, 16)])
def test_random_weights_in_the_fused_kernel_within_the_bound(gpu, oracle, case, A, B, C, nt):
    c = case(A, B, C, nt)
    w = random_weights(np.random.default_rng(A + 7 * B), B, A, zero_beam=B > 1)
    got = c.run("fused", w)
    exp = fused_expected(c, w)
    s, _ = normalise(w)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - exp) <= 2e-5 * A * s[None, None, :, None, None] + 1e-6)


def test_random_weights_seeded_fuzz(gpu, oracle, case):
    """40 seeded cases over antennas <= 256, beams, channels and sample blocks, both beamformers, each within its bound."""
    rng = np.random.default_rng(20261016)
    for i in range(40):
        A = int(rng.choice([1, 3, 17, 63, 64, 65, 128, 129, 192, 200, 256])) if i % 2 else int(rng.integers(1, 257))
        B = int(rng.integers(1, 80))
        C = int(rng.integers(1, 4))
        nt = 16 * int(rng.integers(1, 6))
        c = case(A, B, C, nt, seed=i)
        w = random_weights(rng, B, A, zero_beam=B > 1)
        got = c.run("acc", w)
        acc_bound_check(c, w, got)
        if i % 4 == 0:
            got = c.run("fused", w)
            s, _ = normalise(w)
            assert np.all(np.abs(got - fused_expected(c, w)) <= 2e-5 * A * s[None, None, :, None, None] + 1e-6), (A, B, C, nt)
        c.close()


def test_fp32_chain_form_is_refused_and_writes_nothing(gpu, oracle, case):
    from dc_sand_amd._lib import DCS_ERR_UNSUPPORTED, DcsError

    c = case(64, 16, 2, 32)
    c.g.set_tuning(math_mode=8)
    gpu.memcpy_htod(c.d_w, np.ones((16, 64), np.float32))
    c.refill(c.d_beams)
    for kw in ({"t_coeff": T_COEFF}, {"dt_coeff": 0.0}):
        with pytest.raises(DcsError) as e:
            c.g.beamform_accumulated_weighted(c.d_ant, c.ant.nbytes, c.d_w, c.d_beams, c.nbytes, c.nt, **kw)
        assert e.value.status == DCS_ERR_UNSUPPORTED
    gpu.synchronize()
    assert np.all(c.read_beams().view(np.uint32) == 0xFFFFFFFF)


@pytest.mark.parametrize("kind", ["acc", "fused"])
def test_captured_call_picks_up_new_weights_on_replay(gpu, oracle, case, kind):
    A, B, C, nt = 130, 20, 3, 64
    c = case(A, B, C, nt)
    rng = np.random.default_rng(3)
    w1 = random_weights(rng, B, A)
    w2 = random_weights(rng, B, A)
    ref2 = c.run(kind, w2)  # (also the plain call the capture rule asks for first)
    ref1 = c.run(kind, w1)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        if kind == "acc":
            c.g.beamform_accumulated_weighted(c.d_ant, c.ant.nbytes, c.d_w, c.d_beams, c.nbytes, nt, t_coeff=T_COEFF, stream=s.handle)
        else:
            c.g.generate_and_beamform_weighted(c.d_ant, c.ant.nbytes, c.d_w, c.d_beams, c.nbytes, t0=0, nt=nt, stream=s.handle)
    for w, ref in ((w1, ref1), (w2, ref2)):
        gpu.memcpy_htod(c.d_w, w, stream=s.handle, sync=False)
        c.refill(c.d_beams, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(bits(c.read_beams()), bits(ref))
    graph.close()


@pytest.mark.parametrize("kind", ["acc", "fused"])
def test_beam_shards_reproduce_the_full_call(gpu, oracle, case, kind):
    from dc_sand_amd.beam_weights import BeamWeights
    from dc_sand_amd.sharding import beam_range, local_parameters, slice_table

    A, B, C, nt = 65, 37, 3, 48
    full = case(A, B, C, nt)
    bw = BeamWeights(full.bp)
    rng = np.random.default_rng(9)
    for b in range(B):
        bw.set(b, *random_weights(rng, 1, A, zero_beam=False)[0])
    bw.set(4, *([0.0] * A))
    bw.upload()
    ref = full.run(kind, bw.host)
    table_ab = np.ascontiguousarray(full.table.reshape(B, A).T).ravel()  # slice_table's [a][b] layout
    for rank in range(2):
        sh = beam_range(B, 2, rank)
        lp = local_parameters(full.bp, sh)
        local_ab = slice_table(table_ab, full.bp, sh).reshape(A, sh.n_beams)
        part = case(A, sh.n_beams, C, nt, table=np.ascontiguousarray(local_ab.T).ravel())
        assert part.bp.NR_BEAMS == lp.NR_BEAMS
        part.set_ant(full.ant)
        part.refill(part.d_beams)
        if kind == "acc":
            part.g.beamform_accumulated_weighted(part.d_ant, part.ant.nbytes, bw.device_ptr(sh.beam_lo), part.d_beams, part.nbytes,
                                                 nt, t_coeff=T_COEFF)
        else:
            part.g.generate_and_beamform_weighted(part.d_ant, part.ant.nbytes, bw.device_ptr(sh.beam_lo), part.d_beams,
                                                  part.nbytes, t0=0, nt=nt)
        got = part.read_beams()
        assert np.array_equal(bits(got), bits(ref[:, :, sh.beam_lo:sh.beam_hi]))
        part.close()
    bw.free()


def test_weights_change_between_calls_on_one_stream(gpu, oracle, case):
    """d_weights is read when the work runs: a copy queued between two calls on the stream applies to the second."""
    A, B, C, nt = 64, 32, 2, 32
    c = case(A, B, C, nt)
    rng = np.random.default_rng(1)
    w1, w2 = random_weights(rng, B, A), random_weights(rng, B, A)
    ref2 = c.run("acc", w2)
    s = gpu.Stream()
    d_out2 = c.alloc(c.nbytes)
    gpu.memcpy_htod(c.d_w, w1, stream=s.handle, sync=False)
    c.g.beamform_accumulated_weighted(c.d_ant, c.ant.nbytes, c.d_w, c.d_beams, c.nbytes, nt, t_coeff=T_COEFF, stream=s.handle)
    gpu.memcpy_htod(c.d_w, w2, stream=s.handle, sync=False)
    c.g.beamform_accumulated_weighted(c.d_ant, c.ant.nbytes, c.d_w, d_out2, c.nbytes, nt, t_coeff=T_COEFF, stream=s.handle)
    s.synchronize()
    got2 = np.empty(c.shape, np.float32)
    gpu.memcpy_dtoh(got2, d_out2)
    assert np.array_equal(bits(got2), bits(ref2))
    acc_bound_check(c, w1, c.read_beams())
