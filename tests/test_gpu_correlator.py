"""The correlator on the GPU (include/dcs_correlator.h).  No tolerance anywhere: the visibilities are
compared as integers and the integrated ones as float bits with the numpy model (helpers/correlator_model.py, anchored on the
CPU by tests/test_correlator_model.py).  The antenna tensor is exactly sized, so its last row ends where the allocation ends,
and every output is exactly sized with a canary behind it, which must stay untouched."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers.correlator_cases import BLOCKS, FORM_STATIONS, NR_VIS, STATIONS, WALK, shape_of
from helpers.correlator_model import MAX_BLOCKS, baseline, integrate, nr_baselines, same_bits, visibilities
from helpers.device_buffers import Context, closed_after
from helpers.examples import run_example

pytestmark = pytest.mark.gpu

PREFILL = 0xA5


def seeded_samples(A, C, nblk, seed=0):
    """Full-range int8 [C][nblk][A][16][2] with -128 and 127 at the first and the last byte."""
    ant = np.random.default_rng(100000 * A + 1000 * C + nblk + seed).integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8)
    ant.reshape(-1)[0], ant.reshape(-1)[-1] = -128, 127
    return ant


class CCase(Context):
    """One context of A stations and C channels (no delay table: the correlator has no coefficients) and buffers for up to
    max_blocks sample blocks per channel."""

    def __init__(self, gpu, A, C, max_blocks):
        super().__init__(gpu, C, A, NR_SAMPLES_PER_CHANNEL=16 * max_blocks)
        self.NB = nr_baselines(A)
        self.max_vis_bytes = C * max_blocks * self.NB * 8
        self.d_vis, self.d_out = self.out(self.max_vis_bytes), self.out(self.max_vis_bytes)

    def correlate(self, ant, n, stream=None):
        """The visibilities of ``ant`` from a device tensor of exactly its size and a prefilled output."""
        from dc_sand_amd.generator import block_visibilities_bytes

        C, nblk, A = ant.shape[:3]
        assert (C, A) == (self.C, self.A) and nblk % n == 0
        nt, nr_vis = 16 * nblk, nblk // n
        vbytes = block_visibilities_bytes(self.bp, nt, n)
        assert vbytes == C * nr_vis * self.NB * 8 <= self.max_vis_bytes
        self.refill(self.d_vis)
        self.g.correlate_block(self.upload(ant), ant.nbytes, self.d_vis, vbytes, nt, n, stream=stream)
        self.gpu.synchronize()
        return self.read(self.d_vis, vbytes, np.int32, (C, nr_vis, self.NB, 2))


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(CCase, gpu))


@pytest.mark.parametrize("A", STATIONS + FORM_STATIONS)
def test_visibilities_are_the_model(gpu, case, A):
    """STATIONS with C = 3 and every n of BLOCKS; FORM_STATIONS -- one A and more per tile count 1 .. 16, so that every unit form
    (diagonal or not, the a tiles that exist) is run: helpers/launch_forms.py, tests/test_launch_forms.py -- with C = 2 and
    n = 3, 4, 5: a masked last step, a whole one, two steps."""
    C, blocks = shape_of(A)
    c = case(A, C, max(blocks) * max(NR_VIS))
    for n in blocks:
        for nr_vis in NR_VIS:
            ant = seeded_samples(A, C, n * nr_vis)
            exp = visibilities(ant, n)
            got = c.correlate(ant, n)
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (A, n, nr_vis, np.argwhere(got != exp)[:4])
            assert np.unique(exp).size >= min(100, exp.size // 3), (A, n, nr_vis)  # no trivial expectation
            for a in range(A):
                assert not got[:, :, baseline(a, a), 1].any()


def test_waves_walk_items_beyond_the_grid(gpu, case, record_property):
    """A = 2, n = 1 and C * nr_vis a little above 4 * 2^20: one unit per (channel, visibility), so more items than the 2^20
    workgroups of four waves hold, and the waves of the first workgroups take a second item.  The grid is read from the
    captured launch (nothing allocates, so the capture may come first), and every visibility is compared.  The walk with
    several units per (channel, visibility) -- A > 64 -- would need tensors of several GiB and stays untested."""
    A, C, nr_vis, n = WALK["A"], WALK["C"], WALK["nr_vis"], WALK["n"]
    c = case(A, C, nr_vis * n)
    ant = seeded_samples(A, C, nr_vis * n)
    nt, vbytes = 16 * nr_vis * n, C * nr_vis * c.NB * 8
    d_ant = c.upload(ant)
    s = gpu.Stream()
    nodes = hip_graph.launches(s, lambda: c.g.correlate_block(d_ant, ant.nbytes, c.d_vis, vbytes, nt, n, stream=s.handle))
    s.synchronize()
    assert len(nodes) == 1, nodes
    grid, block = nodes[0]
    assert grid[1] == grid[2] == 1 and block == (256, 1, 1), nodes
    items = C * nr_vis
    record_property("gridDim.x, items", (grid[0], items))
    print(f"correlator walk: gridDim.x {grid[0]}, items {items}")
    assert grid[0] * 4 < items, f"{grid[0]} workgroups of four waves hold {items} items: raise the channel count"
    c.refill(c.d_vis)
    c.g.correlate_block(d_ant, ant.nbytes, c.d_vis, vbytes, nt, n)
    gpu.synchronize()
    got = c.read(c.d_vis, vbytes, np.int32, (C, nr_vis, c.NB, 2))
    step = 64  # the model a slice of channels at a time: it works in int64
    for c0 in range(0, C, step):
        exp = visibilities(ant[c0:c0 + step], n)
        assert np.array_equal(got[c0:c0 + step], exp), (c0, np.argwhere(got[c0:c0 + step] != exp)[:4])
    assert np.unique(got[-1]).size >= 100  # no trivial expectation, also among the items of the second trip


def test_one_hot_every_byte_of_a_row_reaches_its_baselines_with_its_sign(gpu, case):
    """A = 33 (two whole tiles and one row), n = 4.  One byte v = 3 + position of antenna a0 is non-zero, in block
    (position + a0) % 4, so every lane group's share of K is visited.  Alone: only the autocorrelation of a0 is non-zero, v^2.
    Against x = 1 + i in every other antenna: the baselines of a0 are v (1 - i) (a real part, b < a0), v (1 + i) (an imaginary
    part, b < a0) and their conjugates for a > a0, and every other word is what ones against ones or zeros give."""
    A, C, n = 33, 1, 4
    c = case(A, C, n)
    pa, pb = np.tril_indices(A)
    for a0 in (0, 1, 15, 16, 31, 32):
        for pos in range(32):
            v = 3 + pos
            blk = (pos + a0) % n
            alone = np.zeros((C, n, A, 16, 2), dtype=np.int8)
            alone[0, blk, a0].reshape(-1)[pos] = v
            got = c.correlate(alone, n)
            exp = np.zeros((C, 1, c.NB, 2), dtype=np.int32)
            exp[0, 0, baseline(a0, a0), 0] = v * v
            assert np.array_equal(got, exp), (a0, pos, np.argwhere(got != exp)[:4])
            assert np.array_equal(visibilities(alone, n), exp)
            among = np.ones_like(alone)
            among[:, :, a0] = alone[:, :, a0]
            got = c.correlate(among, n)
            exp = np.zeros((C, 1, c.NB, 2), dtype=np.int32)
            exp[0, 0, :, 0] = 2 * 16 * n  # (1 + i)(1 - i) = 2 per sample
            im_part = pos % 2 == 1
            low, high = (pa == a0) & (pb < a0), (pb == a0) & (pa > a0)
            # b < a0: x_a0 conj(1 + i); a > a0: (1 + i) conj(x_a0)
            exp[0, 0, low] = [v, v] if im_part else [v, -v]
            exp[0, 0, high] = [v, -v] if im_part else [v, v]
            exp[0, 0, baseline(a0, a0)] = [v * v, 0]
            assert np.array_equal(got, exp), (a0, pos, np.argwhere(got != exp)[:4])
            assert np.array_equal(visibilities(among, n), exp)


def test_full_scale_sits_524288_below_the_wrap(gpu, case):
    A, C, n = 16, 1, MAX_BLOCKS
    c = case(A, C, n)
    ant = np.full((C, n, A, 16, 2), -128, dtype=np.int8)
    got = c.correlate(ant, n)
    exp = visibilities(ant, n)
    assert np.array_equal(got, exp)
    assert np.all(got[..., 0] == 2_146_959_360) and not got[..., 1].any() and (1 << 31) - int(got.max()) == 524_288


def test_offset_tensors_inside_larger_allocations(gpu, case):
    """d_antenna 48 and d_vis 8 bytes into larger, prefilled allocations: the visibilities are those of the bytes from the
    offset on, and no word before or behind the visibility tensor changes."""
    A, C, n, nr_vis = 19, 2, 3, 2
    c = case(A, C, n * nr_vis)
    ant = seeded_samples(A, C, n * nr_vis, seed=5)
    vbytes = C * nr_vis * c.NB * 8
    d_ant = c.alloc(ant.nbytes + 96)
    gpu.memset(d_ant, 0x7F, ant.nbytes + 96)
    gpu.memcpy_htod(int(d_ant) + 48, ant)
    d_vis = c.out(vbytes + 16)
    c.g.correlate_block(int(d_ant) + 48, ant.nbytes, int(d_vis) + 8, vbytes, 16 * n * nr_vis, n)
    gpu.synchronize()
    host = c.read(d_vis)
    assert np.all(host[:8] == PREFILL) and np.all(host[8 + vbytes:] == PREFILL)
    got = host[8:8 + vbytes].copy().view(np.int32).reshape(C, nr_vis, c.NB, 2)
    assert np.array_equal(got, visibilities(ant, n))
    back = np.empty(ant.nbytes + 96, dtype=np.uint8)
    gpu.memcpy_dtoh(back, d_ant)
    assert np.all(back[:48] == 0x7F) and np.all(back[48 + ant.nbytes:] == 0x7F) and np.array_equal(back[48:48 + ant.nbytes].view(np.int8), ant.reshape(-1))


def test_the_autocorrelations_sum_to_the_incoherent_beam(gpu, case):
    """n = 1: sum_a re V[a][a] is the incoherent beam's block power with NULL weights, both computed on the GPU, exactly."""
    from dc_sand_amd.generator import incoherent_block_power_bytes

    A, C, nblk = 37, 3, 5
    c = case(A, C, nblk)
    ant = seeded_samples(A, C, nblk, seed=9)
    vis = c.correlate(ant, 1)
    pbytes = incoherent_block_power_bytes(c.bp, 16 * nblk)
    d_ant, d_p = c.upload(ant), c.alloc(pbytes)
    c.g.incoherent_block_power(d_ant, ant.nbytes, d_p, pbytes, 16 * nblk)
    gpu.synchronize()
    power = np.empty((C, nblk), dtype=np.uint32)
    gpu.memcpy_dtoh(power, d_p)
    autos = vis[:, :, [baseline(a, a) for a in range(A)], 0].astype(np.int64).sum(axis=2)
    assert np.array_equal(autos, power.astype(np.int64)) and np.unique(power).size == power.size


def planted_visibilities(C, nr_vis, NB, seed):
    """Full-range words, and planted ones whose sums pass 2^24 and are no floats, of both signs."""
    vis = np.random.default_rng(seed).integers(-(1 << 31), 1 << 31, size=(C, nr_vis, NB, 2), dtype=np.int64).astype(np.int32)
    vis[0, :, 0, 0] = (1 << 23) + 1 + np.arange(nr_vis) ** 2
    vis[C - 1, :, NB - 1, 1] = -(1 << 23) - 1 - np.arange(nr_vis) ** 2
    return vis


@pytest.mark.parametrize("m", (1, 3))
def test_integration_is_the_exact_sum_rounded_once(gpu, case, m):
    from dc_sand_amd.generator import visibilities_bytes

    A, C, nr_vis = 7, 3, 6
    c = case(A, C, nr_vis)
    vis = planted_visibilities(C, nr_vis, c.NB, seed=m)
    vbytes, obytes = vis.nbytes, visibilities_bytes(c.bp, nr_vis, m)
    assert obytes == (nr_vis // m) * C * c.NB * 8
    exp = integrate(vis, m)
    S = vis.astype(np.int64).reshape(C, nr_vis // m, m, c.NB, 2).sum(axis=2).transpose(1, 0, 2, 3)
    inexact = (np.abs(S) > 1 << 24) & (exp.astype(np.float64) != S)
    assert (inexact & (S > 0)).any() and (inexact & (S < 0)).any()
    prior = np.random.default_rng(m).uniform(-3e9, 3e9, size=exp.shape).astype(np.float32)
    prior.reshape(-1)[1:5] = [np.nan, np.inf, -np.inf, -0.0]
    for accumulate, want in ((False, exp), (True, integrate(vis, m, prior=prior))):
        c.refill(c.d_vis)
        gpu.memcpy_htod(c.d_vis, vis)
        c.refill(c.d_out)
        if accumulate:
            gpu.memcpy_htod(c.d_out, prior)
        c.g.integrate_visibilities(c.d_vis, vbytes, nr_vis, m, c.d_out, obytes, accumulate=accumulate)
        gpu.synchronize()
        got = c.read(c.d_out, obytes, np.float32, exp.shape)
        assert same_bits(got, want) is None, (m, accumulate, same_bits(got, want))
        assert np.array_equal(c.read(c.d_vis, vbytes, np.int32, vis.shape), vis)


def test_refusals_enqueue_nothing_and_empty_calls_succeed(gpu, case):
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    A, C, n, nr_vis = 5, 2, 2, 2
    c = case(A, C, n * nr_vis)
    ant = seeded_samples(A, C, n * nr_vis)
    nt, vbytes = 16 * n * nr_vis, C * nr_vis * c.NB * 8
    obytes = vbytes // 2
    d_ant = c.alloc(ant.nbytes + 16)
    gpu.memcpy_htod(d_ant, ant)
    c.refill(c.d_vis)
    c.refill(c.d_out)
    gpu.synchronize()
    g = c.g
    bad_calls = [
        lambda: g.correlate_block(d_ant, ant.nbytes - 1, c.d_vis, vbytes, nt, n),       # samples one byte short
        lambda: g.correlate_block(d_ant, ant.nbytes, c.d_vis, vbytes - 1, nt, n),       # visibilities one byte short
        lambda: g.correlate_block(int(d_ant) + 8, ant.nbytes, c.d_vis, vbytes, nt, n),  # 8-byte aligned only
        lambda: g.correlate_block(d_ant, ant.nbytes, int(c.d_vis) + 4, vbytes, nt, n),
        lambda: g.correlate_block(d_ant, ant.nbytes, c.d_vis, vbytes, nt + 8, n),
        lambda: g.correlate_block(d_ant, ant.nbytes, c.d_vis, vbytes, nt, 0),
        lambda: g.correlate_block(d_ant, ant.nbytes, c.d_vis, vbytes, nt, 3),           # 4 blocks are no whole visibilities of 3
        lambda: g.correlate_block(0, ant.nbytes, c.d_vis, vbytes, nt, n),
        lambda: g.integrate_visibilities(c.d_vis, vbytes - 1, nr_vis, 2, c.d_out, obytes),
        lambda: g.integrate_visibilities(c.d_vis, vbytes, nr_vis, 2, c.d_out, obytes - 1),
        lambda: g.integrate_visibilities(c.d_vis, vbytes, nr_vis, 0, c.d_out, obytes),
        lambda: g.integrate_visibilities(c.d_vis, vbytes, nr_vis, nr_vis + 1, c.d_out, obytes),
        lambda: g.integrate_visibilities(int(c.d_vis) + 4, vbytes, nr_vis, 2, c.d_out, obytes),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    # nt == 0 and nr_vis == 0 succeed and enqueue nothing, with empty buffers too
    g.correlate_block(d_ant, 0, c.d_vis, 0, 0, 5)
    g.integrate_visibilities(c.d_vis, 0, 0, 5, c.d_out, 0)
    gpu.synchronize()
    for d in (c.d_vis, c.d_out):
        assert np.all(c.read(d) == PREFILL)
    assert np.array_equal(c.correlate(ant, n), visibilities(ant, n))  # the context and the device are as usable as before


def test_captured_first_calls_pick_up_new_bytes_on_replay(gpu, case):
    """Both calls in one hipGraph as the first calls on a fresh context -- nothing allocates, so nothing has to be run outside
    the capture first -- replayed with new bytes in the same buffers."""
    from dc_sand_amd.generator import visibilities_bytes

    A, C, n, nr_vis, m = 21, 3, 3, 4, 2
    c = case(A, C, n * nr_vis)
    nt, vbytes = 16 * n * nr_vis, C * nr_vis * c.NB * 8
    obytes = visibilities_bytes(c.bp, nr_vis, m)
    sets = [seeded_samples(A, C, n * nr_vis, seed=100 + i) for i in range(3)]
    d_ant = c.alloc(sets[0].nbytes)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.g.correlate_block(d_ant, sets[0].nbytes, c.d_vis, vbytes, nt, n, stream=s.handle)
        c.g.integrate_visibilities(c.d_vis, vbytes, nr_vis, m, c.d_out, obytes, stream=s.handle)
    refs = [visibilities(x, n) for x in sets]
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    for i in (1, 2, 0):
        gpu.memcpy_htod(d_ant, sets[i], stream=s.handle, sync=False)
        c.refill(c.d_vis, stream=s.handle)
        c.refill(c.d_out, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(c.read(c.d_vis, vbytes, np.int32, refs[i].shape), refs[i]), i
        want = integrate(refs[i], m)
        assert same_bits(c.read(c.d_out, obytes, np.float32, want.shape), want) is None, i
    graph.close()


def test_the_example_verifies_itself(gpu):
    assert "OK" in run_example("correlator.py", 12, 2, 4, timeout=120)
