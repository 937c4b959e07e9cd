"""The single-pulse search on the GPU (include/dcs_single_pulse.h).  No tolerance anywhere: sums and
peaks are integers, the signal-to-noise is compared as float bits, all with the numpy model (helpers/single_pulse_model.py,
anchored on the CPU by tests/test_single_pulse_model.py).  Every buffer is exactly sized: a plane's last word that a call
may read ends where its allocation ends; every output has a 0xA5 canary behind it, which must stay untouched; the outputs
are prefilled, and every word outside the blocks of the call must stay as it was."""
import numpy as np
import pytest

from helpers import hip_graph
from helpers import single_pulse_cases as sc
from helpers.dedisperse_model import BAND_DESCENDING_64, DMS_40, dedisperse, dm_delays
from helpers.device_buffers import Context
from helpers.examples import run_example
from helpers.single_pulse_model import CHAIN, NO_TIME, chain_filterbank, nr_blocks_of, peaks, snr, sums

pytestmark = pytest.mark.gpu

PREFILL = 0x3C
PREFILL_WORD = 0x3C3C3C3C
PREFILL_FLOAT = np.frombuffer(bytes([PREFILL] * 4), np.float32)[0]


class SCase(Context):
    """One context (the search has no coefficients and uses none of its parameters; nr_beams is an argument) and the device
    buffers of its calls, exactly sized, outputs with a canary behind; all freed by close()."""

    def __init__(self, gpu):
        super().__init__(gpu, 64)

    def out(self, nbytes, prefill=PREFILL):
        return super().out(nbytes, prefill)

    def peaks(self, plane, first, T, widths, max_width, block_len, peak_blocks=None, first_block=0):
        """One dcs_bf_boxcar_peaks call into a prefilled peak plane, held to the model: the whole peak plane."""
        from dc_sand_amd.generator import boxcar_peaks_bytes, dm_time_bytes

        B, nr_dm, plane_spectra = plane.shape
        widths = np.asarray(widths, dtype=np.uint32)
        nb = nr_blocks_of(T, block_len)
        peak_blocks = first_block + nb if peak_blocks is None else peak_blocks
        nbytes = boxcar_peaks_bytes(B, nr_dm, widths.size, peak_blocks)
        assert nbytes == B * nr_dm * widths.size * peak_blocks * 8 and plane.nbytes == dm_time_bytes(B, nr_dm, plane_spectra)
        d_plane, d_widths, d_out = self.upload(plane), self.upload(widths), self.out(nbytes)
        self.g.boxcar_peaks(d_plane, plane.nbytes, plane_spectra, first, T, B, nr_dm, d_widths, widths.size, max_width, block_len,
                            d_out, nbytes, peak_blocks, first_block)
        self.gpu.synchronize()
        shape = (B, nr_dm, widths.size, peak_blocks, 2)
        got = self.read(d_out, nbytes, np.uint32, shape)
        exp = peaks(plane, first, T, widths, max_width, block_len, out=np.full(shape, PREFILL_WORD, np.uint32), first_block=first_block)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])
        return got

    def sums(self, plane, first, T, d_sums=None, accumulate=False):
        from dc_sand_amd.generator import dm_time_sums_bytes

        B, nr_dm, plane_spectra = plane.shape
        nbytes = dm_time_sums_bytes(B, nr_dm)
        assert nbytes == B * nr_dm * 16
        d_sums = self.out(nbytes) if d_sums is None else d_sums
        self.g.dm_time_sums(self.upload(plane), plane.nbytes, plane_spectra, first, T, B, nr_dm, d_sums, nbytes, accumulate=accumulate)
        self.gpu.synchronize()
        return d_sums, self.read(d_sums, nbytes, np.uint64, (B, nr_dm, 2))

    def snr(self, pk, widths, max_width, sm, count, first_block=0, nr_blocks=None, with_best=True):
        """One dcs_bf_peak_snr call into prefilled outputs, held to the model bit for bit: (snr, best or None)."""
        from dc_sand_amd.generator import best_width_bytes, peak_snr_bytes

        B, nr_dm, nw, pb, _ = pk.shape
        widths = np.asarray(widths, dtype=np.uint32)
        nr_blocks = pb - first_block if nr_blocks is None else nr_blocks
        sbytes, bbytes = peak_snr_bytes(B, nr_dm, nw, pb), best_width_bytes(B, nr_dm, pb)
        assert (sbytes, bbytes) == (B * nr_dm * nw * pb * 4, B * nr_dm * pb * 4)
        d_snr, d_best = self.out(sbytes), self.out(bbytes) if with_best else None
        self.g.peak_snr(self.upload(pk), pk.nbytes, pb, first_block, nr_blocks, B, nr_dm, self.upload(widths), nw, max_width,
                        self.upload(sm), sm.nbytes, count, d_snr, sbytes, d_best, bbytes if with_best else 0)
        self.gpu.synchronize()
        exp, exp_best = snr(pk, widths, max_width, sm, count, first_block, nr_blocks, out=np.full((B, nr_dm, nw, pb), PREFILL_FLOAT),
                            best_out=np.full((B, nr_dm, pb), PREFILL_WORD, np.uint32))
        got = self.read(d_snr, sbytes, np.float32, (B, nr_dm, nw, pb))
        bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
        assert bad.size == 0, (len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])
        if not with_best:
            return got, None
        best = self.read(d_best, bbytes, np.uint32, (B, nr_dm, pb))
        assert np.array_equal(best, exp_best), np.argwhere(best != exp_best)[:3]
        return got, best


def seeded_plane(B, nr_dm, spectra, seed, top=1 << 20):
    return np.random.default_rng(seed).integers(0, top, size=(B, nr_dm, spectra), dtype=np.uint32)


@pytest.fixture
def case(gpu):
    c = SCase(gpu)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------- block and window edges

WIDTHS_5 = sc.WIDTHS_5


def test_block_and_window_edges(case):
    """B = 2 and nr_dm = 5 with an odd plane_spectra and first_spectrum = 3: the ten series begin at every alignment."""
    for T in sc.EDGE_T:
        plane = seeded_plane(2, 5, (3 + T + 99) | 1, seed=T)
        got = case.peaks(plane, 3, T, WIDTHS_5, 100, 64, peak_blocks=nr_blocks_of(T, 64) + 3, first_block=2)
        assert np.array_equal(got[:, :, 1], got[:, :, 4])
    plane = seeded_plane(2, 5, (3 + 100 + 99) | 1, seed=4096)
    got = case.peaks(plane, 3, 100, WIDTHS_5, 100, 4096)  # one short block
    assert got.shape[3] == 1 and np.unique(got[..., 1]).size > 10
    # a window in the middle of longer series: nothing behind it is needed
    plane = seeded_plane(2, 5, 1001, seed=5)
    case.peaks(plane, 333, 300, WIDTHS_5, 100, 128, peak_blocks=4, first_block=1)


@pytest.mark.parametrize("T,block_len,max_width", sc.RUNS)
def test_several_runs_of_blocks_per_series(case, T, block_len, max_width):
    """More than 4096 times per series: several workgroups each, whose runs of blocks meet at any alignment; 192 does not
    divide 4096."""
    plane = seeded_plane(1, 3, 1 + T + max_width - 1, seed=T + block_len)
    widths = sc.run_widths(max_width)
    got = case.peaks(plane, 1, T, widths, max_width, block_len)
    assert np.unique(got[..., 1] % 64).size > 4  # no trivial expectation


# ------------------------------------------------------------------------------------------------------------------------ widths

def test_width_lists(case):
    plane = seeded_plane(1, 2, 130, seed=6)
    case.peaks(plane, 0, 130, [1], 1, 64)
    # the halo is 64 times the block
    powers = sc.POWERS
    plane = seeded_plane(1, 2, 130 + 4095, seed=7)
    got = case.peaks(plane, 0, 130, powers, 4096, 64)
    assert np.all(np.diff(got[..., 0].astype(np.int64), axis=2) > 0)  # a wider boxcar of positive words sums to more
    # widths that take no part: 0, max_width + 1 and 0xFFFFFFFF read {0, 0xFFFFFFFF}; the others are as without them
    plane = seeded_plane(2, 3, 2 + 300 + 99, seed=8)
    plain = case.peaks(plane, 2, 300, WIDTHS_5, 100, 64)
    mixed = case.peaks(plane, 2, 300, sc.MIXED, 100, 64)
    assert np.array_equal(mixed[:, :, [1, 2, 4, 6, 7]], plain)
    assert np.all(mixed[:, :, [0, 3, 5, 8], :, 0] == 0) and np.all(mixed[:, :, [0, 3, 5, 8], :, 1] == NO_TIME)
    # no width takes part
    none = case.peaks(plane, 2, 300, sc.NONE, 100, 64)
    assert np.all(none[..., 0] == 0) and np.all(none[..., 1] == NO_TIME)


# ------------------------------------------------------------------------------------ batches and blocks in every order

@pytest.mark.parametrize("nw", sc.WALK_NR_WIDTHS)
def test_batches_and_blocks_in_every_order(case, nw):
    """One to eight batches of eight widths against runs of 1, 2, 3, 4, 5 and 7 blocks (and, for two of the lists, a run of 64
    and a second workgroup with two): the four waves of a workgroup take the (batch, block) pairs in turn, so with fewer
    blocks than waves a wave skips batches, several per round where the run is one or two blocks
    (helpers/launch_forms.boxcar_walk; tests/test_launch_forms.py holds that in these shapes the waves take several pairs
    each and batches four apart).  Widths that take no part sit in the second and in the last batch.  Every word of the
    prefilled peak plane is compared."""
    widths = sc.walk_widths(nw)
    for nb in sc.WALK_NB:
        T = sc.walk_T(nb)
        plane = seeded_plane(1, 2, T + sc.WALK_MAX_WIDTH - 1, seed=100 * nw + nb)
        got = case.peaks(plane, 0, T, widths, sc.WALK_MAX_WIDTH, sc.WALK_BLOCK_LEN)
        on = [i for i, w in enumerate(widths) if 1 <= w <= sc.WALK_MAX_WIDTH]
        assert np.unique(got[:, :, on, :, 0]).size >= min(100, got[:, :, on, :, 0].size // 2)  # no trivial expectation
    if nw in sc.WALK_LONG_NR_WIDTHS:
        T = sc.WALK_LONG_T
        plane = seeded_plane(1, 2, T + sc.WALK_MAX_WIDTH - 1, seed=nw)
        got = case.peaks(plane, 0, T, widths, sc.WALK_MAX_WIDTH, sc.WALK_BLOCK_LEN)
        assert got.shape[3] == 66


# -------------------------------------------------------------------------------------------------------------------------- ties

def test_ties_take_the_first_time(case):
    plane = np.full((2, 2, 700 + 8), 12345, np.uint32)
    got = case.peaks(plane, 0, 700, [1, 9], 9, 256)
    assert np.array_equal(got[..., 1], np.broadcast_to(np.array([0, 256, 512], np.uint32), (2, 2, 2, 3)))
    assert np.all(got[:, :, 0, :, 0] == 12345) and np.all(got[:, :, 1, :, 0] == 9 * 12345)
    # one block of 256 with the same maximum at two times: in different waves' shares of the block (10 and 200), in the same
    # lanes' later round (10 and 74), in the same round (10 and 40), and next to each other
    for a, b in ((10, 200), (10, 74), (10, 40), (63, 64), (200, 255)):
        plane = np.ones((1, 1, 256 + 3), np.uint32)
        plane[0, 0, [a, b]] = 77
        got = case.peaks(plane, 0, 256, [1, 4], 4, 256)
        assert got[0, 0, 0, 0].tolist() == [77, a] and got[0, 0, 1, 0].tolist() == [80 if b - a > 3 else 156, a - 3 if b - a > 3 else b - 3]


# -------------------------------------------------------------------------------------------------------------------------- wrap

def test_sums_and_prefixes_that_wrap(case):
    T = 200
    for word in (8_355_840, 0xFFFFFFFF):  # 255 * 32768: 4096 of them pass 2^32
        plane = np.full((1, 2, T + 4095), word, np.uint32)
        got = case.peaks(plane, 0, T, [4096, 1, 1000], 4096, 64)
        assert np.all(got[:, :, 0, :, 0] == (word * 4096) % 2**32) and got[0, 0, 0, :, 1].tolist() == [0, 64, 128, 192]
    assert 8_355_840 * 4096 > 2**32
    # words of about 2^20: the prefix over 6095 words wraps, no boxcar sum does
    plane = seeded_plane(2, 2, 2000 + 4095, seed=9, top=1 << 19) + np.uint32(1 << 19)
    assert int(plane[0, 0].astype(np.uint64).sum()) > 2**32 > int(plane.max()) * 4096
    case.peaks(plane, 0, 2000, [4096, 1, 64, 2048], 4096, 128)
    # full-range words: every sum wraps
    plane = seeded_plane(1, 3, 3 + T + 299, seed=10, top=2**32)
    case.peaks(plane, 3, T, [300, 2, 17], 300, 64)


# -------------------------------------------------------------------------------------------------------------------------- sums

def test_sums(case):
    plane = seeded_plane(2, 5, 3 + 5001, seed=11, top=2**32)
    plane[1, 3, 10] = plane[1, 3, 4000] = 0xFFFFFFFF
    _, got = case.sums(plane, 3, 5001)
    exp = sums(plane, 3, 5001)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:3]
    two = np.zeros((1, 1, 9), np.uint32)
    two[0, 0, [2, 7]] = 0xFFFFFFFF
    _, got = case.sums(two, 1, 8)
    assert got[0, 0].tolist() == [2 * (2**32 - 1), (2 * (2**32 - 1) ** 2) % 2**64] and 2 * (2**32 - 1) ** 2 > 2**64
    for T in (1, 2, 3, 4, 5, 255, 1024, 1027):
        small = seeded_plane(2, 3, 2 + T, seed=T, top=2**32)
        assert np.array_equal(case.sums(small, 2, T)[1], sums(small, 2, T)), T
    # accumulate over three calls is one call; an empty call adds nothing, and without accumulate it writes zeros
    d_sums, part = case.sums(plane, 3, 1000)
    assert np.array_equal(part, sums(plane, 3, 1000))
    case.sums(plane, 1003, 2500, d_sums=d_sums, accumulate=True)
    case.sums(plane, 3503, 0, d_sums=d_sums, accumulate=True)
    _, whole = case.sums(plane, 3503, 1501, d_sums=d_sums, accumulate=True)
    assert np.array_equal(whole, exp)
    _, zero = case.sums(plane, 17, 0, d_sums=d_sums)
    assert not zero.any()


# ----------------------------------------------------------------------------------------------------------------------- S/N

def test_signal_to_noise(case):
    T, widths, max_width = 600, [1, 5, 32, 33, 0, 5], 32
    plane = seeded_plane(2, 3, T + max_width - 1, seed=12)
    plane[1, 1] = 777                      # a constant series: var = 0
    plane[0, 2] += np.uint32(0xFFF00000)   # sums that are no doubles
    pk = peaks(plane, 0, T, widths, max_width, 128)
    sm = sums(plane, 0, T)
    got, best = case.snr(pk, widths, max_width, sm, T)
    assert np.all(got[:, :, 3:5] == -np.inf) and not got[1, 1, :3].any() and np.all(best[1, 1] == 0)
    assert np.isfinite(got[:, :, :3]).all() and np.unique(got[:, :, :3]).size > 50 and set(np.unique(best)) <= {0, 1, 2}
    assert np.array_equal(got[:, :, 1], got[:, :, 5])  # the duplicate width: the same figures, and index 1 wins over 5
    # every width dropped; d_best NULL; a range of blocks
    _, none = case.snr(pk[:, :, 3:5].copy(), widths[3:5], max_width, sm, T)
    assert np.all(none == NO_TIME)
    case.snr(pk, widths, max_width, sm, T, with_best=False)
    part, part_best = case.snr(pk, widths, max_width, sm, T, first_block=2, nr_blocks=2)
    assert np.array_equal(part[..., 2:4], got[..., 2:4]) and np.array_equal(part_best[..., 2:4], best[..., 2:4])
    case.snr(pk, widths, max_width, sm, T, first_block=5, nr_blocks=0)
    # a count that is not the number of words, and sums past 2^53
    big = sm.copy()
    big[..., 1] |= np.uint64(1 << 63)
    case.snr(pk, widths, max_width, big, 2**40 + 1)


# ------------------------------------------------------------------------------------------------------------------ refusals

def test_short_buffers_are_refused_and_nothing_is_enqueued(case, gpu):
    """The refusals that come after the version check, with DCS_ERR_INVALID_ARGUMENT."""
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError
    from dc_sand_amd.generator import best_width_bytes, boxcar_peaks_bytes, dm_time_sums_bytes, peak_snr_bytes

    B, nr_dm, T, nw, max_width, pb = 2, 3, 200, 4, 20, 4
    g = case.g
    plane = seeded_plane(B, nr_dm, T + max_width - 1, seed=13)
    ps, pbytes = plane.shape[2], plane.nbytes
    sbytes, kbytes = dm_time_sums_bytes(B, nr_dm), boxcar_peaks_bytes(B, nr_dm, nw, pb)
    nbytes, bbytes = peak_snr_bytes(B, nr_dm, nw, pb), best_width_bytes(B, nr_dm, pb)
    d_plane, d_widths = case.upload(plane), case.upload(np.array([1, 2, 20, 5], np.uint32))
    d_sums, d_peaks, d_snr, d_best = case.out(sbytes), case.out(kbytes), case.out(nbytes), case.out(bbytes)

    def pk(plane_bytes=pbytes, beams=B, dms=nr_dm, widths=nw, out_bytes=kbytes):
        return g.boxcar_peaks(d_plane, plane_bytes, ps, 0, T, beams, dms, d_widths, widths, max_width, 64, d_peaks, out_bytes, pb)

    def sn(peak_bytes=kbytes, sum_bytes=sbytes, snr_bytes=nbytes, best_bytes=bbytes, beams=B, widths=nw):
        return g.peak_snr(d_peaks, peak_bytes, pb, 0, pb, beams, nr_dm, d_widths, widths, max_width, d_sums, sum_bytes, T, d_snr,
                          snr_bytes, d_best, best_bytes)

    calls = [
        lambda: g.dm_time_sums(d_plane, pbytes - 1, ps, 0, T, B, nr_dm, d_sums, sbytes),
        lambda: g.dm_time_sums(d_plane, pbytes, ps, 0, T, B, nr_dm, d_sums, sbytes - 1),
        lambda: g.dm_time_sums(d_plane, pbytes, ps, 0, T, B + 1, nr_dm, d_sums, sbytes + 16),
        lambda: g.dm_time_sums(d_plane, 2**64 - 1, ps, 0, T, 2**32 - 1, 2**32 - 1, d_sums, sbytes),
        lambda: pk(plane_bytes=pbytes - 1), lambda: pk(out_bytes=kbytes - 1), lambda: pk(beams=B + 1), lambda: pk(dms=nr_dm + 1),
        lambda: pk(widths=nw + 1), lambda: pk(beams=2**32 - 1, dms=2**32 - 1, widths=2**32 - 1, plane_bytes=2**64 - 1),
        lambda: sn(peak_bytes=kbytes - 1), lambda: sn(sum_bytes=sbytes - 1), lambda: sn(snr_bytes=nbytes - 1),
        lambda: sn(best_bytes=bbytes - 1), lambda: sn(beams=B + 1), lambda: sn(widths=nw + 1),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    gpu.synchronize()
    for d, n in ((d_sums, sbytes), (d_peaks, kbytes), (d_snr, nbytes), (d_best, bbytes)):
        assert np.all(case.read(d, n, np.uint8, (-1,)) == PREFILL)
    # nothing to do: nothing is written, and the calls succeed
    g.boxcar_peaks(d_plane, pbytes, ps, 0, 0, B, nr_dm, d_widths, nw, max_width, 64, d_peaks, kbytes, pb)
    g.boxcar_peaks(d_plane, pbytes, ps, 0, T, B, nr_dm, d_widths, 0, max_width, 64, d_peaks, 0, pb)
    g.boxcar_peaks(d_plane, 0, ps, 0, T, B, 0, d_widths, nw, max_width, 64, d_peaks, 0, pb)
    g.dm_time_sums(d_plane, 0, ps, 0, T, B, 0, d_sums, 0)
    g.peak_snr(d_peaks, kbytes, pb, 2, 0, B, nr_dm, d_widths, nw, max_width, d_sums, sbytes, T, d_snr, nbytes, d_best, bbytes)
    gpu.synchronize()
    for d, n in ((d_sums, sbytes), (d_peaks, kbytes), (d_snr, nbytes), (d_best, bbytes)):
        assert np.all(case.read(d, n, np.uint8, (-1,)) == PREFILL)


# ------------------------------------------------------------------------------------------------------------------ capture

def test_three_calls_captured_and_replayed_with_new_contents(case, gpu):
    """All three as first calls on a fresh context, captured; replayed after the plane words, the width list and the sums
    that the signal-to-noise reads were changed on the device: the outputs follow the new contents."""
    from dc_sand_amd.generator import best_width_bytes, boxcar_peaks_bytes, dm_time_bytes, dm_time_sums_bytes, peak_snr_bytes

    B, nr_dm, T, nw, max_width, block_len, first, first_block, pb = 2, 3, 700, 4, 50, 128, 2, 1, 8
    ps = first + T + max_width - 1
    nb = nr_blocks_of(T, block_len)
    c = case
    pbytes, sbytes = dm_time_bytes(B, nr_dm, ps), dm_time_sums_bytes(B, nr_dm)
    kbytes, nbytes, bbytes = boxcar_peaks_bytes(B, nr_dm, nw, pb), peak_snr_bytes(B, nr_dm, nw, pb), best_width_bytes(B, nr_dm, pb)
    d_plane, d_widths, d_sums_in = c.alloc(pbytes), c.alloc(nw * 4), c.alloc(sbytes)
    d_sums, d_peaks, d_snr, d_best = c.out(sbytes), c.out(kbytes), c.out(nbytes), c.out(bbytes)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        c.g.dm_time_sums(d_plane, pbytes, ps, first, T, B, nr_dm, d_sums, sbytes, stream=s.handle)
        c.g.boxcar_peaks(d_plane, pbytes, ps, first, T, B, nr_dm, d_widths, nw, max_width, block_len, d_peaks, kbytes, pb, first_block,
                         stream=s.handle)
        c.g.peak_snr(d_peaks, kbytes, pb, first_block, nb, B, nr_dm, d_widths, nw, max_width, d_sums_in, sbytes, T, d_snr, nbytes,
                     d_best, bbytes, stream=s.handle)
    seen = []
    for i, widths in enumerate(([1, 8, 50, 3], [0, 50, 2, 2], [7, 51, 1, 20])):
        plane = seeded_plane(B, nr_dm, ps, seed=80 + i)
        widths = np.array(widths, np.uint32)
        sums_in = sums(plane, i, T)  # of another window each time: not what the captured sums call makes
        gpu.memcpy_htod(d_plane, plane, stream=s.handle, sync=False)
        gpu.memcpy_htod(d_widths, widths, stream=s.handle, sync=False)
        gpu.memcpy_htod(d_sums_in, sums_in, stream=s.handle, sync=False)
        for d, n in ((d_peaks, kbytes), (d_snr, nbytes), (d_best, bbytes)):
            gpu.memset(d, PREFILL, n, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        assert np.array_equal(c.read(d_sums, sbytes, np.uint64, (B, nr_dm, 2)), sums(plane, first, T)), i
        exp = peaks(plane, first, T, widths, max_width, block_len, out=np.full((B, nr_dm, nw, pb, 2), PREFILL_WORD, np.uint32),
                    first_block=first_block)
        got = c.read(d_peaks, kbytes, np.uint32, exp.shape)
        assert np.array_equal(got, exp), (i, np.argwhere(got != exp)[:3])
        exp_snr, exp_best = snr(exp, widths, max_width, sums_in, T, first_block, nb, out=np.full((B, nr_dm, nw, pb), PREFILL_FLOAT),
                                best_out=np.full((B, nr_dm, pb), PREFILL_WORD, np.uint32))
        got_snr = c.read(d_snr, nbytes, np.uint32, exp_snr.shape)
        assert np.array_equal(got_snr, exp_snr.view(np.uint32)), (i, np.argwhere(got_snr != exp_snr.view(np.uint32))[:3])
        assert np.array_equal(c.read(d_best, bbytes, np.uint32, exp_best.shape), exp_best), i
        seen.append((got, got_snr))
    assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[1][1], seen[2][1])
    graph.close()


# -------------------------------------------------------------------------------------------------------------------- chain

def test_the_chain_recovers_the_injected_pulse(case, gpu):
    """Noise bytes with a pulse of 8 spectra along the track of DM index 20 -> dm_delays -> dedisperse_q8 -> the three calls:
    every output is the model's, and the largest signal-to-noise of the search is the pulse (the figures are those of
    tests/test_single_pulse_model.py)."""
    from dc_sand_amd.generator import (best_width_bytes, boxcar_peaks_bytes, dm_delays_bytes, dm_time_bytes, dm_time_sums_bytes,
                                       peak_snr_bytes)

    k = CHAIN
    C, outputs, widths, max_width, block_len = k["C"], k["outputs"], np.array(k["widths"], np.uint32), k["max_width"], k["block_len"]
    table = dm_delays(C, *BAND_DESCENDING_64, DMS_40)
    nr_dm, max_delay = table.shape[0], int(table.max())
    fb = chain_filterbank(table, seed=0)
    rows = fb.shape[1]
    T = outputs - max_width + 1
    nb = nr_blocks_of(T, block_len)
    tbytes, pbytes, sbytes = dm_delays_bytes(case.bp, nr_dm), dm_time_bytes(1, nr_dm, outputs), dm_time_sums_bytes(1, nr_dm)
    kbytes, nbytes, bbytes = boxcar_peaks_bytes(1, nr_dm, widths.size, nb), peak_snr_bytes(1, nr_dm, widths.size, nb), best_width_bytes(1, nr_dm, nb)
    d_fb, d_dms, d_widths = case.upload(fb), case.upload(DMS_40), case.upload(widths)
    d_delays, d_plane, d_sums = case.out(tbytes), case.out(pbytes), case.out(sbytes)
    d_peaks, d_snr, d_best = case.out(kbytes), case.out(nbytes), case.out(bbytes)
    g = case.g
    g.dm_delays(*BAND_DESCENDING_64, d_dms, nr_dm, d_delays, tbytes)
    g.dedisperse_q8(d_fb, fb.nbytes, rows, 0, outputs, 1, d_delays, nr_dm, max_delay, d_plane, pbytes, outputs)
    g.dm_time_sums(d_plane, pbytes, outputs, 0, k["count"], 1, nr_dm, d_sums, sbytes)
    g.boxcar_peaks(d_plane, pbytes, outputs, 0, T, 1, nr_dm, d_widths, widths.size, max_width, block_len, d_peaks, kbytes, nb)
    g.peak_snr(d_peaks, kbytes, nb, 0, nb, 1, nr_dm, d_widths, widths.size, max_width, d_sums, sbytes, k["count"], d_snr, nbytes,
               d_best, bbytes)
    gpu.synchronize()
    plane = dedisperse(fb, table, 0, outputs, max_delay)
    assert np.array_equal(case.read(d_plane, pbytes, np.uint32, plane.shape), plane)
    exp_sums, exp_peaks = sums(plane, 0, k["count"]), peaks(plane, 0, T, widths, max_width, block_len)
    exp_snr, exp_best = snr(exp_peaks, widths, max_width, exp_sums, k["count"])
    assert np.array_equal(case.read(d_sums, sbytes, np.uint64, exp_sums.shape), exp_sums)
    assert np.array_equal(case.read(d_peaks, kbytes, np.uint32, exp_peaks.shape), exp_peaks)
    got_snr, got_best = case.read(d_snr, nbytes, np.float32, exp_snr.shape), case.read(d_best, bbytes, np.uint32, exp_best.shape)
    assert np.array_equal(got_snr.view(np.uint32), exp_snr.view(np.uint32)) and np.array_equal(got_best, exp_best)
    at = np.unravel_index(np.argmax(got_snr), got_snr.shape)
    assert at == (0, k["dm_index"], 3, 1) and got_best[0, k["dm_index"], 1] == 3
    assert case.read(d_peaks, kbytes, np.uint32, exp_peaks.shape)[at][1] == k["row"]
    assert got_snr[at] > 23.0 and np.sort(got_snr.ravel())[-2] < 18.0 and np.delete(got_snr[0], np.arange(18, 23), axis=0).max() < 9.3


# ------------------------------------------------------------------------------------------------------------------ example

def test_example_runs_and_verifies_itself(gpu):
    out = run_example("single_pulse_search.py", 64, 2, 24, 1024)
    assert "bit-identical to the model: True" in out and "the pulse is recovered: True" in out
