"""The RFI flagger on the GPU (include/dcs_rfi.h).  No tolerance anywhere: sums, flags, masks, counts
and cleaned bytes are integers and are compared with the numpy model (helpers/rfi_model.py, anchored on the CPU by
tests/test_rfi_model.py) bit for bit.  Every buffer is exactly sized: the filterbanks' last row ends where their allocation
ends; every output is prefilled and has a 0xA5 canary behind it, which must stay untouched; the rows of the cleaned
filterbank outside the window must stay as they were."""
from functools import partial

import numpy as np
import pytest

from helpers import hip_graph
from helpers import rfi_cases as rc
from helpers import rfi_model as rm
from helpers.dedisperse_model import BAND_DESCENDING_64, DMS_40, dedisperse, dm_delays
from helpers.device_buffers import Context, closed_after
from helpers.examples import run_example
from helpers.filterbank_model import filterbank

pytestmark = pytest.mark.gpu

PREFILL = 0x3C


def gen_thresholds(thr):
    from dc_sand_amd.generator import RfiThresholds

    return RfiThresholds(thr.mean_thr, thr.mean_floor, thr.var_thr, thr.var_floor, thr.zero_dm_thr, thr.zero_dm_floor, thr.max_bad_blocks)


class RCase(Context):
    """One context of C channels (nr_beams is an argument of every call) and the device buffers of its calls, exactly sized,
    outputs prefilled with a canary behind; all freed by close()."""

    def moments(self, fb, first, nb, n, zero_dm=True, d_fb=None):
        """dcs_bf_rfi_moments from prefilled outputs: (cell sums, zero-DM series or None) as the device made them."""
        from dc_sand_amd.generator import rfi_cell_sums_bytes, rfi_zero_dm_bytes

        B, in_spectra, C = fb.shape
        assert C == self.C and fb.dtype == np.uint8
        sbytes, zbytes = rfi_cell_sums_bytes(self.bp, B, nb), rfi_zero_dm_bytes(B, nb * n)
        assert (sbytes, zbytes) == (B * nb * C * 8, B * nb * n * 4)
        d_fb = self.upload(fb) if d_fb is None else d_fb  # exactly fb.nbytes: the last row ends where the allocation ends
        d_cs = self.out(sbytes, PREFILL)
        d_z = self.out(zbytes, PREFILL) if zero_dm else None
        self.g.rfi_moments(d_fb, fb.nbytes, in_spectra, first, nb, n, B, d_cs, sbytes, d_z, zbytes if zero_dm else 0)
        self.gpu.synchronize()
        cs = self.read(d_cs, sbytes, np.uint32, (B, nb, C, 2))
        return cs, (self.read(d_z, zbytes, np.uint32, (B, nb * n)) if zero_dm else None)

    def flags(self, cs, z, n, thr):
        """dcs_bf_rfi_flags on host statistics (uploaded): (cell flags, channel masks, spectrum flags or None, counts)."""
        from dc_sand_amd.generator import (rfi_cell_flags_bytes, rfi_channel_mask_bytes, rfi_counts_bytes,
                                           rfi_spectrum_flags_bytes)

        B, nb, C, _ = cs.shape
        W = nb * n
        fbytes, mbytes, cbytes, pbytes = rfi_cell_flags_bytes(self.bp, B, nb), rfi_channel_mask_bytes(self.bp, B), rfi_counts_bytes(B), \
            rfi_spectrum_flags_bytes(B, W)
        assert (fbytes, mbytes, cbytes, pbytes) == (B * nb * C, B * C, B * 12, B * W)
        d_cs = self.upload(np.ascontiguousarray(cs, dtype=np.uint32))
        d_z = None if z is None else self.upload(np.ascontiguousarray(z, dtype=np.uint32))
        d_cf, d_cm, d_cnt = self.out(fbytes, PREFILL), self.out(mbytes, PREFILL), self.out(cbytes, PREFILL)
        d_sf = None if z is None else self.out(pbytes, PREFILL)
        self.g.rfi_flags(d_cs, cs.nbytes, nb, n, B, d_cf, fbytes, d_cm, mbytes, d_cnt, cbytes, thresholds=gen_thresholds(thr),
                         d_zero_dm=d_z, zero_dm_bytes=0 if z is None else z.nbytes, d_spectrum_flags=d_sf,
                         spectrum_flags_bytes=0 if z is None else pbytes)
        self.gpu.synchronize()
        return (self.read(d_cf, fbytes, np.uint8, (B, nb, C)), self.read(d_cm, mbytes, np.uint8, (B, C)),
                None if z is None else self.read(d_sf, pbytes, np.uint8, (B, W)), self.read(d_cnt, cbytes, np.uint32, (B, 3)))

    def check_flags(self, cs, z, n, thr):
        got, exp = self.flags(cs, z, n, thr), rm.flags(cs, z, n, thr)
        for name, g, e in zip(("cell flags", "channel mask", "spectrum flags", "counts"), got, exp):
            assert (g is None) == (e is None), name
            if e is not None:
                assert g.dtype == e.dtype and np.array_equal(g, e), (name, thr, np.argwhere(g != e)[:4])
        return got

    def clean(self, fb, first, nb, n, fill, cell=None, mask=None, spec=None, out_spectra=None, first_out=0, count=True, in_place=False,
              offset=None):
        """dcs_bf_rfi_clean_q8 against the model, out of place into a prefilled tensor or in place: (bytes, replaced).  With
        ``offset`` every flag tensor lies that many bytes into an allocation of its own, between bytes that would replace
        what it keeps if they were read as its flags: 0xFF around the cell and the spectrum flags, 0 around the channel mask."""
        B, in_spectra, C = fb.shape
        W = nb * n
        d_fb = self.out(fb.nbytes) if in_place else self.upload(fb)
        if in_place:
            self.gpu.memcpy_htod(d_fb, fb)
            out_spectra, first_out, d_out, pre = in_spectra, first, d_fb, fb
        else:
            out_spectra = first_out + W if out_spectra is None else out_spectra
            d_out = self.out(B * out_spectra * C, PREFILL)
            pre = np.full((B, out_spectra, C), PREFILL, np.uint8)

        def up(a, around=0xFF):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.uint8)
            if offset is None:
                return self.upload(a)
            host = np.full(offset + a.size + 16, around, np.uint8)
            host[offset:offset + a.size] = a.ravel()
            return int(self.upload(host)) + offset

        d_rep = self.out(B * 8, 0) if count else None
        self.g.rfi_clean_q8(d_fb, fb.nbytes, in_spectra, first, nb, n, B, fill, d_out, B * out_spectra * C, out_spectra,
                            first_out=first_out, d_cell_flags=up(cell), d_channel_mask=up(mask, 0), d_spectrum_flags=up(spec),
                            d_replaced=d_rep)
        self.gpu.synchronize()
        got = self.read(d_out, B * out_spectra * C, np.uint8, (B, out_spectra, C))
        exp, replaced = rm.clean(fb, first, nb, n, fill, cell, mask, spec, out=pre, first_out=first_out)
        assert np.array_equal(got, exp), np.argwhere(got != exp)[:4]
        if count:
            assert np.array_equal(self.read(d_rep, B * 8, np.uint64, (B,)), replaced)
        return got, replaced


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(RCase, gpu))


def seeded_bytes(B, rows, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, rows, C), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ moments

CHANNELS, MORE_CHANNELS, BLOCK_LENS = rc.CHANNELS, rc.MORE_CHANNELS, rc.BLOCK_LENS  # the tables: helpers/rfi_cases.py
CASES = rc.moments_cases()
_ALL = [c for C in CHANNELS for c in CASES[C]]
assert len(_ALL) == 49 and {c[1] for c in _ALL} == {1, 2, 7} and {c[2] for c in _ALL} == {1, 3} and {c[3] for c in _ALL} == {0, 5}
assert all({c[0] for c in CASES[C]} == set(BLOCK_LENS) for C in CASES)


@pytest.mark.parametrize("C", CHANNELS + MORE_CHANNELS)
def test_moments_are_the_model(gpu, case, C):
    c = case(C)
    for i, (n, nb, B, first) in enumerate(CASES[C]):
        fb = seeded_bytes(B, first + nb * n + (3 if i % 2 else 0), C, seed=1000 * C + n)
        cs, z = c.moments(fb, first, nb, n)
        exp_cs, exp_z = rm.moments(fb, first, nb, n)
        assert np.array_equal(cs, exp_cs), (n, nb, B, first, np.argwhere(cs != exp_cs)[:4])
        assert np.array_equal(z, exp_z), (n, nb, B, first, np.argwhere(z != exp_z)[:4])
        if i % 2 == 0:  # without the zero-DM series: the same cell sums
            alone, none = c.moments(fb, first, nb, n, zero_dm=False)
            assert none is None and np.array_equal(alone, exp_cs)


FORM_CASES = rc.form_cases()


@pytest.mark.parametrize("C", rc.FORM_CHANNELS)
def test_moments_of_every_form_are_the_model(gpu, case, C):
    """The (U, L) pairs, the partial tiles with whole lanes off and the trip counts of the zero-DM reduction that the tables
    above leave out (tests/test_rfi_forms.py has the census), every case with and without the zero-DM series."""
    c = case(C)
    for i, (n, nb, B, first) in enumerate(FORM_CASES[C]):
        fb = seeded_bytes(B, first + nb * n + (2 if i % 2 else 0), C, seed=7000 * C + n)
        exp_cs, exp_z = rm.moments(fb, first, nb, n)
        d_fb = c.upload(fb)
        cs, z = c.moments(fb, first, nb, n, d_fb=d_fb)
        assert np.array_equal(cs, exp_cs), (n, nb, B, first, np.argwhere(cs != exp_cs)[:4])
        assert np.array_equal(z, exp_z), (n, nb, B, first, np.argwhere(z != exp_z)[:4])
        alone, none = c.moments(fb, first, nb, n, zero_dm=False, d_fb=d_fb)
        assert none is None and np.array_equal(alone, exp_cs), (n, nb, B, first)


def test_moments_of_the_longest_block_at_full_scale(gpu, case):
    """block_len = 65536 of bytes 255: s2 = 4 261 478 400, the largest sum there is, and 2 blocks of it."""
    c = case(16)
    n = 65536
    fb = np.full((1, 2 * n, 16), 255, np.uint8)
    cs, z = c.moments(fb, 0, 2, n)
    assert np.all(cs[..., 0] == 255 * n) and np.all(cs[..., 1] == 4_261_478_400) and np.all(z == 16 * 255)
    got = c.check_flags(cs, z, n, rm.Thresholds())
    assert not got[0].any() and got[1].all() and not got[2].any() and not got[3].any()


def test_nothing_to_do_writes_nothing(gpu, case):
    c = case(64)
    d_fb, d_cs, d_z = c.upload(seeded_bytes(1, 8, 64, 1)), c.out(64), c.out(64)
    c.g.rfi_moments(d_fb, 512, 8, 8, 0, 4, 1, d_cs, 0, d_z, 0)
    c.g.rfi_clean_q8(d_fb, 512, 8, 8, 0, 4, 1, 7, d_cs, 0, 0)
    gpu.synchronize()
    assert np.all(c.read(d_cs) == 0xA5) and np.all(c.read(d_z) == 0xA5)


# -------------------------------------------------------------------------------------------------------------------- flags

THRESHOLDS = [rm.Thresholds(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0), rm.Thresholds(6.0, 0.0, 6.0, 0.0, 6.0, 0.0, 2),
              rm.Thresholds(1e300, 0.0, 1e300, 0.0, 1e300, 0.0, 0), rm.Thresholds(3.0, 50.0, 2.0, 1e5, 2.5, 30.0, 1)]


@pytest.mark.parametrize("C", CHANNELS)
def test_flags_of_the_devices_own_sums(gpu, case, C):
    """Noise around 128 with a raised, a loud and a dead channel and a burst, through moments and flags on the device; the
    thresholds 0, 6 and 1e300, and max_bad_blocks 0, 2 and nr_blocks."""
    c = case(C)
    rng = np.random.default_rng(C)
    for n, nb, B in rc.own_sums_shapes(C):
        fb = np.clip(np.rint(rng.normal(128, 16, (B, nb * n, C))), 0, 255).astype(np.uint8)
        fb[0, :, C // 2] = 128
        fb[B - 1, :, C // 3] = np.clip(np.rint(rng.normal(128, 40, nb * n)), 0, 255)
        fb[0, : n, C - 1] = np.minimum(fb[0, :n, C - 1].astype(np.int64) + 20, 255)
        fb[B - 1, n // 2] = np.minimum(fb[B - 1, n // 2].astype(np.int64) + 30, 255)
        cs, z = c.moments(fb, 0, nb, n)
        assert np.array_equal(cs, rm.moments(fb, 0, nb, n)[0])
        seen = []
        for thr in THRESHOLDS + [rm.Thresholds(max_bad_blocks=nb)]:
            seen.append(c.check_flags(cs, z, n, thr))
        c.check_flags(cs, None, n, THRESHOLDS[1])  # without the zero-DM part: the third count is 0
        assert seen[4][1].all()  # no channel has more than nr_blocks bad blocks
        if C >= 64:
            assert seen[0][0].any() and seen[1][0].any() and seen[1][2].any() and not seen[1][0].all()
            assert not seen[2][0].all()


def sums_of(columns):
    """Cell sums uint32 [1][1][C][2] of hand-made columns of bytes, one tuple per channel, and the block length."""
    fb = np.array(columns, np.uint8).T[None]
    return rm.moments(fb, 0, 1, fb.shape[1])[0], fb.shape[1]


def test_flags_of_hand_made_sums(gpu, case):
    below_2 = float(np.nextafter(2.0, 0.0))
    # the strict compare on m: 0 4 8 12 16 has the median 8 and the MAD 4, so thr = 2 puts the limit ON both ends
    cs, n = sums_of([(0,), (4,), (8,), (12,), (16,)])
    c = case(5)
    cell = c.check_flags(cs, None, n, rm.Thresholds(mean_thr=2.0, var_thr=0.0))[0]
    assert not cell.any()
    cell = c.check_flags(cs, None, n, rm.Thresholds(mean_thr=below_2, var_thr=0.0))[0]
    assert cell[0, 0].tolist() == [1, 0, 0, 0, 1]
    # and on q = 0 2 6 8 14 (median 6, MAD 4, the last at distance 8) with m = 0 1 3 2 4
    cs, n = sums_of([(0, 0, 0), (0, 0, 1), (0, 1, 2), (0, 0, 2), (0, 1, 3)])
    q = n * cs[0, 0, :, 1].astype(np.int64) - cs[0, 0, :, 0].astype(np.int64) ** 2
    assert q.tolist() == [0, 2, 6, 8, 14]
    cell = c.check_flags(cs, None, n, rm.Thresholds(mean_thr=1e300, var_thr=2.0))[0]
    assert not cell.any()
    cell = c.check_flags(cs, None, n, rm.Thresholds(mean_thr=1e300, var_thr=below_2))[0]
    assert cell[0, 0].tolist() == [0, 0, 0, 0, 2]
    # ties: two values only; all equal; with a MAD of 0 the floor decides
    cs, n = sums_of([(7, 7)] * 3 + [(9, 9)] * 2)
    for thr in (rm.Thresholds(), rm.Thresholds(mean_floor=3.0), rm.Thresholds(mean_floor=4.0), rm.Thresholds(0, 0, 0, 0, 0, 0)):
        c.check_flags(cs, None, n, thr)
    assert c.check_flags(cs, None, n, rm.Thresholds())[0][0, 0].tolist() == [0, 0, 0, 1, 1]
    assert not c.check_flags(cs, None, n, rm.Thresholds(mean_floor=4.0))[0].any()
    cs, n = sums_of([(200, 100)] * 5)
    assert not c.check_flags(cs, None, n, rm.Thresholds(0, 0, 0, 0, 0, 0))[0].any()
    # the zero-DM series by hand: the same strict compare, and ties
    z = np.array([[0, 4, 8, 12, 16, 8, 8, 8]], np.uint32)  # median 8, distances 8 4 0 4 8 0 0 0, MAD 0
    cs, n = sums_of([(7,)] * 5)  # blocks of one spectrum: q = s2 - s1^2 = 0
    assert n == 1
    cs8 = np.tile(cs, (1, 8, 1, 1))
    for thr in (rm.Thresholds(zero_dm_thr=2.0), rm.Thresholds(zero_dm_thr=below_2), rm.Thresholds(zero_dm_thr=0.0),
                rm.Thresholds(zero_dm_thr=0.0, zero_dm_floor=4.0), rm.Thresholds(zero_dm_thr=1e300)):
        c.check_flags(cs8, z, 1, thr)
    z5 = np.array([[0, 4, 8, 12, 16]], np.uint32)
    cs5 = np.tile(cs, (1, 5, 1, 1))
    assert not c.check_flags(cs5, z5, 1, rm.Thresholds(zero_dm_thr=2.0))[2].any()
    assert c.check_flags(cs5, z5, 1, rm.Thresholds(zero_dm_thr=below_2))[2].tolist() == [[1, 0, 0, 0, 1]]
    # the largest words there are
    zmax = np.array([[0xFFFFFFFF, 0, 0xFFFFFFFF, 0x80000000, 1]], np.uint32)
    c.check_flags(cs5, zmax, 1, rm.Thresholds(zero_dm_thr=1.0))


@pytest.mark.parametrize("C", [1, 2])
def test_flags_of_one_and_two_channels(gpu, case, C):
    c = case(C)
    fb = seeded_bytes(2, 40, C, seed=C)
    nb, n = rc.ONE_AND_TWO_CHANNELS
    cs, z = rm.moments(fb, 0, nb, n)
    for thr in THRESHOLDS:
        c.check_flags(cs, z, n, thr)
    cell = c.check_flags(cs, z, n, THRESHOLDS[0])[0]
    # one channel is its own median, at distance 0; of two the lower is the median and the other is out at thr = 0
    assert not cell.any() if C == 1 else cell.any() and not np.all(cell != 0)


@pytest.mark.parametrize("C,nb,n", rc.ON_CHIP_CASES)
def test_flags_on_both_sides_of_the_on_chip_lines(gpu, case, C, nb, n):
    """Up to 4096 channels and 16384 spectra the values of a bisection stay on chip (LDS, registers); beyond, every pass reads
    them from global memory.  Both lines from both sides, alone and together."""
    c = case(C)
    W = nb * n
    assert (C <= 4096, W <= 16384) in ((True, True), (False, False), (False, True))
    rng = np.random.default_rng(C + W)
    s1 = rng.integers(100 * n - 1000, 100 * n + 1000, size=(1, nb, C)).astype(np.uint64)
    s2 = s1 * s1 // n + n * rng.integers(200, 300, size=s1.shape).astype(np.uint64)  # q = n s2 - s1^2 about 250 n^2, never below 0
    assert s2.max() < 1 << 32
    cs = np.stack([s1, s2], axis=-1).astype(np.uint32)
    z = rng.integers(500_000, 530_000, size=(1, W)).astype(np.uint32)
    z[0, 4000:4004] += 100_000
    got = c.check_flags(cs, z, n, rm.Thresholds())
    assert got[2][0, 4000:4004].all() and got[2].sum() < 40
    c.check_flags(cs, z, n, rm.Thresholds(2.0, 0.0, 2.0, 0.0, 2.0, 0.0, 1))


@pytest.mark.parametrize("nb", rc.UNROLL_NR_BLOCKS)
def test_flags_across_the_unroll_of_the_bad_block_count(gpu, case, nb):
    """The beam kernel counts a channel's bad blocks eight at a time, with a tail.  Hand-made sums (helpers/rfi_cases.py;
    tests/test_rfi_forms.py holds them to their conditions on the model alone) give chosen channels exactly max_bad_blocks and
    one more bad cell, in the unrolled part only, in the tail only, and in both, for max_bad_blocks 0, 1 and 2."""
    c = case(rc.UNROLL_C)
    cs, _ = rm.moments(rc.unroll_filterbank(nb), 0, nb, rc.UNROLL_LEN)
    bad = rc.unroll_expected_bad(nb)
    for M in rc.UNROLL_MAX_BAD:
        cell, mask, _, counts = c.check_flags(cs, None, rc.UNROLL_LEN, rm.Thresholds(max_bad_blocks=M))
        assert np.array_equal((cell != 0).sum(axis=1), bad)
        assert np.array_equal(mask, (bad <= M).astype(np.uint8)) and 0 < (mask == 0).sum() < mask.size  # as made, and not trivial
        assert counts[:, 0].tolist() == bad.sum(axis=1).tolist() and counts[:, 1].tolist() == (bad > M).sum(axis=1).tolist()
        assert counts[:, :2].all() and not counts[:, 2].any()


def test_flags_where_the_top_bits_of_m_and_q_decide(gpu, case):
    """block_len 65536: m up to 255 * 65536, so that bit 23 and bit 22 each decide a median and a MAD, and q up to
    65025 * 2^30, the largest there is.  The sums are made from byte counts, so they are sums that bytes can have; that cells
    are flagged and kept on each side of 2^22 and 2^23, and that the limits lie ON a cell where they are meant to, is held on
    the model alone (tests/test_rfi_forms.py)."""
    c = case(rc.TOP_BITS_C)
    cs = rc.top_bits_sums()
    seen = [c.check_flags(cs, None, rc.TOP_BITS_LEN, thr) for thr in rc.top_bits_thresholds(cs)]
    assert all(0 < (s[0] != 0).sum() < s[0].size for s in seen[:6]) and len({s[0].tobytes() for s in seen}) == len(seen)
    assert (seen[0][0] & 1).any() and (seen[0][0] & 2).any() and 0 < (seen[2][1] == 0).sum() < 70
    z = np.random.default_rng(23).integers(0, 1 << 32, size=(1, cs.shape[1] * rc.TOP_BITS_LEN), dtype=np.uint32)  # a window past 16384
    c.check_flags(cs, z, rc.TOP_BITS_LEN, rc.TOP_THRESHOLDS)


def test_recipe_gives_the_expected_sets(gpu, case):
    B, nb, n, C = rm.RECIPE_SHAPE
    c = case(C)
    fb = rm.recipe()
    cs, z = c.moments(fb, 0, nb, n)
    exp_cs, exp_z = rm.moments(fb, 0, nb, n)
    assert np.array_equal(cs, exp_cs) and np.array_equal(z, exp_z)
    cell, mask, spectrum, counts = c.check_flags(cs, z, n, rm.Thresholds(max_bad_blocks=2))
    bad = cell != 0
    assert bad.sum() == 40 and bad[0, :, 37].all() and bad[1, :, 90].all() and np.flatnonzero(bad[0, :, 200]).tolist() == [3, 4, 5]
    assert np.flatnonzero(mask[0] == 0).tolist() == [37, 200] and np.flatnonzero(mask[1] == 0).tolist() == [90]
    assert np.argwhere(spectrum).tolist() == [[1, 500], [1, 501], [1, 502], [1, 503]]
    assert counts.tolist() == [[22, 2, 0], [18, 1, 4]]
    got, replaced = c.clean(fb, 0, nb, n, 128, cell, mask, spectrum)
    assert replaced.tolist() == [int(((mask[0] == 0).sum() * nb + 3) * n),
                                 int((mask[1] == 0).sum() * nb * n + 2 * n + 4 * C - 4)]


# -------------------------------------------------------------------------------------------------------------------- clean

@pytest.mark.parametrize("C", rc.CLEAN_CHANNELS)
def test_clean_is_the_model(gpu, case, C):
    c = case(C)
    rng = np.random.default_rng(C)
    B, nb, n, first, first_out = rc.clean_shape(C)
    W = nb * n
    fb = seeded_bytes(B, first + W + 1, C, seed=C + 1)
    cell = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3, 0x80], np.uint8), size=(B, nb, C))
    mask = rng.choice(np.array([1, 1, 1, 0x80, 0], np.uint8), size=(B, C))
    spec = rng.choice(np.array([0, 0, 0, 0, 1, 0xFF], np.uint8), size=(B, W))
    kw = dict(out_spectra=first_out + W + 2, first_out=first_out)
    copy, none = c.clean(fb, first, nb, n, 128, **kw)
    assert not none.any() and np.array_equal(copy[:, first_out:first_out + W], fb[:, first:first + W])
    counts = [c.clean(fb, first, nb, n, 77, cell=cell, **kw)[1], c.clean(fb, first, nb, n, 77, mask=mask, **kw)[1],
              c.clean(fb, first, nb, n, 77, spec=spec, **kw)[1]]
    both, all_replaced = c.clean(fb, first, nb, n, 77, cell, mask, spec, **kw)
    if C >= 64:  # no trivial expectation
        assert all(np.all(x > 0) for x in counts) and np.all(all_replaced > np.maximum.reduce(counts)) and np.all(all_replaced < W * C)
    uncounted, _ = c.clean(fb, first, nb, n, 77, cell, mask, spec, count=False, **kw)
    assert np.array_equal(uncounted, both)
    # in place: the rows outside the window keep their bytes
    same, _ = c.clean(fb, first, nb, n, 77, cell, mask, spec, in_place=True)
    assert np.array_equal(same[:, first:first + W], both[:, first_out:first_out + W])
    assert np.array_equal(same[:, :first], fb[:, :first]) and np.array_equal(same[:, first + W:], fb[:, first + W:])
    # blocks of one spectrum, and one block of all
    c.clean(fb, first, W, 1, 0, rng.choice(np.array([0, 0, 1], np.uint8), size=(B, W, C)), mask, spec, **kw)
    c.clean(fb, first, 1, W, 255, cell[:, :1], mask, spec, **kw)


def flag_tensors(rng, B, nb, W, C):
    cell = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3, 0x80], np.uint8), size=(B, nb, C))
    mask = rng.choice(np.array([1, 1, 1, 0x80, 0], np.uint8), size=(B, C))
    spec = rng.choice(np.array([0, 0, 0, 0, 1, 0xFF], np.uint8), size=(B, W))
    return cell, mask, spec


@pytest.mark.parametrize("C", rc.FORM_CHANNELS)
def test_clean_of_every_form_is_the_model(gpu, case, C):
    """The forms test_clean_is_the_model leaves out, as the moments have them: out of place and in place, with and without
    the flag tensors."""
    c = case(C)
    rng = np.random.default_rng(C)
    for i, (n, nb, B, first) in enumerate(FORM_CASES[C]):
        W, first_out = nb * n, (0, 2)[i % 2]
        fb = seeded_bytes(B, first + W + 1, C, seed=C + n)
        cell, mask, spec = flag_tensors(rng, B, nb, W, C)
        kw = dict(out_spectra=first_out + W + 1, first_out=first_out)
        copy, none = c.clean(fb, first, nb, n, 128, **kw)
        assert not none.any() and np.array_equal(copy[:, first_out:first_out + W], fb[:, first:first + W])
        both, replaced = c.clean(fb, first, nb, n, 77, cell, mask, spec, **kw)
        assert np.all(replaced <= W * C) and (C * W < 64 or np.all(replaced > 0))
        c.clean(fb, first, nb, n, 77, cell=cell, count=False, **kw)
        c.clean(fb, first, nb, n, 77, mask=mask, spec=spec, **kw)
        same, _ = c.clean(fb, first, nb, n, 77, cell, mask, spec, in_place=True)
        assert np.array_equal(same[:, first:first + W], both[:, first_out:first_out + W])
        assert np.array_equal(same[:, :first], fb[:, :first]) and np.array_equal(same[:, first + W:], fb[:, first + W:])


@pytest.mark.parametrize("C,offset", [(C, o) for C, offsets in rc.OFFSET_CASES.items() for o in offsets])
def test_clean_with_flag_tensors_at_any_byte_offset(gpu, case, C, offset):
    """include/dcs_rfi.h gives the flag tensors no alignment rule: where one is not aligned to the unit of the row accesses
    the kernel loads it in single bytes.  Every flag tensor lies `offset` bytes into its allocation, between bytes that would
    replace what the tensor's own first and last entries keep; no byte of the filterbank equals the fill, so every byte
    replaced shows.  (A broken byte path fails this; a kernel without one might not, where the hardware serves the
    unaligned vector load.)"""
    B, nb, n, first = rc.OFFSET_SHAPE
    W = nb * n
    c = case(C)
    rng = np.random.default_rng(100 * C + offset)
    fb = seeded_bytes(B, first + W + 1, C, seed=C + offset)
    fb[fb == 77] = 78
    cell, mask, spec = flag_tensors(rng, B, nb, W, C)
    cell[..., 0] = cell[..., -1] = 0     # kept by their own flags, replaced by the bytes around them
    mask[:, 0] = mask[:, -1] = 1
    spec[:, 0] = spec[:, -1] = 0
    aligned, replaced = c.clean(fb, first, nb, n, 77, cell, mask, spec)
    assert np.all(replaced > 0) and np.all(replaced < W * C)
    for kw in (dict(cell=cell), dict(mask=mask), dict(spec=spec), dict(cell=cell, mask=mask, spec=spec)):
        got, _ = c.clean(fb, first, nb, n, 77, offset=offset, **kw)
        if len(kw) == 3:
            assert np.array_equal(got, aligned)
        c.clean(fb, first, nb, n, 77, offset=offset, in_place=True, **kw)


# ------------------------------------------------------------------------------------------------------------------- chains

def test_filterbank_q8_into_rfi_into_dedisperse(gpu, case):
    """Spectra through filterbank_q8, the three RFI calls and dedisperse_q8: per beam with its row of the channel masks at
    nr_beams = 1, and all beams at once on the cleaned filterbank with no mask.  Both planes are the model's."""
    from dc_sand_amd.generator import (dm_time_bytes, filterbank_bytes, rfi_cell_flags_bytes, rfi_cell_sums_bytes,
                                       rfi_channel_mask_bytes, rfi_counts_bytes, rfi_spectrum_flags_bytes, rfi_zero_dm_bytes)

    C, B, nr_dm, n = 64, 2, 7, 32
    table = dm_delays(C, *BAND_DESCENDING_64, DMS_40[:nr_dm])
    max_delay = int(table.max())
    T = 160
    nb = (T + max_delay + n - 1) // n
    rows = nb * n
    rng = np.random.default_rng(12)
    m = np.exp2(rng.uniform(-4.0, 4.0, size=(C, B))).astype(np.float32)
    x = (m[None].astype(np.float64) * (1.0 + 0.25 * rng.standard_normal((rows, C, B))))
    x[:, 20, 0] = m[20, 0]                                  # a dead channel in beam 0
    x[:, 41, 1] += 0.5 * m[41, 1] * rng.standard_normal(rows)  # a loud one in beam 1
    x[100:103, :, 1] += 0.4 * m[None, :, 1]                 # a burst in beam 1
    x = x.astype(np.float32)
    sc = np.stack([m, (16.0 / (0.25 * m.astype(np.float64))).astype(np.float32)], axis=-1)
    fb, _ = filterbank(x, sc, 128.0)
    thr = rm.Thresholds(max_bad_blocks=1)
    cs, z = rm.moments(fb, 0, nb, n)
    cell, mask, spec, counts = rm.flags(cs, z, n, thr)
    cleaned, _ = rm.clean(fb, 0, nb, n, 128, cell, mask, spec)
    assert mask[0, 20] == 0 and mask[1, 41] == 0 and spec[1, 100:103].all() and 2 <= (mask == 0).sum() <= 6
    c = case(C)
    g = c.g
    fbytes, pbytes = filterbank_bytes(c.bp, B, rows), dm_time_bytes(B, nr_dm, T)
    d_x, d_sc, d_fb, d_clean = c.upload(x), c.upload(sc), c.alloc(fbytes), c.out(fbytes, PREFILL)
    d_cs, d_z = c.out(rfi_cell_sums_bytes(c.bp, B, nb)), c.out(rfi_zero_dm_bytes(B, rows))
    d_cf, d_cm = c.out(rfi_cell_flags_bytes(c.bp, B, nb)), c.out(rfi_channel_mask_bytes(c.bp, B))
    d_sf, d_cnt = c.out(rfi_spectrum_flags_bytes(B, rows)), c.out(rfi_counts_bytes(B))
    d_delays, d_masked, d_plane = c.upload(table), c.out(pbytes, PREFILL), c.out(pbytes, PREFILL)
    g.filterbank_q8(d_x, x.nbytes, rows, B, d_sc, 128.0, d_fb, fbytes, rows)
    g.rfi_moments(d_fb, fbytes, rows, 0, nb, n, B, d_cs, cs.nbytes, d_z, z.nbytes)
    g.rfi_flags(d_cs, cs.nbytes, nb, n, B, d_cf, cell.nbytes, d_cm, mask.nbytes, d_cnt, counts.nbytes, thresholds=gen_thresholds(thr),
                d_zero_dm=d_z, zero_dm_bytes=z.nbytes, d_spectrum_flags=d_sf, spectrum_flags_bytes=spec.nbytes)
    g.rfi_clean_q8(d_fb, fbytes, rows, 0, nb, n, B, 128, d_clean, fbytes, rows, d_cell_flags=d_cf, d_channel_mask=d_cm,
                   d_spectrum_flags=d_sf)
    for b in range(B):  # row b of the masks is the mask of a dedispersion of beam b alone
        g.dedisperse_q8(int(d_fb) + b * rows * C, rows * C, rows, 0, T, 1, d_delays, nr_dm, max_delay,
                        int(d_masked) + b * nr_dm * T * 4, nr_dm * T * 4, T, d_channel_mask=int(d_cm) + b * C)
    g.dedisperse_q8(d_clean, fbytes, rows, 0, T, B, d_delays, nr_dm, max_delay, d_plane, pbytes, T)
    gpu.synchronize()
    assert np.array_equal(c.read(d_cf, cell.nbytes, np.uint8, cell.shape), cell)
    assert np.array_equal(c.read(d_cm, mask.nbytes, np.uint8, mask.shape), mask)
    assert np.array_equal(c.read(d_sf, spec.nbytes, np.uint8, spec.shape), spec)
    assert np.array_equal(c.read(d_cnt, counts.nbytes, np.uint32, counts.shape), counts)
    assert np.array_equal(c.read(d_clean, fbytes, np.uint8, fb.shape), cleaned)
    exp_masked = np.concatenate([dedisperse(fb[b:b + 1], table, 0, T, max_delay, mask[b]) for b in range(B)])
    got = c.read(d_masked, pbytes, np.uint32, (B, nr_dm, T))
    assert np.array_equal(got, exp_masked), np.argwhere(got != exp_masked)[:3]
    exp_plane = dedisperse(cleaned, table, 0, T, max_delay)
    got = c.read(d_plane, pbytes, np.uint32, (B, nr_dm, T))
    assert np.array_equal(got, exp_plane), np.argwhere(got != exp_plane)[:3]
    assert not np.array_equal(exp_plane, exp_masked) and not np.array_equal(exp_plane, dedisperse(fb, table, 0, T, max_delay))


# ------------------------------------------------------------------------------------------------------------------ capture

def test_three_calls_captured_and_replayed_with_new_bytes(gpu, case):
    """All three calls as first calls on a fresh context, captured in one graph; replayed after the filterbank bytes were
    changed on the device: every output follows the new bytes, the zero-DM series included, which a memset node zeroes."""
    C, B, nb, n, first = 100, 2, 5, 24, 3
    W, rows = nb * n, 3 + nb * n
    thr = rm.Thresholds(4.0, 0.0, 4.0, 0.0, 4.0, 0.0, 1)
    c = case(C)
    g = c.g
    fbytes = B * rows * C
    d_fb = c.alloc(fbytes)
    d_cs, d_z, d_cf, d_cm = c.out(B * nb * C * 8), c.out(B * W * 4), c.out(B * nb * C), c.out(B * C)
    d_sf, d_cnt, d_out, d_rep = c.out(B * W), c.out(B * 12), c.out(B * W * C, PREFILL), c.out(B * 8, 0)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        g.rfi_moments(d_fb, fbytes, rows, first, nb, n, B, d_cs, B * nb * C * 8, d_z, B * W * 4, stream=s.handle)
        g.rfi_flags(d_cs, B * nb * C * 8, nb, n, B, d_cf, B * nb * C, d_cm, B * C, d_cnt, B * 12, thresholds=gen_thresholds(thr),
                    d_zero_dm=d_z, zero_dm_bytes=B * W * 4, d_spectrum_flags=d_sf, spectrum_flags_bytes=B * W, stream=s.handle)
        g.rfi_clean_q8(d_fb, fbytes, rows, first, nb, n, B, 128, d_out, B * W * C, W, d_cell_flags=d_cf, d_channel_mask=d_cm,
                       d_spectrum_flags=d_sf, d_replaced=d_rep, stream=s.handle)
    seen = []
    for i in range(3):
        rng = np.random.default_rng(80 + i)
        fb = np.clip(np.rint(rng.normal(128, 16, (B, rows, C))), 0, 255).astype(np.uint8)
        fb[i % B, :, 10 + i] = 128
        fb[(i + 1) % B, first + 7 * (i + 1)] = 160
        gpu.memcpy_htod(d_fb, fb, stream=s.handle, sync=False)
        gpu.memset(d_rep, 0, B * 8, stream=s.handle)
        graph.launch(s)
        s.synchronize()
        cs, z = rm.moments(fb, first, nb, n)
        cell, mask, spec, counts = rm.flags(cs, z, n, thr)
        out, replaced = rm.clean(fb, first, nb, n, 128, cell, mask, spec)
        assert np.array_equal(c.read(d_cs, cs.nbytes, np.uint32, cs.shape), cs), i
        assert np.array_equal(c.read(d_z, z.nbytes, np.uint32, z.shape), z), i
        assert np.array_equal(c.read(d_cf, cell.nbytes, np.uint8, cell.shape), cell), i
        assert np.array_equal(c.read(d_cm, mask.nbytes, np.uint8, mask.shape), mask), i
        assert np.array_equal(c.read(d_sf, spec.nbytes, np.uint8, spec.shape), spec), i
        assert np.array_equal(c.read(d_cnt, counts.nbytes, np.uint32, counts.shape), counts), i
        assert np.array_equal(c.read(d_out, out.nbytes, np.uint8, out.shape), out), i
        assert np.array_equal(c.read(d_rep, B * 8, np.uint64, (B,)), replaced), i
        assert mask[i % B, 10 + i] == 0 and spec[(i + 1) % B, 7 * (i + 1)] == 1
        seen.append(mask)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    graph.close()


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_short_buffers_are_refused_and_nothing_is_enqueued(gpu, case):
    """The refusals that need the context's C: they come after the version check, with DCS_ERR_INVALID_ARGUMENT."""
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    C, B, nb, n = 64, 2, 3, 8
    W = nb * n
    c = case(C)
    g = c.g
    fbytes, sbytes, cfb, cmb = B * W * C, B * nb * C * 8, B * nb * C, B * C
    d_fb = c.upload(seeded_bytes(B, W, C, seed=5))
    d_cs, d_cf, d_cm, d_cnt, d_out = c.out(sbytes), c.out(cfb), c.out(cmb), c.out(B * 12), c.out(fbytes)
    calls = [
        lambda: g.rfi_moments(d_fb, fbytes - 1, W, 0, nb, n, B, d_cs, sbytes),
        lambda: g.rfi_moments(d_fb, fbytes, W, 0, nb, n, B, d_cs, sbytes - 1),
        lambda: g.rfi_moments(d_fb, fbytes, W, 0, nb, n, B + 1, d_cs, sbytes),
        lambda: g.rfi_flags(d_cs, sbytes - 1, nb, n, B, d_cf, cfb, d_cm, cmb, d_cnt, B * 12),
        lambda: g.rfi_flags(d_cs, sbytes, nb, n, B, d_cf, cfb - 1, d_cm, cmb, d_cnt, B * 12),
        lambda: g.rfi_flags(d_cs, sbytes, nb, n, B, d_cf, cfb, d_cm, cmb - 1, d_cnt, B * 12),
        lambda: g.rfi_flags(d_cs, sbytes, nb, n, B, d_cf, cfb, d_cm, cmb, d_cnt, B * 12 - 1),
        lambda: g.rfi_clean_q8(d_fb, fbytes - 1, W, 0, nb, n, B, 128, d_out, fbytes, W),
        lambda: g.rfi_clean_q8(d_fb, fbytes, W, 0, nb, n, B, 128, d_out, fbytes - 1, W),
        lambda: g.rfi_clean_q8(d_fb, fbytes, W, 1, nb, n, B, 128, d_out, fbytes, W),
        lambda: g.rfi_clean_q8(d_fb, fbytes, W, 0, nb, n, B, 128, d_out, fbytes, W, first_out=1),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    with pytest.raises(ValueError):
        g.rfi_clean_q8(d_fb, fbytes, W, 0, nb, n, B, 256, d_out, fbytes, W)
    gpu.synchronize()
    for d in (d_cs, d_cf, d_cm, d_cnt, d_out):
        assert np.all(c.read(d) == 0xA5)


# ------------------------------------------------------------------------------------------------------------------ example

def test_example_runs_and_verifies_itself(gpu):
    out = run_example("rfi_excision.py")
    assert "without cleaning the strongest peak is the burst at DM 0: True" in out
    assert "with cleaning it is the pulse: True" in out
