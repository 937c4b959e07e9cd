"""The pulsar folder on the GPU (include/dcs_fold.h).  No tolerance anywhere: profiles, hits and the
scrunched plane are integers and are compared with the numpy model (helpers/fold_model.py, anchored on the CPU by
tests/test_fold_model.py) bit for bit.  Every buffer is exactly sized: the filterbank's window ends where its allocation ends;
every output is prefilled and has a 0xA5 canary behind it, which must stay untouched, and the sub-integrations outside the
addressed ones must stay as they were.  The case table is helpers/fold_cases.py; tests/test_fold_forms.py has its census."""
from functools import partial

import numpy as np
import pytest

from helpers import fold_cases as fc
from helpers import fold_model as fm
from helpers import hip_graph
from helpers.dedisperse_model import dm_delays
from helpers.device_buffers import Context, closed_after

pytestmark = pytest.mark.gpu

PREFILL = 0x3C
PRE32, PRE64 = 0x3C3C3C3C, 0x3C3C3C3C3C3C3C3C


class FCase(Context):
    """One context of C channels and the device buffers of its calls, exactly sized, outputs prefilled with a canary behind."""

    def fold(self, fb, models, first, L, nbin, bpm=1, delays=None, max_delay=0, mask=None, hits=True, first_subint=0, extra=1,
             d_delays=None):
        """dcs_bf_fold_q8 into prefilled outputs of first_subint + S + extra sub-integrations: (profiles, hits or None) as the
        device made them, compared with the model, the untouched sub-integrations included."""
        from dc_sand_amd.generator import fold_hits_bytes, fold_profiles_bytes

        B, in_spectra, C = fb.shape
        P, S = models.shape
        OS = first_subint + S + extra
        pbytes, hbytes = fold_profiles_bytes(self.bp, B, OS, nbin), fold_hits_bytes(P, OS, nbin)
        assert (pbytes, hbytes) == (B * OS * C * nbin * 4, P * OS * nbin * 4) and C == self.C
        d_fb, d_m = self.upload(fb), self.upload(models)
        if d_delays is None and delays is not None:
            d_delays = self.upload(np.ascontiguousarray(delays, dtype=np.int32))
        d_mask = None if mask is None else self.upload(mask)
        d_p, d_h = self.out(pbytes, PREFILL), self.out(hbytes, PREFILL) if hits else None
        self.g.fold_q8(d_fb, fb.nbytes, in_spectra, first, L, S, B, d_m, models.nbytes, nbin, d_p, pbytes, OS, first_subint=first_subint,
                       beams_per_model=bpm, d_delays=d_delays, delays_bytes=0 if d_delays is None else P * C * 4, max_delay=max_delay,
                       d_channel_mask=d_mask, d_hits=d_h, hits_bytes=hbytes if hits else 0)
        self.gpu.synchronize()
        exp_p, exp_h = fm.fold(fb, models, first, L, nbin, bpm, delays, max_delay, mask, profiles=np.full((B, OS, C, nbin), PRE32, np.uint32),
                               hits=np.full((P, OS, nbin), PRE32, np.uint32), first_subint=first_subint)
        got_p = self.read(d_p, pbytes, np.uint32, (B, OS, C, nbin))
        assert np.array_equal(got_p, exp_p), np.argwhere(got_p != exp_p)[:4]
        got_h = None
        if hits:
            got_h = self.read(d_h, hbytes, np.uint32, (P, OS, nbin))
            assert np.array_equal(got_h, exp_h), np.argwhere(got_h != exp_h)[:4]
        return got_p, got_h, d_p


@pytest.fixture
def case(gpu):
    yield from closed_after(partial(FCase, gpu))


def seeded_bytes(B, rows, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, rows, C), dtype=np.uint8)


CASES = fc.cases()


@pytest.mark.parametrize("C,group", [(C, g) for C in fc.CHANNELS for g in range(fc.GROUPS)])
def test_fold_is_the_model(gpu, case, C, group):
    """Every nbin of the table at this C (a third of them per test): the models of every kind, delay tables from
    dcs_bf_dm_delays on the device, hand tables with entries that fold to zero, masks, no table, with and without hits."""
    c = case(C)
    for i, r in enumerate(CASES[C][group::fc.GROUPS]):
        seed = 1000 * C + r.nbin
        P = r.B // r.bpm
        models = fc.models_of(r, seed)
        mask = fc.mask_of(r, seed + 1)
        delays = d_delays = None
        max_delay = 0
        if r.delays == "dm":  # made on the device, and held to the model of the delays
            band, dms = fc.band_of(C), fc.dms_of(P)
            delays = dm_delays(C, *band, dms)
            max_delay = int(delays.max()) - (1 if i % 2 and delays.max() > 0 else 0)  # odd cases: the largest delays fold to zero
            d_delays = c.out(P * C * 4)
            c.g.dm_delays(*band, c.upload(dms), P, d_delays, P * C * 4)
            gpu.synchronize()
            assert np.array_equal(c.read(d_delays, P * C * 4, np.int32, (P, C)), delays)
        elif r.delays == "hand":
            max_delay = fc.HAND_MAX_DELAY
            delays = fc.hand_table(r, max_delay, seed + 2)
        fb = seeded_bytes(r.B, r.first + r.S * r.L + max_delay, C, seed + 3)  # the window ends where the allocation ends
        got_p, _, _ = c.fold(fb, models, r.first, r.L, r.nbin, r.bpm, delays, max_delay, mask, hits=r.hits, first_subint=r.first_subint,
                             d_delays=d_delays)
        # every byte of a column that takes part is in one of its bins, and a column that does not folds to zero
        on, d = fm.columns_on(C, None if delays is None else delays[0], max_delay, mask)
        rows = r.first + np.arange(r.L)[:, None] + d[None, :]
        sums = np.where(on, fb[0][rows, np.arange(C)[None, :]].astype(np.int64).sum(axis=0), 0)
        assert np.array_equal(got_p[0, r.first_subint].astype(np.int64).sum(axis=-1), sums)


def test_a_cut_subintegration_accumulates_to_the_bits_of_one_call(gpu, case):
    from dc_sand_amd.fold import advance

    C, B, L, nbin = 100, 3, 513, 100
    c = case(C)
    fb = seeded_bytes(B, L + 2, C, 7)
    m0 = np.array([[fm.model(fc.TURN - 12345, fc.TURN // 37 + 5, -(1 << 41) - 7)] for _ in range(B)], dtype=fm.model_dtype)
    whole_p, whole_h, _ = c.fold(fb, m0, 2, L, nbin, extra=0)
    pbytes, hbytes = B * C * nbin * 4, B * nbin * 4
    for cut in (1, 256, 512):
        m1 = np.array([[advance(m0[p, 0], cut)] for p in range(B)], dtype=fm.model_dtype)
        d_fb, d_p, d_h = c.upload(fb), c.out(pbytes, PREFILL), c.out(hbytes, PREFILL)
        c.g.fold_q8(d_fb, fb.nbytes, L + 2, 2, cut, 1, B, c.upload(m0), m0.nbytes, nbin, d_p, pbytes, 1, d_hits=d_h, hits_bytes=hbytes)
        c.g.fold_q8(d_fb, fb.nbytes, L + 2, 2 + cut, L - cut, 1, B, c.upload(m1), m1.nbytes, nbin, d_p, pbytes, 1, d_hits=d_h,
                    hits_bytes=hbytes, accumulate=True)
        gpu.synchronize()
        assert np.array_equal(c.read(d_p, pbytes, np.uint32, whole_p.shape), whole_p), cut
        assert np.array_equal(c.read(d_h, hbytes, np.uint32, whole_h.shape), whole_h), cut
    # accumulate adds modulo 2^32 onto what is there
    d_fb, d_p = c.upload(fb), c.out(pbytes, 0xFF)
    c.g.fold_q8(d_fb, fb.nbytes, L + 2, 2, L, 1, B, c.upload(m0), m0.nbytes, nbin, d_p, pbytes, 1, accumulate=True)
    gpu.synchronize()
    assert np.array_equal(c.read(d_p, pbytes, np.uint32, whole_p.shape), whole_p + np.uint32(0xFFFFFFFF))


def test_full_scale_at_the_longest_subintegration(gpu, case):
    """Bytes 255, subint_len 2^24, one channel and one bin: the word is 255 * 2^24, the largest there is, and the hits 2^24."""
    L = 1 << 24
    c = case(1)
    d_fb, d_m = c.upload(np.full((1, L, 1), 255, np.uint8)), c.upload(np.array([[fm.model(123, fc.TURN // 3 + 1, 99)]], dtype=fm.model_dtype))
    d_p, d_h = c.out(4, PREFILL), c.out(4, PREFILL)
    c.g.fold_q8(d_fb, L, L, 0, L, 1, 1, d_m, 24, 1, d_p, 4, 1, d_hits=d_h, hits_bytes=4)
    gpu.synchronize()
    assert c.read(d_p, 4, np.uint32).tolist() == [255 << 24] and c.read(d_h, 4, np.uint32).tolist() == [L]


def test_nothing_to_do_writes_nothing(gpu, case):
    c = case(64)
    d_fb, d_m, d_p, d_h, d_s = c.upload(seeded_bytes(1, 8, 64, 1)), c.upload(np.zeros(24, np.uint8)), c.out(64), c.out(64), c.out(64)
    c.g.fold_q8(d_fb, 512, 8, 8, 4, 0, 1, d_m, 0, 16, d_p, 0, 0, d_hits=d_h, hits_bytes=0)
    c.g.fold_scrunch(d_p, 0, 1, 0, 0, 0, 16, d_s, 0)
    gpu.synchronize()
    assert np.all(c.read(d_p) == 0xA5) and np.all(c.read(d_h) == 0xA5) and np.all(c.read(d_s) == 0xA5)


@pytest.mark.parametrize("C,nbin", [(1, 1), (3, 3), (64, 100), (100, 64), (317, 257), (64, 1024)])
def test_scrunch_is_the_model(gpu, case, C, nbin):
    """Seeded profile words near 2^32, so that the sums pass it; placement, and accumulate onto a prefilled plane."""
    from dc_sand_amd.generator import fold_profiles_bytes, fold_scrunched_bytes

    B, OS, first, S = 2, 4, 1, 2
    c = case(C)
    prof = np.random.default_rng(C + nbin).integers((1 << 32) - (1 << 20), 1 << 32, size=(B, OS, C, nbin), dtype=np.uint64).astype(np.uint32)
    pbytes, sbytes = fold_profiles_bytes(c.bp, B, OS, nbin), fold_scrunched_bytes(B, OS, nbin)
    assert (pbytes, sbytes) == (prof.nbytes, B * OS * nbin * 8)
    d_p, d_s = c.upload(prof), c.out(sbytes, PREFILL)
    pre = np.full((B, OS, nbin), PRE64, np.uint64)
    c.g.fold_scrunch(d_p, pbytes, B, OS, first, S, nbin, d_s, sbytes)
    gpu.synchronize()
    exp = fm.scrunch(prof, first, S, out=pre)
    got = c.read(d_s, sbytes, np.uint64, (B, OS, nbin))
    assert np.array_equal(got, exp) and (C < 2 or exp[:, first:first + S].min() > 1 << 32)
    c.g.fold_scrunch(d_p, pbytes, B, OS, 0, OS, nbin, d_s, sbytes, accumulate=True)
    gpu.synchronize()
    assert np.array_equal(c.read(d_s, sbytes, np.uint64, (B, OS, nbin)), fm.scrunch(prof, 0, OS, out=exp, accumulate=True))


def test_both_calls_captured_and_replayed_with_new_tables(gpu, case):
    """Both calls as first calls on a fresh context, captured in one graph and replayed three times with the models, the delay
    table and the filterbank rewritten between the replays: each replay is the model of the contents at that replay."""
    C, B, bpm, L, S, nbin, max_delay, first = 100, 8, 4, 200, 2, 65, 9, 1
    P, rows = B // bpm, first + S * L + max_delay
    c = case(C)
    g = c.g
    pbytes, hbytes, sbytes = B * S * C * nbin * 4, P * S * nbin * 4, B * S * nbin * 8
    d_fb, d_m, d_d = c.alloc(B * rows * C), c.alloc(P * S * 24), c.alloc(P * C * 4)
    d_p, d_h, d_s = c.out(pbytes, PREFILL), c.out(hbytes, PREFILL), c.out(sbytes, PREFILL)
    s = gpu.Stream()
    with hip_graph.capture(s) as graph:
        g.fold_q8(d_fb, B * rows * C, rows, first, L, S, B, d_m, P * S * 24, nbin, d_p, pbytes, S, beams_per_model=bpm, d_delays=d_d,
                  delays_bytes=P * C * 4, max_delay=max_delay, d_hits=d_h, hits_bytes=hbytes, stream=s.handle)
        g.fold_scrunch(d_p, pbytes, B, S, 0, S, nbin, d_s, sbytes, stream=s.handle)
    seen = []
    for i in range(3):
        rng = np.random.default_rng(40 + i)
        fb = seeded_bytes(B, rows, C, 50 + i)
        models = np.array([fm.model(int(rng.integers(0, 1 << 62)) * 4 + i, fc.TURN // (20 + 7 * i) + i, (i - 1) * (1 << 42)) for _ in range(P * S)],
                          dtype=fm.model_dtype).reshape(P, S)
        delays = rng.integers(-1, max_delay + 2, size=(P, C)).astype(np.int32)
        for d, h in ((d_fb, fb), (d_m, models), (d_d, delays)):
            gpu.memcpy_htod(d, np.ascontiguousarray(h), stream=s.handle, sync=False)
        graph.launch(s)
        s.synchronize()
        exp_p, exp_h = fm.fold(fb, models, first, L, nbin, bpm, delays, max_delay)
        assert np.array_equal(c.read(d_p, pbytes, np.uint32, exp_p.shape), exp_p), i
        assert np.array_equal(c.read(d_h, hbytes, np.uint32, exp_h.shape), exp_h), i
        assert np.array_equal(c.read(d_s, sbytes, np.uint64, (B, S, nbin)), fm.scrunch(exp_p, 0, S)), i
        seen.append(exp_p)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    graph.close()


def test_short_buffers_are_refused_and_nothing_is_enqueued(gpu, case):
    """The refusals that need the context's C: they come after the version check, with DCS_ERR_INVALID_ARGUMENT."""
    from dc_sand_amd._lib import DCS_ERR_INVALID_ARGUMENT, DcsError

    C, B, L, S, nbin = 64, 2, 8, 3, 16
    c = case(C)
    g = c.g
    fbytes, mbytes, pbytes, hbytes, sbytes = B * S * L * C, B * S * 24, B * S * C * nbin * 4, B * S * nbin * 4, B * S * nbin * 8
    d_fb, d_m, d_d = c.upload(seeded_bytes(B, S * L, C, 5)), c.upload(np.zeros(mbytes, np.uint8)), c.upload(np.zeros((B, C), np.int32))
    d_p, d_h, d_s = c.out(pbytes), c.out(hbytes), c.out(sbytes)

    def fold(fb=fbytes, mb=mbytes, pb=pbytes, hb=hbytes, db=B * C * 4, beams=B):
        g.fold_q8(d_fb, fb, S * L, 0, L, S, beams, d_m, mb, nbin, d_p, pb, S, d_delays=d_d, delays_bytes=db, d_hits=d_h, hits_bytes=hb)

    calls = [lambda: fold(fb=fbytes - 1), lambda: fold(mb=mbytes - 1), lambda: fold(pb=pbytes - 1), lambda: fold(hb=hbytes - 1),
             lambda: fold(db=B * C * 4 - 1), lambda: fold(beams=B + 1),
             lambda: g.fold_scrunch(d_p, pbytes - 1, B, S, 0, S, nbin, d_s, sbytes),
             lambda: g.fold_scrunch(d_p, pbytes, B, S, 0, S, nbin, d_s, sbytes - 1)]
    for i, call in enumerate(calls):
        with pytest.raises(DcsError) as e:
            call()
        assert e.value.status == DCS_ERR_INVALID_ARGUMENT, i
    gpu.synchronize()
    for d in (d_p, d_h, d_s):
        assert np.all(c.read(d) == 0xA5)


def test_example_runs_and_verifies_itself(gpu):
    from helpers.examples import run_example

    out = run_example("folded_pulsar.py")
    assert "the peak bin of every sub-integration is the predicted one: True" in out
    assert "every off-pulse bin is flat to the noise model: True" in out
