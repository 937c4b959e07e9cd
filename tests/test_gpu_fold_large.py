"""The pulsar folder held to its 64-bit offsets (include/dcs_fold.h): a filterbank and profiles past 2^32 bytes, which never
exist on the host (helpers/large_tensor.py: the filling, the pattern whose period does not divide 2^32, the row reads;
helpers/fold_large.py: the shapes).  A byte offset worked out in 32 bits wraps inside the same allocation, 4 GiB lower: nothing
faults and no canary is touched, so the tensors hold contents in which the rows 4 GiB apart differ.  Every other test of the
folder passes with 32-bit offsets; these do not (tests/test_fold_large_plan.py)."""
import numpy as np
import pytest

from helpers import fold_large as fl
from helpers import fold_model as fm
from helpers import large_tensor as lt
from helpers.device_buffers import Context

pytestmark = pytest.mark.gpu


@pytest.fixture
def case(gpu):
    c = Context(gpu, fl.C)
    yield c
    c.close()


def test_filterbank_past_4_gib_on_both_sides_of_the_line(gpu, case):
    from dc_sand_amd.generator import fold_hits_bytes, fold_profiles_bytes, fold_scrunched_bytes

    g = case.g
    pat = fl.pattern(71)
    d_fb = case.out(fl.NBYTES)
    lt.fill(gpu, d_fb, fl.NBYTES, pat)
    S, nbin = fl.NR_SUBINTS, fl.NBIN
    models, delays = fl.models(81, S, nbin), fl.delays(82)
    d_m, d_d = case.upload(models), case.upload(delays)
    pbytes, hbytes, sbytes = fold_profiles_bytes(case.bp, fl.B, S, nbin), fold_hits_bytes(fl.B, S, nbin), fold_scrunched_bytes(fl.B, S, nbin)
    d_p, d_h, d_s = case.out(pbytes), case.out(hbytes), case.out(sbytes)
    seen = []
    # the window at the line, which ends where the tensor ends, and the window that holds the rows 4 GiB below its upper half
    for first in (fl.FIRST_AT_LINE, fl.FIRST_BELOW):
        for d in (d_p, d_h, d_s):
            case.refill(d)
        g.fold_q8(d_fb, fl.NBYTES, fl.IN_SPECTRA, first, fl.SUBINT_LEN, S, fl.B, d_m, models.nbytes, nbin, d_p, pbytes, S, d_delays=d_d,
                  delays_bytes=delays.nbytes, max_delay=fl.MAX_DELAY, d_hits=d_h, hits_bytes=hbytes)
        g.fold_scrunch(d_p, pbytes, fl.B, S, 0, S, nbin, d_s, sbytes)
        gpu.synchronize()
        exp_p, exp_h = fl.expected_fold(pat, first)
        got = case.read(d_p, pbytes, np.uint32, exp_p.shape)
        assert np.array_equal(got, exp_p), (first, np.argwhere(got != exp_p)[:3])
        assert np.array_equal(case.read(d_h, hbytes, np.uint32, exp_h.shape), exp_h), first
        assert np.array_equal(case.read(d_s, sbytes, np.uint64, (fl.B, S, nbin)), fm.scrunch(exp_p, 0, S)), first
        seen.append(got)
    # what a read 4 GiB low would have folded at the line is not what was found there (tests/test_fold_large_plan.py: it differs)
    assert not np.array_equal(seen[0][1, 3], fl.expected_fold(pat, fl.FIRST_AT_LINE, wrapped=True)[0][1, 3])
    # the filterbank is read only: a sample of its rows on both sides of the line, and its canary
    rows = np.array([0, 1, fl.IN_SPECTRA - 1, fl.IN_SPECTRA, fl.IN_SPECTRA + fl.LINE_ROW - 1, fl.IN_SPECTRA + fl.LINE_ROW,
                     2 * fl.IN_SPECTRA - 1], dtype=np.int64)
    assert np.array_equal(lt.read_rows(gpu, d_fb, fl.C, rows), lt.rows_of(pat, rows))
    case.guard_untouched(d_fb)


def test_profiles_past_4_gib_on_both_sides_of_the_line(gpu, case):
    from dc_sand_amd.generator import fold_profiles_bytes, fold_scrunched_bytes

    g = case.g
    S, L, nbin, OS = fl.SHORT_SUBINTS, fl.SHORT_LEN, fl.BIG_NBIN, fl.OUT_SUBINTS
    assert fold_profiles_bytes(case.bp, fl.B, OS, nbin) == fl.PROFILES_BYTES
    d_p = case.out(fl.PROFILES_BYTES, fl.PREFILL)
    sbytes = fold_scrunched_bytes(fl.B, OS, nbin)
    d_s = case.out(sbytes, fl.PREFILL)
    expected = {}
    for seed, first_subint in ((91, fl.FIRST_SUB_BELOW), (93, fl.FIRST_SUB_AT_LINE)):
        fb, models = fl.short_filterbank(seed), fl.models(seed + 1, S, nbin)
        g.fold_q8(case.upload(fb), fb.nbytes, S * L, 0, L, S, fl.B, case.upload(models), models.nbytes, nbin, d_p, fl.PROFILES_BYTES, OS,
                  first_subint=first_subint)
        g.fold_scrunch(d_p, fl.PROFILES_BYTES, fl.B, OS, first_subint, S, nbin, d_s, sbytes)
        gpu.synchronize()
        expected[first_subint] = fl.expected_short(seed)
        # after either call: every sub-integration addressed so far holds its own call's profiles -- beam 0's first ones are
        # where a store of the second call 4 GiB low would have landed -- and their neighbours hold the prefill
        for at, exp in expected.items():
            for b in range(fl.B):
                subs = b * OS + at + np.arange(S, dtype=np.int64)
                got = lt.read_rows(gpu, d_p, fl.SUBINT_BYTES, subs).view(np.uint32).reshape(S, fl.C, nbin)
                assert np.array_equal(got, exp[b]), (first_subint, at, b, np.argwhere(got != exp[b])[:3])
                got = lt.read_rows(gpu, d_s, nbin * 8, subs).view(np.uint64)
                assert np.array_equal(got, exp[b].astype(np.uint64).sum(axis=1)), (first_subint, at, b)
        untouched = np.array(sorted({S, S + 1, fl.FIRST_SUB_AT_LINE - 1, OS - 1, OS + S, OS + fl.FIRST_SUB_AT_LINE - 1, OS + fl.LINE_SUB + S // 2,
                                     2 * OS - 1} | ({fl.FIRST_SUB_AT_LINE, OS + fl.LINE_SUB} if first_subint == fl.FIRST_SUB_BELOW else set())),
                             dtype=np.int64)
        assert np.all(lt.read_rows(gpu, d_p, fl.SUBINT_BYTES, untouched) == fl.PREFILL)
        assert np.all(lt.read_rows(gpu, d_s, nbin * 8, untouched) == fl.PREFILL)
    case.guard_untouched(d_p)
    case.guard_untouched(d_s)
