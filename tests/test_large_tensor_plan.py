"""The plans of tests/test_gpu_large_tensors.py, without a device: that each tensor named as passing 2^32 bytes does, that
the pattern's period does not divide 2^32, that the row sample holds the rows it promises, and -- the CPU stand-in for
"would fail if the kernel's offsets were 32-bit" -- that for every sampled row above a line the bytes 4 GiB lower differ from
the row's own, and with them the exact models' outputs."""
import numpy as np
import pytest

from helpers import filterbank_model, incoherent_model, stokes_model
from helpers import large_tensor as lt

CASES = lt.row_cases()
IDS = [c[0] for c in CASES]

# the sizes of the issue's tables
SIZES = {
    "staged_whole": (4299161600, 4299161600), "chain_whole": (4299161600, 4299161600),
    "chain_ragged": (4366336000, 4433510400), "staged_ragged": (4297064448, 8594128896),
    "q8": (None, 4299161600), "power": (None, 4299161600),
    "q8_chain": (None, 4299161600), "power_chain": (4299161600, 4299161600), "fused_output": (None, 4429185024),
    "fused_samples": (4362076160, None), "stokes_iquv": (8598323200, 4299161600), "stokes_i": (8598323200, None),
    "integrate_stokes": (4299161600, 4299161600), "integrate_block_power": (4299161600, 4299161600),
    "incoherent_256": (4311744512, None), "incoherent_130": (4302438400, None), "filterbank": (4299161600, None),
    "filterbank_ring": (None, 4299161600),
}


def pattern_of(name, rb_in):
    if name == "integrate_stokes":
        return lt.stokes_int32_pattern(rb_in // 4, seed=3)
    if name in ("filterbank", "integrate_block_power"):
        return lt.spectra_pattern(rb_in // 4, seed=5)
    return lt.int8_pattern(rb_in, seed=1)


@pytest.mark.parametrize("name,rb_in,rb_out,rows,crossing", CASES, ids=IDS)
def test_sizes_and_period(name, rb_in, rb_out, rows, crossing):
    assert set(SIZES) == set(IDS)
    for which, rb, want in (("in", rb_in, SIZES[name][0]), ("out", rb_out, SIZES[name][1])):
        nbytes = rows * rb
        if which in crossing:
            assert nbytes == want and nbytes > lt.LINE
            # one shape can pass one tensor's line by a little; where input and output differ in size, or a tensor is twice
            # another (x and y against IQUV, two beam tiles), the larger passes one or two lines by as little
            assert nbytes % lt.LINE < 0.04 * lt.LINE, (name, which, nbytes / lt.LINE)
        else:
            assert want is None and nbytes <= lt.LINE
    for rb in {rb_in, rb_out}:
        p = lt.period_rows(rb)
        assert p > 1 and p % 2 == 1 and lt.LINE % (p * rb) != 0 and p * rb <= lt.HOST_LIMIT
    # grids beyond 2^31 workgroups are refused by the launchers: no case comes near (a workgroup takes at least one row)
    assert rows < 1 << 27


def brute_alias_rows(rb, r, k):
    return {(o - k * lt.LINE) // rb for o in (r * rb, (r + 1) * rb - 1) if o - k * lt.LINE >= 0}


@pytest.mark.parametrize("name,rb_in,rb_out,rows,crossing", CASES, ids=IDS)
def test_the_sample_holds_the_rows_it_promises(name, rb_in, rb_out, rows, crossing):
    sample = lt.plan(rb_in, rb_out, rows, seed=11)
    have = set(sample.tolist())
    assert np.all(np.diff(sample) > 0) and sample[0] == 0 and sample[-1] == rows - 1
    assert {0, 1, rows - 2, rows - 1} <= have
    seeded = set(np.random.default_rng(11).integers(0, rows, size=64).tolist())
    assert seeded <= have and len(seeded) >= 60
    for rb in (rb_in, rb_out):
        nbytes = rows * rb
        for k in range(1, nbytes // lt.LINE + 1):
            line = k * lt.LINE
            if line >= nbytes:
                continue
            r = line // rb
            assert r * rb <= line < (r + 1) * rb and {r - 1, r} <= have and (r + 1 in have or r + 1 == rows)
        for r in (set(range(rows - 2, rows)) | seeded) & have:  # and the alias rows of what lies at or above a line
            for k in (1, 2):
                assert brute_alias_rows(rb, r, k) <= have, (r, k)
    assert sample.size * max(rb_in, rb_out) <= lt.HOST_LIMIT and sample.size <= 1024
    # a sample with extra rows holds them and their aliases
    more = set(lt.plan(rb_in, rb_out, rows, seed=11, extra=[rows - 3]).tolist())
    assert have <= more and rows - 3 in more and brute_alias_rows(rb_in, rows - 3, 1) <= more


def model_of(name, rb_in):
    """The exact-integer (or exact-order) model of one input row's bytes, where the case has one."""
    if name in ("stokes_iquv", "stokes_i"):
        y = lt.rows_of(lt.int8_pattern(rb_in, seed=2), [5]).view(np.int8).reshape(1, 1, -1, 16, 2)  # any fixed row of y
        ns = 4 if name == "stokes_iquv" else 1
        return lambda b: stokes_model.block_stokes(b.view(np.int8).reshape(1, 1, -1, 16, 2), y, ns)
    if name.startswith("incoherent"):
        return lambda b: incoherent_model.block_power(b.view(np.int8).reshape(1, 1, -1, 16, 2))
    if name == "integrate_stokes":
        return lambda b: stokes_model.integrate(b.view(np.int32).reshape(1, 1, -1, 4), 1)
    if name == "filterbank":
        k = np.stack([np.full(rb_in // 4, 1000.0, np.float32), np.full(rb_in // 4, 24.0 / 250.0, np.float32)], axis=-1)[None]
        return lambda b: filterbank_model.quantise(b.view(np.float32).reshape(1, 1, -1), k, 128.0)[0]
    return None


@pytest.mark.parametrize("name,rb_in,rb_out,rows,crossing", CASES, ids=IDS)
def test_a_wrapped_offset_would_show(name, rb_in, rb_out, rows, crossing):
    """Input side: the bytes k * 2^32 below every sampled row at or above a line differ from the row's own, and so does the
    model's output.  Output side: a wrapped store lands on the alias rows, whose own expectation (the model of THEIR input
    rows) differs from what landed there -- the same inequality between a row and its alias."""
    if name == "filterbank_ring":  # no input rows: a written row (model bytes) and a row that keeps the prefill
        C, NB, out_spectra, T, first = lt.RING_SHAPE
        written = [(NB - 1) * out_spectra + first + t for t in range(T)]
        sample = lt.plan(rb_out, rb_out, rows, seed=10, extra=written)
        for r in written:
            assert r * rb_out > lt.LINE and r in sample
            for a in brute_alias_rows(rb_out, r, 1):
                assert a in sample and a % out_spectra < first  # the alias must stay as prefilled
        return
    pattern = pattern_of(name, rb_in)
    flat = np.ascontiguousarray(pattern).reshape(-1).view(np.uint8)
    assert flat.size == lt.period_rows(rb_in) * rb_in
    sample = lt.plan(rb_in, rb_out, rows, seed=11)
    model = model_of(name, rb_in)
    seen = 0
    for r in sample.tolist():
        own = lt.rows_of(pattern, [r])[0]
        for k in (1, 2):
            below = lt.row_as_wrapped(pattern, rb_in, r, k) if "in" in crossing else None
            if below is not None:
                assert not np.array_equal(own, below), (r, k)
                if model is not None:
                    assert not np.array_equal(model(own), model(below)), (r, k)
                seen += 1
            if "out" in crossing:  # input row r gives output row r: its alias rows' inputs differ from its own
                for a in brute_alias_rows(rb_out, r, k):
                    assert a != r and not np.array_equal(own, lt.rows_of(pattern, [a])[0]), (r, a, k)
                    if model is not None:
                        assert not np.array_equal(model(own), model(lt.rows_of(pattern, [a])[0])), (r, a, k)
                    seen += 1
    assert seen >= 4, seen


def test_fill_rows_and_reads_agree_on_a_host_stand_in():
    """fill, rows_of, elements_of and read_rows against a numpy buffer standing in for the device."""
    class Host:
        def __init__(self, nbytes):
            self.mem = np.zeros(nbytes, np.uint8)

        def memcpy_htod(self, dst, src):
            src = np.ascontiguousarray(src).reshape(-1).view(np.uint8)
            self.mem[dst:dst + src.size] = src

        def memcpy_dtod(self, dst, src, n):
            self.mem[dst:dst + n] = self.mem[src:src + n].copy()

        def memcpy_dtoh(self, dst, src):
            dst.reshape(-1).view(np.uint8)[:] = self.mem[src:src + dst.nbytes]

        def synchronize(self):
            pass

    rb, rows = 24, 1000
    pattern = np.random.default_rng(0).integers(-128, 128, size=(7, rb), dtype=np.int8)
    host = Host(rows * rb)
    lt.fill(host, 0, rows * rb, pattern)
    whole = host.mem.reshape(rows, rb)
    assert np.array_equal(whole, np.tile(pattern.view(np.uint8), (rows // 7 + 1, 1))[:rows])
    some = np.array([0, 1, 2, 10, 500, 501, 999])
    assert np.array_equal(lt.rows_of(pattern, some), whole[some]) and np.array_equal(lt.read_rows(host, 0, rb, some), whole[some])
    index = np.array([[0, 5], [23999, 168]])
    assert np.array_equal(lt.elements_of(pattern, index).view(np.uint8), host.mem[index])
    short = Host(50)  # a tensor smaller than the pattern
    lt.fill(short, 0, 50, pattern)
    assert np.array_equal(short.mem, pattern.view(np.uint8).ravel()[:50])
