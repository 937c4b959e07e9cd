"""Every kernel held to its 64-bit offsets: one call per kernel at the smallest shape at which a tensor of its passes
2^32 bytes (helpers/large_tensor.py: the cases, the filling and the row sample; tests/test_large_tensor_plan.py shows on the
CPU that a wrapped offset would change what is compared here).

A base address, a hop, a row index or a line worked out in 32 bits wraps at 2^32 bytes: the kernel then reads or writes
inside the same allocation, 4 GiB lower, nothing faults and no canary is touched.  So the inputs are filled with a pattern
whose period does not divide 2^32, every output is exactly sized with a 64-byte canary and prefilled with 0xA5, and a
sample of rows -- both sides of every line, their alias rows 4 GiB lower, the ends and 64 seeded rows -- is compared bit for
bit with the numpy models of the small tests: a wrapped load gives other values, a wrapped store leaves the prefill above
the line and spoils the alias row.  No tolerance anywhere; nothing on the host is proportional to a tensor.

Not here: the incoherent beam's OUTPUT ([C][nt / 16] uint32) would need 32 GiB of samples to pass the line even with one
antenna; the fp32 chain form keeps its small bound tests, and the slow class and non-finite values are held bit for bit
at small shapes (tests/test_gpu_beamformer_exact_slow.py)."""
import numpy as np
import pytest

from conftest import rand_table
from helpers import filterbank_model, hip_graph, incoherent_model, stokes_model
from helpers import large_tensor as lt
from helpers.bacc_case import MIN_DEPTH, T_COEFF, blocks_on_some_wave, random_weights
from helpers.beam_complex_model import complex_model
from helpers.beam_power_model import block_power, integrate as integrate_power
from helpers.beam_quant_model import quantise
from helpers.beamformer_model import (acc_model, all_pairs_fast, first_difference, fused_model, normalise, weighted_coefficients)
from helpers.device_buffers import DeviceBuffers
from helpers.filterbank_model import same_bits

pytestmark = pytest.mark.gpu

PREFILL = 0xA5
DEVICE_LIMIT = 24 << 30


@pytest.fixture
def mem(gpu, record_property):
    """The device memory of one test: counted, and freed whatever the test's end."""
    m = DeviceBuffers(gpu, limit=DEVICE_LIMIT)
    yield m
    m.close()
    record_property("device bytes held", m.total)


def filled(mem, nbytes, pattern):
    d = mem.alloc(nbytes)
    lt.fill(mem.gpu, d, nbytes, pattern)
    return d


def not_trivial(exp):
    assert np.unique(exp).size >= 100, np.unique(exp).size


# ---------------------------------------------------------------------------------------------------------------- beamformers

class BF:
    """One beamformer case: the context with its table, the generator context that supplies the coefficient bits, the
    filled antenna tensor, the prefilled output, the row sample and the samples of its rows."""

    def __init__(self, gpu, oracle, mem, name, seed=0):
        from dc_sand_amd import BeamformerParameters
        from dc_sand_amd.generator import SteeringCoefficientGenerator

        A, B, C, nt, self.per_beam, _ = lt.BEAMFORMER_CASES[name]
        self.gpu, self.oracle, self.mem, self.A, self.B, self.C, self.nt, self.nblk = gpu, oracle, mem, A, B, C, nt, nt // 16
        self.rb_in, self.rb_out, self.rows = lt.beamformer_rows(name)
        self.in_bytes, self.out_bytes = self.rows * self.rb_in, self.rows * self.rb_out
        self.bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
        self.op = oracle.params_from(self.bp)
        self.table = rand_table(self.bp.n_pairs, seed=A + B + seed)  # [b * A + a]
        self.table_ab = np.ascontiguousarray(self.table.reshape(B, A).T).ravel()  # the generator's [a * B + b]
        self.g, self.gen = SteeringCoefficientGenerator(self.bp), SteeringCoefficientGenerator(self.bp)
        self.g.upload_delays(self.table)
        self.gen.upload_delays(self.table_ab)
        self.pattern = lt.int8_pattern(self.rb_in, seed=1000 * A + seed)
        self.d_ant = filled(mem, self.in_bytes, self.pattern)
        self.d_out = mem.out(self.out_bytes)
        self.d_w = mem.alloc(B * A * 4)
        self.sample = lt.plan(self.rb_in, self.rb_out, self.rows, seed=A + B + C)
        self.n = self.sample.size
        self.x = lt.rows_of(self.pattern, self.sample).view(np.int8).reshape(self.n, 1, A, 16, 2)
        self.chan, self.blk = self.sample // self.nblk, self.sample % self.nblk
        self._buf = None

    def coefficient_bits(self, channels, dts):
        """fp32 [len(dts)][len(channels)][A][B][2] from the GPU generator, one slab per channel, each asserted within 1 ULP
        of the oracle."""
        dts = np.ascontiguousarray(np.atleast_1d(np.asarray(dts, dtype=np.float32)))
        nbytes = dts.size * self.A * self.B * 8
        if self._buf is None or self._buf_bytes < nbytes:
            self._buf, self._buf_bytes = self.mem.out(nbytes, 0xFF, 0xFF), nbytes
        out = np.empty((dts.size, len(channels), self.A, self.B, 2), dtype=np.float32)
        for i, c in enumerate(channels):
            self.mem.refill(self._buf)
            self.gen.generate_slab_dt(self._buf, nbytes, int(c), 1, dts)
            coef = self.mem.read(self._buf, nbytes, np.float32, (dts.size, 1, self.A, self.B, 2))
            res = self.oracle.compare_generated(self.op, self.table_ab, dts, int(c), 1, np.ascontiguousarray(coef), nthreads=8)
            assert res["max_ulp"] <= 1 and res["first_over_1ulp"] == -1 and sum(res["hist"]) == coef.size, (int(c), res)
            out[:, i] = coef[:, 0]
        return out

    def coefficients_of_the_rows(self):
        """fp32 [n][A][B][2]: the coefficients at T_COEFF of every sampled row's channel."""
        from dc_sand_amd.generator import delta_times

        dt = delta_times(self.bp, T_COEFF, 1)
        assert all_pairs_fast(self.table_ab, dt, self.C, self.bp.SAMPLING_PERIOD), "a pair outside the fast classes: change the inputs"
        channels, inverse = np.unique(self.chan, return_inverse=True)
        return self.coefficient_bits(channels, dt)[0][inverse]

    def weights(self):
        w = random_weights(np.random.default_rng(self.A + 7 * self.B), self.B, self.A, zero_beam=self.B > 1)
        w[:, self.A // 2] = 0.0
        self.gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
        return w

    def floats(self, coef, complex_product, w=None):
        """The model's float beams [n][1][B][16][2] of the sampled rows."""
        s = None
        if w is not None:
            s, gh = normalise(w)
            coef = weighted_coefficients(coef, gh)
        return complex_model(coef, self.x, False, scale=s) if complex_product else acc_model(coef, self.x, scale=s)

    def run(self, call):
        """``call(stream)`` into the prefilled output; the sampled rows' bytes, the canary checked."""
        self.mem.refill(self.d_out)
        call(None)
        self.gpu.synchronize()
        got = lt.read_rows(self.gpu, self.d_out, self.rb_out, self.sample)
        self.mem.guard_untouched(self.d_out)
        return got

    def check_floats(self, what, call, exp):
        not_trivial(exp)
        got = self.run(call).view(np.float32).reshape(exp.shape)
        diff = first_difference(got, exp)
        assert diff is None, f"{what}; 'c' is the index into the row sample, row {self.sample.tolist()}: {diff}"

    def depth(self, record_property, what, call):
        """The launch as captured (the call has run once): several blocks on some wave, so the pair hop and the later
        pairs are what ran."""
        s = self.gpu.Stream()
        grid, block = hip_graph.largest_launch(hip_graph.launches(s, lambda: call(s.handle)))
        s.synchronize()
        proven = blocks_on_some_wave(self.B, self.C, self.nt, grid, block)
        record_property(f"{what}: gridDim.x, blockDim.x, blocks proven on some wave", (grid[0], block[0], proven))
        assert proven >= MIN_DEPTH, (what, grid, block, proven)

    def close(self):
        self.g.close()
        self.gen.close()


def float_calls(c, weighted):
    """(what, complex product?, weights?, call) of the float entry points."""
    g, tail = c.g, (c.d_out, c.out_bytes, c.nt)
    calls = [("element-wise", False, False, lambda s: g.beamform_accumulated(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, stream=s)),
             ("complex", True, False, lambda s: g.beamform_accumulated_complex(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, stream=s))]
    if weighted:
        calls += [("element-wise, weighted", False, True,
                   lambda s: g.beamform_accumulated_weighted(c.d_ant, c.in_bytes, c.d_w, *tail, t_coeff=T_COEFF, stream=s)),
                  ("complex, weighted", True, True,
                   lambda s: g.beamform_accumulated_complex(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, d_weights=c.d_w, stream=s))]
    return calls


def check_float_case(gpu, oracle, mem, record_property, name, weighted, complex_too=True):
    c = BF(gpu, oracle, mem, name)
    assert ("in" in lt.BEAMFORMER_CASES[name][5]) == (c.in_bytes > lt.LINE) and c.out_bytes > lt.LINE
    coef = c.coefficients_of_the_rows()
    w = c.weights() if weighted else None
    for what, complex_product, with_w, call in float_calls(c, weighted):
        if complex_product and not complex_too:
            continue
        c.check_floats(f"{name}, {what}", call, c.floats(coef, complex_product, w if with_w else None))
        c.depth(record_property, what, call)
    c.close()


def test_matrix_core_staged_whole(gpu, oracle, mem, record_property):
    """(A, B, C, nt) = (64, 16, 2048, 16400): antenna and float beams 4,299,161,600 bytes each."""
    check_float_case(gpu, oracle, mem, record_property, "staged_whole", weighted=True)


def test_matrix_core_chain_whole(gpu, oracle, mem, record_property):
    """(128, 32, 1024, 16400): antenna and float beams 4,299,161,600 bytes each."""
    check_float_case(gpu, oracle, mem, record_property, "chain_whole", weighted=True)


def test_matrix_core_chain_ragged(gpu, oracle, mem, record_property):
    """(130, 33, 1024, 16400), !FULL with a partial third beam tile: antenna 4,366,336,000, beams 4,433,510,400 bytes."""
    check_float_case(gpu, oracle, mem, record_property, "chain_ragged", weighted=False)


def test_matrix_core_staged_ragged_two_tiles(gpu, oracle, mem, record_property):
    """(48, 24, 4096, 10928): antenna 4,297,064,448 bytes, beams 8,594,128,896 (two lines)."""
    check_float_case(gpu, oracle, mem, record_property, "staged_ragged", weighted=False, complex_too=False)


@pytest.mark.parametrize("name", ["q8", "q8_chain"])
def test_8bit_beams(gpu, oracle, mem, record_property, name):
    """(64, 256, 512, 16400), four tiles per workgroup: int8 beams 4,299,161,600 bytes, element-wise and complex; and the
    same with 128 antennas, where kChain stores them.  The clip counters are compared for sanity only (exact counts would
    need the whole tensor; the small tests hold them exactly)."""
    c = BF(gpu, oracle, mem, name)
    assert c.out_bytes > lt.LINE
    coef = c.coefficients_of_the_rows()
    # |v| is about sqrt(A / 2) * 74 rms per component: gains that put one sigma at 20 .. 40, so that a few components clip
    gains = (20.0 / (np.sqrt(c.A / 2.0) * 74.0) * (1.0 + np.arange(c.B) / c.B)).astype(np.float32)
    d_k, d_clip = mem.alloc(c.B * 4), mem.alloc(c.B * 8)
    gpu.memcpy_htod(d_k, gains)
    tail = (d_k, c.d_out, c.out_bytes, c.nt)
    calls = [("element-wise", False, lambda s: c.g.beamform_accumulated_q8(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, d_clip_count=d_clip, stream=s)),
             ("complex", True, lambda s: c.g.beamform_accumulated_complex_q8(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, d_clip_count=d_clip, stream=s))]
    for what, complex_product, call in calls:
        exp, _ = quantise(c.floats(coef, complex_product), gains)
        not_trivial(exp)
        gpu.memset(d_clip, 0, c.B * 8)
        got = c.run(call).view(np.int8).reshape(exp.shape)
        assert same_bits(got, exp) is None, (what, same_bits(got, exp))
        clips = np.empty(c.B, dtype=np.uint64)
        gpu.memcpy_dtoh(clips, d_clip)
        assert np.all(clips <= np.uint64(c.C * c.nt * 2)), clips
        c.depth(record_property, what, call)
    c.close()


@pytest.mark.parametrize("name", ["power", "power_chain"])
def test_block_power_and_its_integration(gpu, oracle, mem, record_property, name):
    """(64, 1024, 1024, 16400): block power 4,299,161,600 bytes, element-wise and complex; then integrate_block_power of that
    tensor with n = 1 (spectra of the same size: a permutation of the rows) and n = 5.  And the two detecting calls with 128
    antennas, where kChain stores the power (antenna 4,299,161,600 bytes as well)."""
    from dc_sand_amd.generator import power_spectra_bytes

    c = BF(gpu, oracle, mem, name)
    assert c.out_bytes > lt.LINE
    coef = c.coefficients_of_the_rows()
    tail = (c.d_out, c.out_bytes, c.nt)
    calls = [("element-wise", False, lambda s: c.g.beamform_accumulated_power(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, stream=s)),
             ("complex", True, lambda s: c.g.beamform_accumulated_complex_power(c.d_ant, c.in_bytes, *tail, t_coeff=T_COEFF, stream=s))]
    for what, complex_product, call in calls:
        exp = block_power(c.floats(coef, complex_product))  # [n][1][B]
        not_trivial(exp)
        got = c.run(call).view(np.float32).reshape(exp.shape)
        assert same_bits(got, exp) is None, (what, same_bits(got, exp))
        c.depth(record_property, what, call)
    if name != "power":
        c.close()
        return
    # ---- the integrations of the tensor the complex call left: in row (c, block), out row (block / n, c)
    C, K, B, rb = c.C, c.nblk, c.B, c.rb_out
    d_s = mem.out(c.out_bytes)
    for n in (1, 5):
        sbytes = power_spectra_bytes(c.bp, K, n)
        assert (sbytes > lt.LINE) == (n == 1)
        # the sampled in rows and, so that both tensors' lines are covered, the in rows of the sampled out rows
        if n == 1:
            rows_in = lt.plan(rb, rb, c.rows, seed=n, extra=[(o % C) * K + o // C for o in lt.plan(rb, rb, c.rows, seed=n)])
        else:
            rows_in = c.sample
        ch, group = rows_in // K, (rows_in % K) // n
        out_rows, first = np.unique(group * C + ch, return_index=True)
        ch, group = ch[first], group[first]
        members = np.unique((ch * K + group * n)[:, None] + np.arange(n)[None, :])  # ascending and distinct
        P = lt.read_rows(gpu, c.d_out, rb, members).view(np.float32)  # [m * n][B]: the very input
        index = np.searchsorted(members, (ch * K + group * n)[:, None] + np.arange(n)[None, :])
        exp = integrate_power(P[index], n)[0]  # [m][n][B] as [C'][blocks][B] -> [1][m][B]
        not_trivial(exp)
        mem.refill(d_s)
        c.g.integrate_block_power(c.d_out, c.out_bytes, K, n, d_s, sbytes)
        gpu.synchronize()
        got = lt.read_rows(gpu, d_s, rb, out_rows).view(np.float32)
        mem.guard_untouched(d_s, sbytes)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
    c.close()


def check_fused(gpu, oracle, mem, name):
    """generate_and_beamform over all nt (> 256: the delta times are staged through pinned memory, in several chunks)."""
    from dc_sand_amd.generator import delta_times

    c = BF(gpu, oracle, mem, name)
    assert max(c.in_bytes, c.out_bytes) > lt.LINE and c.nt > 256
    dts = delta_times(c.bp, 0, c.nt)
    assert all_pairs_fast(c.table_ab, dts, c.C, c.bp.SAMPLING_PERIOD), "a pair outside the fast classes: change the inputs"
    exp = np.empty((c.n, 1, c.B, 16, 2), dtype=np.float32)
    for blk in np.unique(c.blk):  # the rows of one block share its 16 times
        rows = np.flatnonzero(c.blk == blk)
        coef = c.coefficient_bits(c.chan[rows], dts[16 * blk:16 * blk + 16])  # [16][k][A][B][2]
        exp[rows] = fused_model(coef, c.x[rows])
    c.check_floats(name, lambda s: c.g.generate_and_beamform(c.d_ant, c.in_bytes, c.d_out, c.out_bytes, t0=0, nt=c.nt, stream=s), exp)
    c.close()


def test_fused_kernel_output_past_the_line(gpu, oracle, mem):
    """(4, 512, 2048, 528): float beams 4,429,185,024 bytes."""
    check_fused(gpu, oracle, mem, "fused_output")


def test_fused_kernel_samples_past_the_line(gpu, oracle, mem):
    """(256, 1, 8192, 1040): antenna 4,362,076,160 bytes."""
    check_fused(gpu, oracle, mem, "fused_samples")


# ------------------------------------------------------------------------------------------ detection, integration, filterbanks

def context(C, A=1, B=1, nt=16):
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import SteeringCoefficientGenerator

    bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=nt)
    return bp, SteeringCoefficientGenerator(bp)


def test_stokes_block(gpu, mem):
    """(B, C, nt) = (64, 4096, 16400): x and y 8,598,323,200 bytes each (two lines), IQUV 4,299,161,600; nr_stokes 4 and 1."""
    B, C, nt = lt.STOKES_SHAPE
    rows, rb_in = C * (nt // 16), B * 32
    in_bytes = rows * rb_in
    bp, g = context(C, B=B, nt=nt)
    px, py = lt.int8_pattern(rb_in, seed=1), lt.int8_pattern(rb_in, seed=2)
    d_x, d_y = filled(mem, in_bytes, px), filled(mem, in_bytes, py)
    d_bs = mem.out(rows * B * 16)
    assert in_bytes > 2 * lt.LINE and rows * B * 16 > lt.LINE
    for ns in (4, 1):
        rb_out = B * 4 * ns
        sample = lt.plan(rb_in, rb_out, rows, seed=ns)
        x = lt.rows_of(px, sample).view(np.int8).reshape(-1, 1, B, 16, 2)
        y = lt.rows_of(py, sample).view(np.int8).reshape(-1, 1, B, 16, 2)
        exp = stokes_model.block_stokes(x, y, ns)
        not_trivial(exp)
        mem.refill(d_bs)
        g.stokes_block(d_x, d_y, in_bytes, d_bs, rows * rb_out, nt, nr_stokes=ns)
        gpu.synchronize()
        got = lt.read_rows(gpu, d_bs, rb_out, sample).view(np.int32).reshape(exp.shape)
        mem.guard_untouched(d_bs, rows * rb_out)
        assert np.array_equal(got, exp), (ns, sample[np.argwhere(got != exp)[:4, 0]], np.argwhere(got != exp)[:4])
    g.close()


def test_integrate_stokes(gpu, mem):
    """IQUV of the shape above, 4,299,161,600 bytes of planted block values in; n = 1 (spectra of the same size: out row
    (block, c) is in row (c, block)) and n = 5."""
    from dc_sand_amd.generator import stokes_spectra_bytes

    B, C, nt = lt.STOKES_SHAPE
    K, ns, rb = nt // 16, 4, B * 16
    rows = C * K
    in_bytes = rows * rb
    bp, g = context(C, B=B, nt=nt)
    pattern = lt.stokes_int32_pattern(B * ns, seed=3)
    d_bs = filled(mem, in_bytes, pattern)
    d_s = mem.out(in_bytes)
    assert in_bytes > lt.LINE
    for n in (1, 5):
        sbytes = stokes_spectra_bytes(bp, K, n, ns)
        assert (sbytes > lt.LINE) == (n == 1)
        base = lt.plan(rb, rb, rows, seed=n)
        rows_in = lt.plan(rb, rb, rows, seed=n, extra=[(o % C) * K + o // C for o in base]) if n == 1 else base
        ch, group = rows_in // K, (rows_in % K) // n
        out_rows, first = np.unique(group * C + ch, return_index=True)
        ch, group = ch[first], group[first]
        members = (ch * K + group * n)[:, None] + np.arange(n)[None, :]
        block = lt.rows_of(pattern, members.ravel()).view(np.int32).reshape(-1, n, B, ns)  # [m][n][B][ns] as [C'][blocks][B][ns]
        exp = stokes_model.integrate(block, n)[0]  # [m][B][ns]
        not_trivial(exp)
        if n == 5:  # sums beyond 2^24 that are no floats, of both signs: the one rounding is exercised
            S = block.astype(np.int64).sum(axis=1)
            inexact = (np.abs(S) > 1 << 24) & (exp.astype(np.float64) != S)
            assert (inexact & (S > 0)).any() and (inexact & (S < 0)).any()
        mem.refill(d_s)
        g.integrate_stokes(d_bs, in_bytes, K, n, ns, d_s, sbytes)
        gpu.synchronize()
        got = lt.read_rows(gpu, d_s, rb, out_rows).view(np.float32).reshape(exp.shape)
        mem.guard_untouched(d_s, sbytes)
        assert same_bits(got, exp) is None, (n, same_bits(got, exp))
    g.close()


@pytest.mark.parametrize("A,C,nt", lt.INCOHERENT_SHAPES)
def test_incoherent_block_power(gpu, mem, A, C, nt):
    """(A, C, nt) = (256, 2048, 4112): antenna 4,311,744,512 bytes; (130, 2048, 8080): 4,302,438,400, five loads per row,
    ragged.  The output is small and read whole."""
    rows, rb_in = C * (nt // 16), A * 32
    in_bytes = rows * rb_in
    assert lt.LINE < in_bytes < 1.04 * lt.LINE
    bp, g = context(C, A=A, nt=nt)
    pattern = lt.int8_pattern(rb_in, seed=A)
    d_ant = filled(mem, in_bytes, pattern)
    d_p = mem.out(rows * 4)
    # a row is one value here: 192 seeded rows more, so that the expectation has its 100 distinct values
    sample = lt.plan(rb_in, 4, rows, seed=A, extra=np.random.default_rng(A + 1).integers(0, rows, size=192))
    exp =incoherent_model.block_power(lt.rows_of(pattern, sample).view(np.int8).reshape(-1, 1, A, 16, 2)).ravel()
    not_trivial(exp)
    g.incoherent_block_power(d_ant, in_bytes, d_p, rows * 4, nt)
    gpu.synchronize()
    got = mem.read(d_p, rows * 4, np.uint32)[sample]
    assert np.array_equal(got, exp), (sample[np.flatnonzero(got != exp)[:4]], got[got != exp][:4], exp[got != exp][:4])
    g.close()


TARGET_STD, LEVEL = 24.0, 128.0


def test_filterbank_calls_on_spectra_past_the_line(gpu, mem):
    """(C, NB, T) = (4096, 64, 4100): spectra 4,299,161,600 bytes; spectrum 4096 begins on the line.  spectra_sums of
    sampled (channel, beam) series rebuilt from the pattern, all 4100 values; the scales; filterbank_q8 in both channel
    orders with the scales the GPU made, at sampled spectra and every beam."""
    from dc_sand_amd.generator import filterbank_bytes, filterbank_scales_bytes, spectra_sums_bytes

    C, NB, T = lt.FILTERBANK_SHAPE
    xbytes = T * C * NB * 4
    assert lt.LINE < xbytes < 1.04 * lt.LINE
    bp, g = context(C)
    pattern = lt.spectra_pattern(NB, seed=5)  # rows (spectrum, channel) of NB floats
    d_x = filled(mem, xbytes, pattern)
    ub, kb, fb = spectra_sums_bytes(bp, NB), filterbank_scales_bytes(bp, NB), filterbank_bytes(bp, NB, T)
    d_sums, d_scales, d_fb, d_clip = mem.out(ub), mem.out(kb), mem.out(fb), mem.alloc(NB * 8)

    # ---- sums and scales of 258 series
    rng = np.random.default_rng(6)
    cs = np.concatenate([[0, C - 1], rng.integers(0, C, 256)])
    bs = np.concatenate([[0, NB - 1], rng.integers(0, NB, 256)])
    series = lt.elements_of(pattern, (np.arange(T, dtype=np.int64)[:, None] * C + cs[None, :]) * NB + bs[None, :])  # [T][258]
    exp_sums = filterbank_model.spectra_sums(series[:, :, None])  # [258][1][2]
    g.spectra_sums(d_x, xbytes, T, NB, d_sums, ub)
    g.filterbank_scales(d_sums, ub, T, NB, TARGET_STD, d_scales, kb)
    gpu.synchronize()
    sums = mem.read(d_sums, ub, np.float64, (C, NB, 2))
    assert same_bits(sums[cs, bs], exp_sums[:, 0]) is None, same_bits(sums[cs, bs], exp_sums[:, 0])
    scales = mem.read(d_scales, kb, np.float32, (C, NB, 2))
    exp_scales = filterbank_model.scales(exp_sums, T, TARGET_STD)
    assert same_bits(scales[cs, bs], exp_scales[:, 0]) is None, same_bits(scales[cs, bs], exp_scales[:, 0])
    assert np.unique(exp_sums).size >= 100 and np.unique(exp_scales).size >= 100

    # ---- the bytes of sampled spectra, every channel and beam of them: out row (beam, spectrum) of C bytes
    ts = lt.plan(C * NB * 4, C * NB * 4, T, seed=7)
    assert {0, 4095, 4096, 4097, T - 1} <= set(ts.tolist()) and ts.size * C * NB * 4 <= lt.HOST_LIMIT
    x = lt.elements_of(pattern, ts[:, None] * (C * NB) + np.arange(C * NB, dtype=np.int64)[None, :]).reshape(ts.size, C, NB)
    q, _ = filterbank_model.quantise(x, scales, LEVEL)  # [nT][C][NB]
    not_trivial(q)
    out_rows = (np.arange(NB)[:, None] * T + ts[None, :]).ravel()
    for descending in (False, True):
        exp = np.transpose(q[:, ::-1] if descending else q, (2, 0, 1)).reshape(-1, C)
        mem.refill(d_fb)
        gpu.memset(d_clip, 0, NB * 8)
        g.filterbank_q8(d_x, xbytes, T, NB, d_scales, LEVEL, d_fb, fb, T, descending=descending, d_clip_count=d_clip)
        gpu.synchronize()
        got = lt.read_rows(gpu, d_fb, C, out_rows)
        mem.guard_untouched(d_fb)
        assert same_bits(got, exp) is None, (descending, same_bits(got, exp))
        clips = np.empty(NB, dtype=np.uint64)
        gpu.memcpy_dtoh(clips, d_clip)
        assert np.all(clips <= np.uint64(T * C)), clips
    g.close()


def test_filterbank_into_a_ring_past_the_line(gpu, mem):
    """(C, NB) = (4096, 64), out_spectra 16400, T = 8 at first_spectrum 16392, both orders: the filterbanks are
    4,299,161,600 bytes and the last beam's last rows lie past the line.  Every sampled row that is not written keeps the
    prefill, the rows 4 GiB below the written ones among them."""
    from dc_sand_amd.generator import filterbank_bytes

    C, NB, out_spectra, T, first = lt.RING_SHAPE
    bp, g = context(C)
    fb = filterbank_bytes(bp, NB, out_spectra)
    assert lt.LINE < fb < 1.04 * lt.LINE and ((NB - 1) * out_spectra + first) * C > lt.LINE
    g_ = np.random.default_rng(8).standard_normal((T, C, NB))
    m = np.exp2(np.random.default_rng(9).uniform(-20.0, 20.0, size=(C, NB)))
    x = (m[None] * (1.0 + 0.25 * g_)).astype(np.float32)
    scales = np.stack([m.astype(np.float32), (TARGET_STD / (0.25 * m)).astype(np.float32)], axis=-1)  # of the distribution itself
    d_x, d_scales = mem.alloc(x.nbytes), mem.alloc(scales.nbytes)
    gpu.memcpy_htod(d_x, x)
    gpu.memcpy_htod(d_scales, scales)
    d_fb = mem.out(fb)
    q, _ = filterbank_model.quantise(x, scales, LEVEL)  # [T][C][NB]
    not_trivial(q)
    rows = NB * out_spectra
    written = [b * out_spectra + first + t for b in (0, NB // 2, NB - 2, NB - 1) for t in range(T)]
    sample = lt.plan(C, C, rows, seed=10, extra=written)
    beam, spectrum = sample // out_spectra, sample % out_spectra
    assert np.count_nonzero(spectrum >= first) >= len(written) and np.count_nonzero(spectrum < first) >= 64
    for descending in (False, True):
        exp = np.full((sample.size, C), PREFILL, dtype=np.uint8)
        for i in np.flatnonzero(spectrum >= first):
            row = q[spectrum[i] - first, :, beam[i]]
            exp[i] = row[::-1] if descending else row
        mem.refill(d_fb)
        g.filterbank_q8(d_x, x.nbytes, T, NB, d_scales, LEVEL, d_fb, fb, out_spectra, first_spectrum=first, descending=descending)
        gpu.synchronize()
        got = lt.read_rows(gpu, d_fb, C, sample)
        mem.guard_untouched(d_fb)
        assert same_bits(got, exp) is None, (descending, same_bits(got, exp), sample)
    g.close()
