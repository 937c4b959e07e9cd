"""The complex-product beamformer (include/dcs_beam_complex.h, dcs_beam_complex_quant.h; DESIGN.md sections 5.13, 5.14) on
structured inputs: the low part beyond int32, full-scale samples, one antenna at a time, a seeded fuzz over shapes.

tests/test_gpu_beam_complex.py and test_gpu_beam_complex_quant.py feed uniform random samples and seeded tables; nothing
there comes near S2 * 256 + S3 > 2^31 - 1, the one place where the kernels' fmaf((float)s2, 256.0f, (float)s3) and the
element-wise kernels' (float)(s2 * 256 + s3) differ, and a mix-up of re, +im and -im in one antenna shows only statistically.

Every comparison is equality of uint32 or byte views against the model (helpers/beam_complex_model.py) on the GPU
generator's coefficient bits (Exact), no tolerance anywhere; the canary behind every buffer must be intact.  "Power" is
block_power of the model's floats bit for bit, "q8" the bytes AND clip counters of helpers/beam_quant_model.py on them."""
from functools import partial

import numpy as np
import pytest

from conftest import rand_table
from helpers import complex_edges as ce
from helpers.bacc_case import T_COEFF, random_weights
from helpers.beam_complex_model import SUM_BOUND, digit_sums, operands, recombine
from helpers.beam_power_model import block_power, same_bits
from helpers.beam_quant_model import gains_with_clipping, gains_without_clipping, quantise
from helpers.beamformer_model import F32, digits, first_difference, normalise, weighted_coefficients
from helpers.device_buffers import closed_after
from test_gpu_beam_complex_quant import CQ, ExactQ
from test_gpu_beam_quant import same
from test_gpu_beamformer_exact import constant_table, full_scale_samples, one_hot_samples, weights_for

pytestmark = pytest.mark.gpu


@pytest.fixture
def exactq(gpu, oracle):
    yield from closed_after(partial(ExactQ, gpu, oracle))


class Calls:
    """The three complex calls of a CQ at one coefficient time (t_coeff= or dt_coeff=), each from clean buffers, and their
    comparison with the model of the coefficient bits ``coef`` of that time."""

    def __init__(self, x, coef, **time):
        self.x, self.c, self.coef, self.time = x, x.c, coef, time
        self.largest_sum = 0

    def model(self, conj, w=None):
        """(the model's floats, its integer sums); every sum within the bound of the contract."""
        if w is None:
            sums, s = digit_sums(self.coef, self.c.ant, conj), None
        else:
            s, gh = normalise(w)
            sums = digit_sums(weighted_coefficients(self.coef, gh), self.c.ant, conj)
        self.largest_sum = max([self.largest_sum] + [int(np.abs(v).max()) for v in sums])
        exp = recombine(*sums, scale=s)
        assert np.all(np.isfinite(exp))
        return exp, sums

    def _weights(self, w):
        if w is not None:
            self.c.gpu.memcpy_htod(self.c.d_w, np.ascontiguousarray(w, dtype=np.float32))
        return None if w is None else self.c.d_w

    def floats(self, conj, w=None):
        c = self.c
        c.refill(c.d_beams)
        c.g.beamform_accumulated_complex(c.d_ant, c.ant.nbytes, c.d_beams, c.nbytes, c.nt, d_weights=self._weights(w),
                                         conjugate=conj, **self.time)
        return c.read_beams()  # (synchronises; asserts the canary)

    def power(self, conj, w=None):
        x, c = self.x, self.c
        c.refill(x.d_p)
        c.g.beamform_accumulated_complex_power(c.d_ant, c.ant.nbytes, x.d_p, x.pbytes, c.nt, d_weights=self._weights(w),
                                               conjugate=conj, **self.time)
        c.gpu.synchronize()
        return x.read_power()  # (asserts the canary)

    def q8(self, gains, conj, w=None):
        c = self.c
        c.refill(c.d_q)
        c.gpu.memcpy_htod(c.d_k, np.ascontiguousarray(gains, dtype=np.float32))
        c.gpu.memset(c.d_clip, 0, c.B * 8)
        c.g.beamform_accumulated_complex_q8(c.d_ant, c.ant.nbytes, c.d_k, c.d_q, c.qbytes, c.nt, d_weights=self._weights(w),
                                            conjugate=conj, d_clip_count=c.d_clip, **self.time)
        c.gpu.synchronize()
        return c.read_q8(), c.counts()  # (asserts the canary)

    def check(self, conj, w=None, power=False, q8=(), what=""):
        """The float call, and on request the detecting one and the quantising one with each gain set of ``q8`` (functions
        of the model's floats, or arrays), against the model.  Returns the model's floats and integer sums."""
        c = self.c
        what = f"{what}, conjugate {conj}, {'weighted' if w is not None else 'unweighted'}, {self.time}, (A, B, C, nt) = {(c.A, c.B, c.C, c.nt)}"
        exp, sums = self.model(conj, w)
        diff = first_difference(self.floats(conj, w), exp)
        assert diff is None, f"float, {what}: {diff}"
        if power:
            diff = same_bits(self.power(conj, w), block_power(exp))
            assert diff is None, f"power, {what}: {diff}"
        for gains in q8:
            k = gains(exp) if callable(gains) else gains
            q_exp, n_exp = quantise(exp, k)
            got, n = self.q8(k, conj, w)
            assert same(got, q_exp) is None, f"q8, {what}: {same(got, q_exp)}"
            assert np.array_equal(n, n_exp), f"q8 clip counters, {what}: {n} for {n_exp}"
        return exp, sums


def time_by_index(c, t=T_COEFF):
    from dc_sand_amd.generator import delta_times

    return delta_times(c.bp, t, 1)[0], {"t_coeff": t}


# ---- a. the low part beyond int32
WRAP_SHAPE = (256, 17, 2, 32)  # kChain, four whole chunks, a ragged second beam tile
DRIVEN = (3, 16)               # one beam of each tile
Q8_GAIN = 127.0 / 45000.0      # the driven beams' |v| of about 41904 lands at 118


def test_low_part_beyond_int32(gpu, oracle, exactq, record_property):
    """S2 * 256 + S3 > 2^31 - 1: the input for which the complex kernels form the low part with an fma.

    With every sample -128, low = 128 * (256 * P2 + P3), P_d the sum of -digit_d over the 2 * A operand digits of a plane;
    leaving int32 needs 256 * P2 + P3 >= 2^24 at 256 antennas, so the 512 middle digits may fall short of -128 by 255 in
    total and P3 must make up 256 times the shortfall.  No unweighted table gets there: a unit-modulus coefficient never has
    the middle digit -128 in both components, so 256 antennas fall short by 256 at least (tests/
    test_beam_complex_edges_inputs.py).  With weights, s_b = max_a |g| leaves one such antenna (ghat = 1) and 255 that may
    take any ghat < 1 (helpers/complex_edges.py): antenna 0 at PHASE_0, whose cos has the digits (69, -128, -94) and whose
    sin the middle digit -119; the others at fp32(pi / 4) with the first fp32 weight g >= 0.9 that gives RN32(g * w) the digits
    (d1, -128, <= -110) in both components.  g is looked for at run time in the bits the GPU generator returned, per driven
    beam, and the digit conditions are asserted on those bits ("change the inputs" when they fail).

    Block 0 of every channel is all -128, block 1 seeded random; beams 3 and 16 carry the construction, the others random
    weights.  Asserted from the model first: in block 0 of both driven beams the exact low part is beyond int32 in the im
    plane (re with the conjugate flag), and the int32 form would give other floats and other bytes there.  Then the float,
    power and q8 outputs are the model's.  Second pass, the driven weights negated: the same integers negated (other
    digits, so the low part is another one and stays inside int32 -- the negative side cannot leave it: 127 * 128 < 2^14).

    On an MI355X the generator's bits are numpy's here: the scan gives g = 0.90397966 for both beams, the largest exact low part
    is 2155561088 = 2^31 + 8077440, the driven beams read -41904.375 (the int32 form: -42418.387; bytes -118 and -120), and
    the negated pass reaches 2147181184, inside int32.  With the integer form compiled into the kernels this test, and no
    other of the suite, fails: 64 of 2176 words differ, first at (c 0, block 0, beam 3, sample 0, plane 1)."""
    A, B, C, nt = WRAP_SHAPE
    table = constant_table(A * B, ce.PHASE_REST)
    table.reshape(B, A)["fPhase_rad"][:, 0] = ce.PHASE_0
    x = CQ(exactq(A, B, C, nt, table=table))
    c = x.c
    ant = c.ant.copy()
    ant[:, 0] = -128
    c.set_ant(ant)
    dt, time = time_by_index(c)
    coef = c.coefficient_bits(dt)[0]
    assert np.array_equal(table["fPhase_rad"].reshape(B, A)[0], ce.phases(A))
    gains = ce.wrap_gains(coef, DRIVEN)  # raises, naming the condition, when these bits do not admit the construction
    calls = Calls(x, coef, **time)
    others = [b for b in range(B) if b not in DRIVEN]
    totals = {}
    for sign in (1.0, -1.0):
        w = random_weights(np.random.default_rng(17), B, A, zero_beam=False)
        w[list(DRIVEN)] = ce.wrap_weights(coef, DRIVEN, sign)[list(DRIVEN)]
        s, gh = normalise(w)
        assert all(s[b] == 1 and gh[b, 0] == sign and np.all(gh[b, 1:] == F32(sign) * gains[b]) for b in DRIVEN)
        wc = weighted_coefficients(coef, gh)
        for conj in (False, True):
            plane = 0 if conj else 1
            exp, (s1, s2, s3) = calls.model(conj, w)
            low = ce.exact_low(s2, s3)
            v32 = ce.int32_model(wc, c.ant, conj, scale=s)
            k = gains_without_clipping(exp)
            k[list(DRIVEN)] = Q8_GAIN
            q, n = quantise(exp, k)
            q32, _ = quantise(v32, k)
            d = list(DRIVEN)
            assert low.min() >= -2 ** 31  # never on the negative side
            assert np.all(np.abs(low[:, :, others]) <= ce.INT32_MAX) and np.all(np.abs(low[:, 1]) <= ce.INT32_MAX)
            if sign > 0:
                assert np.all(low[:, 0, d, :, plane] > ce.INT32_MAX), f"the exact low part stays inside int32: {int(low[:, 0, d, :, plane].min())} -- change the inputs"
                assert np.all(exp[:, 0, d, :, plane] != v32[:, 0, d, :, plane]) and np.all(q[:, 0, d, :, plane] != q32[:, 0, d, :, plane])
                assert np.all(exp[:, 0, d, :, plane] < -40000) and np.all(np.abs(q[:, :, d].astype(int)) < 127) and np.all(n[d] == 0)
                totals[conj] = s1 * 65536 + low
                print(f"conjugate {conj}: g = {[repr(float(gains[b])) for b in DRIVEN]}, largest exact low part {int(low.max())} = 2^31 + "
                      f"{int(low.max()) - 2 ** 31}; beam 3: {float(exp[0, 0, 3, 0, plane])!r}, with the int32 form {float(v32[0, 0, 3, 0, plane])!r}; "
                      f"bytes {int(q[0, 0, 3, 0, plane])} and {int(q32[0, 0, 3, 0, plane])}")
                record_property(f"conjugate {conj}: g, largest exact low part", (float(gains[DRIVEN[0]]), int(low.max())))
            else:  # the same magnitudes with the opposite sign, and no low part outside int32 anywhere
                assert np.array_equal((s1 * 65536 + low)[:, :, d], -totals[conj][:, :, d])
                assert np.all(np.abs(low) <= ce.INT32_MAX) and first_difference(exp, v32) is None
                assert np.all(exp[:, 0, d, :, plane] > 40000)
                print(f"conjugate {conj}, negated: largest exact low part {int(low.max())}, smallest {int(low.min())}; beam 3: {float(exp[0, 0, 3, 0, plane])!r}")
            calls.check(conj, w, power=True, q8=(k,), what=f"the wrap inputs, sign {sign}")
    assert calls.largest_sum <= SUM_BOUND


# ---- b. full-scale samples
FULL_SCALE_SHAPES = [(64, 16, 2, 32), (256, 17, 2, 32), (200, 20, 2, 48)]  # staged; kChain whole and partial last chunk
FULL_SCALE_TABLES = {"zero": 0.0, "pi": np.float32(np.pi), "pi/2": np.float32(np.pi / 2), "pi/4": np.float32(np.pi / 4), "random": None}
FULL_SCALE_PATTERNS = (-128, 127, "alternating", "mixed")


def table_of(name, A, B):
    phase = FULL_SCALE_TABLES[name]
    return rand_table(A * B, seed=A + B) if phase is None else constant_table(A * B, phase)


def full_scale_pattern(pattern, C, nt, A):
    """full_scale_samples' patterns, and "mixed": -128 in re with 127 in im -- opposite-signed products in one plane."""
    if pattern != "mixed":
        return full_scale_samples(pattern, C, nt, A)
    x = np.empty((C, nt // 16, A, 16, 2), dtype=np.int8)
    x[..., 0], x[..., 1] = -128, 127
    return x


@pytest.mark.parametrize("A,B,C,nt", FULL_SCALE_SHAPES)
def test_full_scale_samples(gpu, oracle, exactq, A, B, C, nt):
    """Samples all -128, all 127, alternating by antenna, and -128 in re with 127 in im (opposite-signed products in one
    plane), against the constant tables of phase 0, fp32(pi), fp32(pi / 2), fp32(pi / 4) and the seeded random table, plain and
    conjugated: the float call always; at all -128 also power, q8 with both gain sets, and all of it weighted.

    The largest |S_d| these reach is 2 * 128 * 100 * A -- 6553600 = 0.78 * 2^23 at 256 antennas -- in the low digit at
    fp32(pi / 4), whose cos and sin both have the low digit -100, where both products of a plane have one sign (samples
    all -128: the im plane, or re conjugated).  The axis tables reach 128 * 128 * A (fp32(pi): -127 of cos = -1 and the -1 of
    sin = -8.7e-8 in one plane), the random table a random walk's few hundred thousand.  Asserted from the model."""
    x = CQ(exactq(A, B, C, nt))
    c = x.c
    w = weights_for(A, B, A + B)
    largest = 0
    for name in FULL_SCALE_TABLES:
        c.set_table(table_of(name, A, B))
        dt, time = time_by_index(c)
        calls = Calls(x, c.coefficient_bits(dt)[0], **time)
        for pattern in FULL_SCALE_PATTERNS:
            c.set_ant(full_scale_pattern(pattern, C, nt, A))
            for conj in (False, True):
                what = f"table {name}, samples {pattern}"
                if pattern == -128:
                    for wt in (None, w):
                        calls.check(conj, wt, power=True, q8=(gains_without_clipping, gains_with_clipping), what=what)
                else:
                    calls.check(conj, what=what)
        print(f"(A, B, C, nt) = {(A, B, C, nt)}, table {name}: largest |S_d| {calls.largest_sum}")
        largest = max(largest, calls.largest_sum)
    assert largest == 2 * 128 * 100 * A, (largest, 2 * 128 * 100 * A)


# ---- c. one antenna at a time
@pytest.mark.parametrize("A,B,C", [(37, 21, 2), (130, 20, 1), (256, 16, 1)])
def test_one_antenna_at_a_time(gpu, oracle, exactq, A, B, C):
    """one_hot_samples (nt = 16 * A: block k carries the value in antenna k's re and in antenna A - 1 - k's im, nothing
    else), values 1 and -128.  With x = (v, 0) in antenna k alone the two planes are v times the digits of F_re and of F_ip;
    with x = (0, v) they are v times the digits of F_in and of F_re: a wrong operand (re, +im, -im), a wrong digit or a wrong
    antenna index shows in the block the failure message names -- the block IS the antenna (re; A - 1 - block for im).
    Staged with ragged antennas; kChain with a partial last chunk of 2 antennas; kChain with four whole chunks.

    Asserted from the coefficient bits: some (antenna, beam) has a -128 among the low digits of F_ip or F_in, so "the digits
    of the negated number" are other digits than the negated ones.  Should a seed yield none, change the seed."""
    x = CQ(exactq(A, B, C, 16 * A))
    c = x.c
    dt, time = time_by_index(c)
    calls = Calls(x, c.coefficient_bits(dt)[0], **time)
    w = weights_for(A, B, A)
    for wt in (None, w):
        coef = calls.coef if wt is None else weighted_coefficients(calls.coef, normalise(wt)[1])
        for conj in (False, True):
            _, F_ip, F_in = operands(coef, conj)
            lows = np.stack([d for F in (F_ip, F_in) for d in digits(F)[1:]])
            assert np.any(lows == -128), "no -128 among the low digits of F_ip and F_in: change the table's seed"
    for value in (1, -128):
        c.set_ant(one_hot_samples(C, A, value))
        for wt in (None, w):
            for conj in (False, True):
                calls.check(conj, wt, what=f"one-hot samples of {value}")


# ---- d. seeded fuzz over shapes
def test_seeded_fuzz_bit_for_bit(gpu, oracle, exactq):
    """30 seeded cases in the style of tests/test_gpu_beamformer_exact.py's fuzz: antennas from the edges of the 64-antenna
    chunks or uniform in 1 .. 256, beams 1 .. 90 (mostly off the 16-beam tile), 1 .. 4 channels, 1 .. 40 sample blocks, time by
    index or by value, the conjugate flag alternating, weighted as well every third case; the float call always, power every
    second case, q8 (with and without clipping) every third."""
    rng = np.random.default_rng(20261019)
    clipped = 0
    for case in range(30):
        A = int(rng.choice([1, 3, 17, 63, 64, 65, 100, 128, 129, 191, 192, 200, 255, 256])) if case % 2 else int(rng.integers(1, 257))
        B = int(rng.integers(1, 91))
        C = int(rng.integers(1, 5))
        nblk = int(rng.integers(1, 41))
        if A * B * C * nblk > 600000:
            nblk = max(1, 600000 // (A * B * C))
        x = CQ(exactq(A, B, C, 16 * nblk, table=rand_table(A * B, seed=7000 + case),
                      ant=rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8)))
        if rng.integers(0, 2):
            dt = np.float32(rng.uniform(0.0, 1.5))
            time = {"dt_coeff": float(dt)}
        else:
            dt, time = time_by_index(x.c, int(rng.integers(0, 2000)))
        calls = Calls(x, x.c.coefficient_bits(dt)[0], **time)
        for wt in (None, weights_for(A, B, case)) if case % 3 == 0 else (None,):
            exp, _ = calls.check(bool(case % 2), wt, power=case % 2 == 0, q8=(gains_without_clipping, gains_with_clipping) if case % 3 == 0 else (),
                                 what=f"fuzz case {case}")
            if case % 3 == 0:
                clipped += int(quantise(exp, gains_with_clipping(exp))[1].sum())
        x.c.close()
    assert clipped > 1000  # the clipping branch and its counters took part
