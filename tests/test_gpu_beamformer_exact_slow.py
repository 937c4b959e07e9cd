"""Both beamformers held to their stated arithmetic in the SLOW class, bit for bit (include/dcs_beamformer.h,
include/dcs_beam_weights.h, include/dcs_beam_complex.h): the twin of tests/test_gpu_beamformer_exact.py for tables that
all_pairs_fast refuses.

With one slow-class pair a beamformer makes EVERY coefficient of the table (the fused kernel: of a 16-sample block) with
coeff_slow, in code of its own: four rolled trips that rotate the coefficient registers, ghat and terms loaded inside the
loop, no coefficient sharing between the waves of a tile, the notes that become NaN rows (bf_beamform_i8_kernel.inc); the
channel outermost and no prefetch rotation in the fused kernel (bf_beamform_kernel.inc).  The generator switches per run of
consecutive pairs instead (a wave's 128 or 256, a flag word's 64, a workgroup's 256), so the table as it is would give the
fast path's bits for most pairs.

The slow path's bits still come from the GPU GENERATOR, never from the kernel under test.  A pair's coefficient depends on
its four delay values, the time, C and the sampling period, not on its index or its neighbours, and every form of the
generator calls the same coeff_slow(fRateTerm, fPhase0, c, D) the beamformers call.  So a second generator context of the
same parameters with 2 B beams takes the table interleaved with FILLER beams (helpers/beamformer_model.py:
interleave_with_filler -- fPhase_rad = 40000, plainly slow): every second pair is slow, every run of the generator takes
coeff_slow for all its pairs, and beams 0, 2, 4, ... are the beamformer's.  The whole 2 B tensor is asserted within 1 ULP of
the oracle, the only inequality in this file; how many of its words differ from the oracle at all is recorded per test
(expected: none -- coeff_slow is the verifier's definition).  Where every pair of a table is slow the plain generator and
the filler route must return the same bits: test_a_table_that_is_slow_throughout asserts it.  The same route with fillers
of the full-degree fast class gives the bits of a fast block of the fused kernel that ONE full-degree pair has put on the
full-degree polynomials (test_fused_kernel_class_changing_during_a_call).

Every case states its class pattern on the CPU before its beamformer call (helpers/slow_tables.py: classes_of -- no pair at
any time within 0.5 % of a class boundary -- and at least one slow pair per call, resp. per block), with the weights taken
into account: a pair of weight 0 is made from zero terms, whatever its delay values are.  Every assertion on beam values is
equality of the uint32 views, the canary behind the output intact, values finite unless the model says NaN (then NaN of
any payload).  Still bound-tested only: the fp32 chain form (math_mode 8)."""
import numpy as np
import pytest

from helpers import slow_tables
from helpers.bacc_case import ACC_SHAPES, T_COEFF
from helpers.beamformer_model import (FAST_HIGH, FAST_LOW, FILLER_PHASE, FILLER_PHASE_HIGH, SLOW, acc_model, acc_model_nonfinite,
                                      first_difference_or_nan, flagged_table, fused_model, interleave_with_filler, normalise,
                                      real_beams, weighted_coefficients, zero_weight_coefficients)
from test_gpu_beam_complex import Complex, check_model
from test_gpu_beamformer_exact import (DT_COEFF, FUSED_EXACT_SHAPES, FUSED_PASS_SHAPES, PAIRS_PER_SLICE, Exact, prove_fused_passes,
                                       weights_for)
from test_gpu_class_replay import CHAIN_DEEP, STAGED_DEEP

pytestmark = pytest.mark.gpu


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class SlowExact(Exact):
    """Exact plus the second coefficient source: a generator context of 2 B beams whose table is this case's, interleaved
    with filler beams."""

    def __init__(self, gpu, oracle, A, B, C, nt, table, record_property=None, **kw):
        self.gen2 = None
        self.words_checked = self.words_differing = 0
        self.record_property = record_property
        super().__init__(gpu, oracle, A, B, C, nt, table=table, **kw)
        self.bp2 = self.bp.with_beams(2 * B)
        self.op2 = oracle.params_from(self.bp2)

    def _table_ab(self):
        super()._table_ab()
        self.filler = None  # the class of the fillers in gen2's table: none uploaded

    @staticmethod
    def _not_finite(table):
        return ~np.logical_and.reduce([np.isfinite(table[name]) for name in table.dtype.names])

    def filled_bits(self, dts, filler):
        """fp32 [len(dts)][C][A][B][2] from the generator context of 2 B beams, every second beam a filler of the class
        ``filler``; its whole output (fillers included) is asserted within 1 ULP of the oracle."""
        from dc_sand_amd.generator import SteeringCoefficientGenerator

        dts = np.ascontiguousarray(np.atleast_1d(np.asarray(dts, dtype=np.float32)))
        if self.gen2 is None:
            self.gen2 = SteeringCoefficientGenerator(self.bp2)
        if self.filler != filler:
            self.table2 = interleave_with_filler(self.table_ab, self.A, self.B, {SLOW: FILLER_PHASE, FAST_HIGH: FILLER_PHASE_HIGH}[filler])
            self.gen2.upload_delays(self.table2)
            self.filler = filler
        cls = slow_tables.classes_of(self.table2, dts, self.C).reshape(dts.size, self.A, 2 * self.B)
        assert np.all(cls[:, :, 1::2] == filler) and np.all(cls <= filler)  # every second pair, at every time; none higher
        coef2, res = self.generated_bits(self.gen2, self.op2, self.table2, 2 * self.B, dts, not_finite=self._not_finite(self.table2))
        if filler == SLOW:  # expected to differ nowhere: coeff_slow is the verifier's definition (the fast path: within 1 ULP)
            self.words_checked += coef2.size
            self.words_differing += coef2.size - res["hist"][0]
        return real_beams(coef2)

    def slow_coefficient_bits(self, dts):
        """What coeff_slow gives for every pair of the table (fillers that are plainly slow)."""
        return self.filled_bits(dts, SLOW)

    def full_degree_coefficient_bits(self, dts):
        """What the full-degree fast path gives for every pair of a table without a slow pair (fillers of that class): a
        beamformer makes a whole table (block) so when one of its pairs is of that class, while the generator -- and with it
        coefficient_bits -- keeps the low-degree polynomials for the runs without such a pair, 1 ULP away now and then."""
        return self.filled_bits(dts, FAST_HIGH)

    def plain_generator_bits(self, dts):
        """coefficient_bits without its fast precondition: the generator on the table as it is."""
        dts = np.ascontiguousarray(np.atleast_1d(np.asarray(dts, dtype=np.float32)))
        return self.generated_bits(self.gen, self.op, self.table_ab, self.B, dts, not_finite=self._not_finite(self.table_ab))[0]

    def classes(self, w, dts):
        """The classes [len(dts)][B * A] a call with the weights ``w`` sees; no pair unclear."""
        return slow_tables.classes_of(self.table if w is None else flagged_table(self.table, w), dts, self.C)

    def same_bits(self, got, exp, what, finite=True):
        assert not finite or np.all(np.isfinite(exp)), what
        diff = first_difference_or_nan(got, exp)
        assert diff is None, f"{what} at (A, B, C, nt) = {(self.A, self.B, self.C, self.nt)}: {diff}"

    def weighted(self, coef, w):
        """(w' = RN32(ghat * w), s_b); the coefficient of a pair of weight 0 is made from zero terms."""
        s, gh = normalise(w)
        with np.errstate(invalid="ignore"):
            return weighted_coefficients(zero_weight_coefficients(coef, w), gh), s

    # ---- the int8 matrix-core form
    def check_acc_slow(self, weights=(None,), t_coeff=None, dt_coeff=None, finite=True, table_class=SLOW):
        """beamform_accumulated[_weighted] at one coefficient time; ``table_class``: the highest class among the pairs of
        every call's table, SLOW unless the case is about the full-degree fast class."""
        from dc_sand_amd.generator import delta_times

        by_index = dt_coeff is None
        dt = delta_times(self.bp, t_coeff, 1)[0] if by_index else np.float32(dt_coeff)
        kw = {"t_coeff": t_coeff} if by_index else {"dt_coeff": float(dt)}
        for w in weights:  # the condition, on the CPU: the table of every call holds a slow (full-degree) pair
            assert self.classes(w, dt).max() == table_class, "no pair of the class meant under these weights: change the inputs"
        coef = self.filled_bits(dt, table_class)[0]
        assert np.all(np.isfinite(coef)) == finite
        out = []
        for w in weights:
            if w is None:
                exp = acc_model_nonfinite(coef, self.ant)
            else:
                wc, s = self.weighted(coef, w)
                exp = acc_model_nonfinite(wc, self.ant, scale=s)
            got = self.call("acc", w, finite=finite, **kw)
            self.same_bits(got, exp, f"matrix-core form, slow class, {'weighted' if w is not None else 'unweighted'}, {kw}", finite)
            out.append(got)
        return out

    # ---- the fused per-sample kernel
    def check_fused_slow(self, weights=(None,), t0=0, dts=None, block_classes=None, finite=True):
        """generate_and_beamform[_weighted][_dt].  ``block_classes``: the class every 16-sample block must be in (default:
        all slow); a block that is not slow takes its bits from coefficient_bits, a slow one from slow_coefficient_bits."""
        from dc_sand_amd.generator import delta_times

        by_index = dts is None
        dts = delta_times(self.bp, t0, self.nt) if by_index else np.ascontiguousarray(dts, dtype=np.float32)
        assert dts.size == self.nt
        kw = {"t0": t0} if by_index else {"dt": dts}
        pattern = np.full(self.nt // 16, SLOW) if block_classes is None else np.asarray(block_classes)
        for w in weights:
            assert np.array_equal(slow_tables.block_classes(self.classes(w, dts)), pattern), "the blocks' classes are not what the case means"
        got = [self.call("fused", w, finite=finite, **kw) for w in weights]
        # slices of whole blocks of one kind, no more than PAIRS_PER_SLICE generated pairs (the fillers count) at a time
        step = max(16, PAIRS_PER_SLICE // (self.C * self.A * 2 * self.B) // 16 * 16)
        source = {SLOW: self.slow_coefficient_bits, FAST_HIGH: self.full_degree_coefficient_bits, FAST_LOW: self.coefficient_bits}
        lo = 0
        while lo < self.nt:
            cls = pattern[lo // 16]
            hi = lo + 16
            while hi < min(lo + step, self.nt) and pattern[hi // 16] == cls:
                hi += 16
            coef = source[cls](dts[lo:hi])
            x = self.ant[:, lo // 16:hi // 16]
            for w, g in zip(weights, got):
                with np.errstate(invalid="ignore"):
                    if w is None:
                        exp = fused_model(np.ascontiguousarray(coef), x)
                    else:
                        s, gh = normalise(w)
                        exp = fused_model(zero_weight_coefficients(coef, w), x, ghat=gh, scale=s)
                self.same_bits(np.ascontiguousarray(g[:, lo // 16:hi // 16]), exp,
                               f"fused kernel, blocks {lo // 16}..{hi // 16 - 1} of class {cls}, "
                               f"{'weighted' if w is not None else 'unweighted'}, {'t0 = %d' % t0 if by_index else 'dt by value'}", finite)
            lo = hi
        return got

    def close(self):
        if self.record_property is not None:
            self.record_property("slow-path generator words that differ from the oracle (of those checked)",
                                 (self.words_differing, self.words_checked))
        print(f"slow-path generator words that differ from the oracle: {self.words_differing} of {self.words_checked}")
        if self.gen2 is not None:
            self.gen2.close()
        super().close()


def slow_weights_for(A, B, seed):
    """weights_for (a zero beam, antenna A // 2 flagged in every beam, a -0.0), except that the slow pair of
    slow_tables.one_slow_pair / crossing, (beam B // 2, antenna A // 2), keeps a weight: flagged, it would be made from zero
    terms and the weighted call would see a table without a slow pair."""
    w = weights_for(A, B, seed)
    b, a = B // 2, A // 2
    if not w[b].any():  # the zero beam: let it be the next one
        other = (b + 1) % B
        w[[b, other]] = w[[other, b]]
    if w[b, a] == 0:
        w[b, a] = np.float32(0.75)
    assert w[b, a] != 0 and (A == 1 or np.all(np.delete(w[:, a], b) == 0)) and (B == 1 or np.any(~w.any(axis=1)))
    return w


# ---- a. the int8 matrix-core form, every kernel family: all of ACC_SHAPES (1 / 2 / 4 beam tiles per workgroup and partial
# tiles, staged at 1 .. 64 antennas, kChain at 65 .. 256 with whole and partial chunks and waves without a chunk), the table
# with ONE slow pair
@pytest.mark.parametrize("A,B,C,nt", ACC_SHAPES)
def test_matrix_core_form_in_the_slow_class_bit_for_bit(gpu, oracle, record_property, A, B, C, nt):
    """Unweighted and weighted; by time index and by fDeltaTime value in turn."""
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_slow_pair(A, B), record_property)
    w = slow_weights_for(A, B, A + 7 * B)
    if ACC_SHAPES.index((A, B, C, nt)) % 2 == 0:
        c.check_acc_slow(weights=(None, w), t_coeff=T_COEFF)
    else:
        c.check_acc_slow(weights=(None, w), dt_coeff=DT_COEFF)
    c.close()


@pytest.mark.parametrize("A,B,C,nt", [(37, 21, 3, 48), (200, 20, 2, 32)])
def test_the_cases_tell_the_slow_path_from_the_fast_one(gpu, oracle, record_property, A, B, C, nt):
    """A condition on the inputs, not on the kernels: for the table with one slow pair the generator on the table as it is
    (the fast path for every run of pairs without the slow one) and the filler route differ in some words, and both
    models give other beams from the one than from the other -- a beamformer that took the fast path, or that made only
    the slow pair's neighbourhood with coeff_slow, would fail the equality of the tests above."""
    from dc_sand_amd.generator import delta_times

    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_slow_pair(A, B), record_property)
    dts = delta_times(c.bp, 0, 16)
    fast, slow = np.ascontiguousarray(c.plain_generator_bits(dts)), np.ascontiguousarray(c.slow_coefficient_bits(dts))
    differing = int(np.sum(fast.view(np.uint32) != slow.view(np.uint32)))
    record_property("coefficient words that differ between the two paths (of those compared)", (differing, fast.size))
    assert differing > 0 and np.max(np.abs(fast - slow)) < 2e-7  # 1 ULP of a number below 1 at the most
    assert not bits_equal(acc_model(fast[0], c.ant), acc_model(slow[0], c.ant))
    assert not bits_equal(fused_model(fast, c.ant[:, :1]), fused_model(slow, c.ant[:, :1]))
    c.close()


# ---- b. several sample blocks per wave, as tests/test_gpu_class_replay.py picks the shapes: kStaged and kChain
@pytest.mark.parametrize("A,B,C,nt,depth", [STAGED_DEEP, CHAIN_DEEP])
def test_matrix_core_form_in_the_slow_class_with_several_blocks_per_wave(gpu, oracle, record_property, A, B, C, nt, depth):
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_slow_pair(A, B), record_property)
    w = slow_weights_for(A, B, A + 7 * B)
    c.check_acc_slow(weights=(None, w), t_coeff=T_COEFF)
    for weighted in (False, True):
        record_property(f"{'weighted' if weighted else 'unweighted'}: gridDim.x, blockDim.x, blocks proven on some wave",
                        c.prove_depth(depth, lambda s: c.enqueue_floats(weighted, s)))
    c.close()


# ---- c. a table that is slow throughout: the anchor of the filler route
@pytest.mark.parametrize("A,B,C,nt", [(37, 21, 3, 48), (200, 20, 2, 32)])
def test_a_table_that_is_slow_throughout(gpu, oracle, record_property, A, B, C, nt):
    """Every pair's fPhase_rad in +-[40000, 100000], one rate term below the constant divide's range, one rate of 1e-2.
    Every run of the plain generator is slow here, so it and the filler route must return the same bits for the real
    beams; then both beamformers against the model."""
    from dc_sand_amd.generator import delta_times

    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.all_slow(A, B), record_property)
    dts = np.concatenate([delta_times(c.bp, 0, nt), delta_times(c.bp, T_COEFF, 1), [DT_COEFF]]).astype(np.float32)
    assert np.all(c.classes(None, dts) == SLOW)
    assert bits_equal(c.plain_generator_bits(dts), c.slow_coefficient_bits(dts)), "the filler route and the plain generator differ"
    w = slow_weights_for(A, B, A + 7 * B)
    c.check_acc_slow(weights=(None, w), t_coeff=T_COEFF)
    c.check_acc_slow(weights=(None, w), dt_coeff=DT_COEFF)
    c.check_fused_slow(weights=(None, w), t0=0)
    c.close()


# ---- d. the fused per-sample kernel: the shapes of its fast-class twin (three LDS chunks of antennas; (4, 512, 5, 512), 4
# channels per pass with one live in the last; (65, 512, 3, 512), three launches; every launch of the others, and of
# that one, takes ONE channel per pass), the table with ONE slow pair
@pytest.mark.parametrize("A,B,C,nt", FUSED_EXACT_SHAPES)
def test_fused_kernel_in_the_slow_class_bit_for_bit(gpu, oracle, record_property, A, B, C, nt):
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_slow_pair(A, B), record_property)
    c.check_fused_slow(weights=(None, slow_weights_for(A, B, A + 7 * B)), t0=0)
    c.close()


# ---- d''. the slow branch ("channel outermost and unrolled") at 4 and 2 channels per pass, the form read from the launch
# (test_gpu_beamformer_exact.py: FUSED_PASS_SHAPES): 4 with three live channels in the last pass and with two beam tiles;
# 2 in a workgroup of two passes (65 antennas) and in one of a single pass
@pytest.mark.parametrize("A,B,C,nt,passes", [FUSED_PASS_SHAPES[i] for i in (0, 1, 3, 5)])
def test_fused_kernel_passes_of_two_and_four_channels_in_the_slow_class(gpu, oracle, record_property, A, B, C, nt, passes):
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_slow_pair(A, B), record_property)
    c.check_fused_slow(weights=(None, slow_weights_for(A, B, A + 7 * B)), t0=0)
    prove_fused_passes(c, record_property, passes)
    c.close()


def test_fused_kernel_class_changing_during_a_call(gpu, oracle, record_property):
    """One pair's phase grows by 3e4 rad per unit of time; the times by value.  Block 0 (times 0.1 .. 0.9) is fast, full
    degree; the bound crosses 32000 inside block 1 (between 1.05 and 1.1), which therefore runs slow as a whole; block 2
    is slow throughout.  Blocks 1 and 2 are held to slow_coefficient_bits.  Block 0 is held to
    full_degree_coefficient_bits, not to coefficient_bits: the one full-degree pair puts the whole block on the
    full-degree polynomials, while the generator keeps the low-degree ones for the waves without that pair (91 of the
    block's 2016 words are 1 ULP apart between the two)."""
    A, B, C, nt = 37, 21, 3, 48
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.crossing(A, B), record_property)
    c.check_fused_slow(weights=(None, slow_weights_for(A, B, 3 * A + B)), dts=slow_tables.crossing_times(),
                       block_classes=slow_tables.CROSSING_BLOCK_CLASSES)
    c.close()


@pytest.mark.parametrize("A,B,C,nt,passes", [(5, 21, 1366, 48, (4, 4, 2)), (5, 21, 683, 48, (2, 2, 1))])
def test_fused_kernel_class_changing_during_a_call_with_several_channels_per_pass(gpu, oracle, record_property, A, B, C, nt, passes):
    """The same three blocks (full degree, slow, slow) where a pass takes 4 and 2 channels: 2052 workgroups of two beam
    tiles, the form read from the launch; two live channels in the last pass of 4, one in the last pass of 2."""
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.crossing(A, B), record_property)
    dts = slow_tables.crossing_times()
    c.check_fused_slow(weights=(None, slow_weights_for(A, B, 3 * A + B)), dts=dts, block_classes=slow_tables.CROSSING_BLOCK_CLASSES)
    prove_fused_passes(c, record_property, passes, dts=dts)
    c.close()


# ---- d'. one pair of the full-degree fast class: no slow path, but the same difference between the beamformers (whole
# table, whole block) and the generator (per run of pairs), which the fast-class exact tests -- rand_table and constant
# tables, every pair of one class -- never meet
@pytest.mark.parametrize("A,B,C,nt", [(64, 16, 2, 32), (130, 20, 2, 32)])
def test_one_full_degree_pair_puts_the_whole_table_on_the_full_degree_polynomials(gpu, oracle, record_property, A, B, C, nt):
    c = SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_full_degree_pair(A, B), record_property)
    w = slow_weights_for(A, B, A + 7 * B)
    c.check_acc_slow(weights=(None, w), t_coeff=T_COEFF, table_class=FAST_HIGH)
    c.check_fused_slow(weights=(None, w), t0=0, block_classes=[FAST_HIGH] * (nt // 16))
    c.close()


# ---- e. the complex product: its third operand (the digits of the negated sine) hangs off the same rolled loop
@pytest.mark.parametrize("A,B,C,nt", [(37, 21, 3, 48), (200, 20, 2, 32)])
def test_complex_product_in_the_slow_class_bit_for_bit(gpu, oracle, record_property, A, B, C, nt):
    from dc_sand_amd.generator import delta_times

    x = Complex(SlowExact(gpu, oracle, A, B, C, nt, slow_tables.one_slow_pair(A, B), record_property))
    c = x.c
    dt = delta_times(c.bp, T_COEFF, 1)[0]
    w = slow_weights_for(A, B, A + 7 * B)
    assert np.any(c.classes(None, dt) == SLOW) and np.any(c.classes(w, dt) == SLOW)
    coef = np.ascontiguousarray(c.slow_coefficient_bits(dt)[0])
    for conj in (False, True):
        v = check_model(x, coef, conj, what="slow class, unweighted")
        assert np.all(np.isfinite(v))
        v = check_model(x, coef, conj, w=w, what="slow class, weighted")
        assert np.all(np.isfinite(v))
    x.c.close()


# ---- f. delay values that are not finite
def non_finite_weights(A, B, flagged):
    """Seeded weights without a zero beam, antenna ``flagged`` at weight 0 in every beam."""
    from helpers.bacc_case import random_weights

    w = random_weights(np.random.default_rng(A + 3 * B), B, A, zero_beam=False)
    w[:, flagged] = 0.0
    return w


def check_nan_beams(got, nan_beams, what):
    B = got.shape[2]
    for b in range(B):
        if b in nan_beams:
            assert np.all(np.isnan(got[:, :, b])), (what, "beam", b, "must be NaN in both planes, every channel and block")
        else:
            assert np.all(np.isfinite(got[:, :, b])), (what, "beam", b, "must be finite")


@pytest.mark.parametrize("kind,A,B,C,nt", [("acc", 37, 21, 2, 32), ("acc", 130, 20, 1, 32), ("fused", 37, 5, 2, 16)])
def test_delay_values_that_are_not_finite(gpu, oracle, record_property, kind, A, B, C, nt):
    """fDelayRate_sps = inf in one beam, fDelay_s = NaN in another.  Unweighted, and with weights that leave both pairs a
    weight: exactly those two beams are NaN in both planes, in every channel and block, and every other beam is the
    model's bits.  With the NaN pair's antenna flagged (weight 0) include/dcs_beam_weights.h says what happens: the antenna
    "contributes nothing, even where its delay values are not finite (its coefficient is made from zero terms)" -- so that
    beam is finite and the model's bits like the others, and the beam of the infinite rate alone is NaN."""
    table, (inf_beam, nan_beam), nan_antenna = slow_tables.non_finite(A, B)
    c = SlowExact(gpu, oracle, A, B, C, nt, table, record_property)
    kept = non_finite_weights(A, B, flagged=0)
    flagged = non_finite_weights(A, B, flagged=nan_antenna)
    assert nan_antenna != 0 and kept[inf_beam, min(3, A - 1)] != 0 and kept[nan_beam, nan_antenna] != 0 and flagged[inf_beam, min(3, A - 1)] != 0
    weights = (None, kept, flagged)
    if kind == "acc":
        got = c.check_acc_slow(weights=weights, t_coeff=T_COEFF, finite=False)
    else:
        got = c.check_fused_slow(weights=weights, t0=0, finite=False)
    check_nan_beams(got[0], (inf_beam, nan_beam), "unweighted")
    check_nan_beams(got[1], (inf_beam, nan_beam), "weighted, both pairs with a weight")
    check_nan_beams(got[2], (inf_beam,), "weighted, the NaN pair's antenna flagged")
    c.close()
