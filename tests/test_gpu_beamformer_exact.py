"""Both beamformers held to their stated arithmetic, bit for bit (include/dcs_beamformer.h, include/dcs_beam_weights.h).

The chain has no unanchored link: the coefficient bits come from the GPU GENERATOR (never from the kernel under test) --
the beamformer's table transposed to the generator's [a * B + b] order in a second context of the same parameters, the very
fDeltaTime values of the beamformer call -- and that tensor is asserted within 1 ULP of the oracle in the same test (the
only inequality in this file).  The beamformers make their coefficients with the generator's own dcs_pair_terms /
coeff_fast, whose fast forms are proven bit-identical to each other (test_arithmetic_forms_agree_and_class_boundaries), so
these are the exact bits a call used, and everything after the coefficient is integer or single-operation fp32 arithmetic
that tests/helpers/beamformer_model.py restates in numpy (anchored, in turn, by tests/test_beamformer_model.py).

Precondition, asserted on the CPU for every case: all pairs in the fast classes (all_pairs_fast).  With a slow-class pair
the beamformers switch the whole table (resp. 16-sample block) to the slow path while the generator does so per wave.

Every assertion on beam values is equality of the uint32 views, the 64-byte canary behind the output untouched, all
values finite.  The slow class and non-finite delay values are held the same way, bit for bit, in
tests/test_gpu_beamformer_exact_slow.py (the slow path's coefficient bits come from the same generator, made to take
coeff_slow for every pair).  Not covered by either file (its bound tests stay): the fp32 chain form (math_mode 8: the
matrix instruction's internal order is not specified)."""
import numpy as np
import pytest

from conftest import rand_table
from helpers import bacc_cases as bc
from helpers.bacc_case import DEEP_SHAPES, FUSED_SHAPES, T_COEFF, Case, random_weights
from helpers.beamformer_model import (acc_model, all_pairs_fast, first_difference, fused_model, normalise, weighted_coefficients)

pytestmark = pytest.mark.gpu

DT_COEFF = np.float32(0.3710937)  # an fDeltaTime off the time-index grid, for the calls by value
PAIRS_PER_SLICE = 24 << 20  # coefficient pairs generated, checked and modelled at a time (192 MiB of fp32 pairs)


class Exact(Case):
    """A Case (context, samples, output buffer with a canary, weights buffer) plus the generator context that supplies the
    coefficient bits."""

    def __init__(self, gpu, oracle, A, B, C, nt, seed=0, table=None, ant=None):
        from dc_sand_amd.generator import SteeringCoefficientGenerator

        super().__init__(gpu, oracle, A, B, C, nt, seed=seed, table=table)
        if ant is not None:
            self.set_ant(np.ascontiguousarray(ant, dtype=np.int8))
        self.gen = SteeringCoefficientGenerator(self.bp)
        self._table_ab()

    def _table_ab(self):
        self.table_ab = np.ascontiguousarray(self.table.reshape(self.B, self.A).T).ravel()  # the generator's [a * B + b]
        self.gen.upload_delays(self.table_ab)

    def set_table(self, table):
        super().set_table(table)
        self._table_ab()

    def coefficient_bits(self, dts):
        """fp32 [len(dts)][C][A][B][2] from the GPU generator, asserted within 1 ULP of the oracle."""
        dts = np.ascontiguousarray(np.atleast_1d(np.asarray(dts, dtype=np.float32)))
        assert all_pairs_fast(self.table_ab, dts, self.C, self.bp.SAMPLING_PERIOD), "a pair outside the fast classes: change the inputs"
        return self.generated_bits(self.gen, self.op, self.table_ab, self.B, dts)[0]

    def generated_bits(self, gen, op, table_ab, nr_beams, dts, not_finite=None):
        """(fp32 [len(dts)][C][A][nr_beams][2] from the generator context ``gen``, whose table is ``table_ab``, the oracle's
        comparison of it): the canary behind the tensor intact and every word within 1 ULP of the oracle.  ``not_finite``:
        a mask over the pairs of table_ab whose delay values are not finite -- their words must all be NaN, and the
        oracle compares the rest (those pairs as the zero entry's (1, 0))."""
        gpu = self.gpu
        nbytes = gen.output_bytes(nt=dts.size)
        buf = gpu.mem_alloc(nbytes + 64)
        gpu.memset(buf, 0xFF, nbytes + 64)
        gen.generate_dt(buf, nbytes, dts)
        host = np.empty(nbytes + 64, dtype=np.uint8)
        gpu.memcpy_dtoh(host, buf)
        buf.free()
        assert np.all(host[nbytes:] == 0xFF)
        coef = host[:nbytes].view(np.float32).reshape(dts.size, self.C, self.A, nr_beams, 2)
        seen, table = coef, table_ab
        if not_finite is not None and not_finite.any():
            mask = not_finite.reshape(self.A, nr_beams)
            assert np.all(np.isnan(coef[:, :, mask]))
            seen, table = coef.copy(), table_ab.copy()
            seen[:, :, mask] = (np.float32(1), np.float32(0))
            table[not_finite] = np.zeros((), dtype=table.dtype)
        res = self.oracle.compare_generated(op, table, dts, 0, self.C, seen, nthreads=8)
        assert res["max_ulp"] <= 1 and res["first_over_1ulp"] == -1 and sum(res["hist"]) == coef.size, res
        return coef, res

    def call(self, kind, w=None, finite=True, **kw):
        """One beamformer call into the 0xFF-filled buffer; `kw` picks the time: acc t_coeff= / dt_coeff=, fused t0= / dt=.
        ``finite=False`` only where the delay table holds a value that is not finite."""
        gpu, g = self.gpu, self.g
        self.refill(self.d_beams)
        if w is not None:
            gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
        if kind == "acc" and w is None:
            g.beamform_accumulated(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, self.nt, **kw)
        elif kind == "acc":
            g.beamform_accumulated_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, self.nt, **kw)
        elif w is not None:
            g.generate_and_beamform_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, nt=self.nt, **kw)
        elif "dt" in kw:
            g.generate_and_beamform_dt(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, kw["dt"])
        else:
            g.generate_and_beamform(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, t0=kw["t0"], nt=self.nt)
        got = self.read_beams()  # asserts the canary
        assert not finite or np.all(np.isfinite(got)), (kind, kw)
        return got

    def same_bits(self, got, exp, what):
        diff = first_difference(got, exp)
        assert diff is None, f"{what} at (A, B, C, nt) = {(self.A, self.B, self.C, self.nt)}: {diff}"

    # ---- the int8 matrix-core form
    def check_acc(self, weights=(None,), t_coeff=None, dt_coeff=None):
        """beamform_accumulated[_weighted] at one coefficient time, unweighted (None) and / or with each [B][A] weights."""
        from dc_sand_amd.generator import delta_times

        by_index = dt_coeff is None
        dt = delta_times(self.bp, t_coeff, 1)[0] if by_index else np.float32(dt_coeff)
        kw = {"t_coeff": t_coeff} if by_index else {"dt_coeff": float(dt)}
        coef = self.coefficient_bits(dt)[0]
        for w in weights:
            if w is None:
                exp = acc_model(coef, self.ant)
            else:
                s, gh = normalise(w)
                exp = acc_model(weighted_coefficients(coef, gh), self.ant, scale=s)
            self.same_bits(self.call("acc", w, **kw), exp, f"matrix-core form, {'weighted' if w is not None else 'unweighted'}, {kw}")

    # ---- the fused per-sample kernel
    def check_fused(self, weights=(None,), t0=0, dts=None):
        """generate_and_beamform[_weighted][_dt] over nt time steps from time index t0, or at the fDeltaTime values dts."""
        from dc_sand_amd.generator import delta_times

        by_index = dts is None
        dts = delta_times(self.bp, t0, self.nt) if by_index else np.ascontiguousarray(dts, dtype=np.float32)
        assert dts.size == self.nt
        kw = {"t0": t0} if by_index else {"dt": dts}
        got = [self.call("fused", w, **kw) for w in weights]
        # the model in slices of whole 16-sample blocks, so that no more than PAIRS_PER_SLICE coefficients exist at a time
        step = max(16, PAIRS_PER_SLICE // (self.C * self.A * self.B) // 16 * 16)
        for lo in range(0, self.nt, step):
            hi = min(lo + step, self.nt)
            coef = self.coefficient_bits(dts[lo:hi])
            x = self.ant[:, lo // 16:hi // 16]
            for w, g in zip(weights, got):
                s, gh = (None, None) if w is None else normalise(w)
                exp = fused_model(coef, x, ghat=gh, scale=s)
                self.same_bits(np.ascontiguousarray(g[:, lo // 16:hi // 16]), exp,
                               f"fused kernel, {'weighted' if w is not None else 'unweighted'}, {'t0 = %d' % t0 if by_index else 'dt by value'}, "
                               f"blocks {lo // 16}..{hi // 16 - 1}")

    def close(self):
        self.gen.close()
        super().close()


def weights_for(A, B, seed):
    """random_weights (magnitudes 1e-3 .. 1e3, either sign) with a zero beam (where there are two) and a flagged antenna."""
    w = random_weights(np.random.default_rng(seed), B, A, zero_beam=B > 1)
    if A > 1:
        w[:, A // 2] = 0.0
        w[0, 0] = -0.0
    return w


# ---- a. the int8 matrix-core form.  All 35 shapes of ACC_SHAPES: 1 / 2 / 4 beam tiles per workgroup and partial tiles, the
# staged form at 1 .. 64 antennas, kChain at 65 .. 256 (whole and partial chunks, waves without a chunk), odd block counts,
# several workgroups per (channel, beam group), the shapes that leave the XCD-grouped numbering's identity tail,
# (64, 1024, 1, 32).  At these channel counts (64 at the most) the launcher splits the sample blocks until every wave has
# ONE: no wave sees a second block, a second pair or a second round.  DEEP_SHAPES, below, are the shapes that do.
@pytest.mark.parametrize("A,B,C,nt", bc.shapes_of(bc.EXACT + "test_matrix_core_form_is_the_fixed_point_model_bit_for_bit"))
def test_matrix_core_form_is_the_fixed_point_model_bit_for_bit(gpu, oracle, A, B, C, nt):
    """By time index (unweighted and weighted) and by fDeltaTime value (unweighted and weighted)."""
    c = Exact(gpu, oracle, A, B, C, nt)
    w = weights_for(A, B, A + 7 * B)
    c.check_acc(weights=(None, w), t_coeff=T_COEFF)
    c.check_acc(weights=(None, w), dt_coeff=DT_COEFF)
    c.close()


# ---- a'. the same form where a wave takes several sample blocks (helpers/bacc_cases.py: DEEP_SHAPES): the live second block
# of a pair, the later pairs (kStaged's LDS offsets of later blocks, kChain's stepping of its two sample buffers and the
# re-zeroed accumulators), waves of one workgroup with different block counts, the equal-shares split with several rounds
@pytest.mark.parametrize("A,B,C,nt,depth", bc.shapes_of(bc.EXACT + "test_matrix_core_form_with_several_blocks_per_wave_bit_for_bit", raw=True))
def test_matrix_core_form_with_several_blocks_per_wave_bit_for_bit(gpu, oracle, record_property, A, B, C, nt, depth):
    """Unweighted and weighted at one time form per shape (by index and by value in turn).  The launch itself, read from
    a captured graph, must prove `depth` blocks on some wave: 3 is a live second pair; and its grid, block and dynamic LDS
    bytes must be those of helpers/launch_forms.py: bacc_plan, whose census tests/test_launch_forms.py takes."""
    c = Exact(gpu, oracle, A, B, C, nt)
    w = weights_for(A, B, A + 7 * B)
    if DEEP_SHAPES.index((A, B, C, nt, depth)) % 2 == 0:
        c.check_acc(weights=(None, w), t_coeff=T_COEFF)
    else:
        c.check_acc(weights=(None, w), dt_coeff=DT_COEFF)
    for weighted in (False, True):
        record_property(f"{'weighted' if weighted else 'unweighted'}: gridDim.x, blockDim.x, blocks proven on some wave",
                        c.prove_depth(depth, lambda s: c.enqueue_floats(weighted, s), kind=bc.FW if weighted else bc.F))
    c.close()


# ---- b. the fused per-sample kernel.  FUSED_SHAPES plus: three LDS chunks of antennas with a partial last one;
# (4, 512, 5, 512), one launch of 4 channels per pass whose last pass has one live channel; (65, 512, 3, 512), whose 33 280
# pairs leave the terms table 252 time steps: THREE launches (240, 240 and 32 steps: the offsets tex0 and nt16_total, the
# staged fDeltaTime values), each with too few workgroups for more than ONE channel per pass.  Every other shape of this
# list is one launch of one channel per pass as well; FUSED_PASS_SHAPES, below, are the shapes of 2 and 4.
FUSED_EXACT_SHAPES = FUSED_SHAPES + [(300, 7, 3, 32), (4, 512, 5, 512), (65, 512, 3, 512)]


@pytest.mark.parametrize("A,B,C,nt", FUSED_EXACT_SHAPES)
def test_fused_kernel_is_the_verifiers_sum_bit_for_bit(gpu, oracle, A, B, C, nt):
    c = Exact(gpu, oracle, A, B, C, nt)
    c.check_fused(weights=(None, weights_for(A, B, A + 7 * B)), t0=0)
    c.close()


# ---- b'. the passes of 2 and 4 channels.  A workgroup walks cpb channels, CH at a time: (A, B, C, nt, (cpb, CH, live channels
# in the last pass of the last workgroup)), the triple as Case.prove_passes reads it from the launch.  Each shape launches
# 2048 workgroups, the fewest at which the launcher keeps the form, with few beams (the dead lanes of a 16-beam tile cost
# the model nothing) and 256 time steps, the most a captured call takes.
#   CH = 4: three live channels in the last pass; two beam tiles with a ragged second and two live; 64 antennas, the last
#           count with 4 channels per pass (32 KiB of LDS), and one live
#   CH = 2 of cpb = 4 (a workgroup makes TWO passes, the last workgroup a whole and a partial one): 65 antennas, the first
#           count with 2; 129, across two LDS chunks of antennas, the second holding one antenna
#   CH = 2 of cpb = 2: 5 antennas; 64 (where cpb = 4 would have meant CH = 4); 130, two LDS chunks
FUSED_PASS_SHAPES = [(5, 3, 511, 256, (4, 4, 3)), (7, 20, 254, 256, (4, 4, 2)), (64, 3, 509, 256, (4, 4, 1)),
                     (65, 3, 511, 256, (4, 2, 1)), (129, 2, 511, 256, (4, 2, 1)),
                     (5, 3, 255, 256, (2, 2, 1)), (64, 3, 255, 256, (2, 2, 1)), (130, 3, 255, 256, (2, 2, 1))]


def prove_fused_passes(c, record_property, passes, dts=None):
    """The form of the unweighted and of the weighted call, read from a captured launch (nothing runs), asserted to be
    ``passes`` and recorded.  Behind the calls themselves: a first call allocates, and d_w holds the weights."""
    for weighted in (False, True):
        record_property(f"{'weighted' if weighted else 'unweighted'}{'' if dts is None else ', dt by value'}: "
                        "channels per workgroup, channels per pass, live channels in the last pass",
                        c.prove_passes(passes, lambda s: c.enqueue_fused(weighted, s, dts=dts)))


@pytest.mark.parametrize("A,B,C,nt,passes", FUSED_PASS_SHAPES)
def test_fused_kernel_passes_of_two_and_four_channels_bit_for_bit(gpu, oracle, record_property, A, B, C, nt, passes):
    c = Exact(gpu, oracle, A, B, C, nt)
    c.check_fused(weights=(None, weights_for(A, B, A + 7 * B)), t0=0)
    prove_fused_passes(c, record_property, passes)
    c.close()


@pytest.mark.parametrize("A,B,C,nt,passes", [FUSED_PASS_SHAPES[3], FUSED_PASS_SHAPES[0]])
def test_fused_kernel_passes_of_two_and_four_channels_times_by_value(gpu, oracle, record_property, A, B, C, nt, passes):
    """Off the time-index grid and descending, as test_fused_kernel_time_offset_and_times_by_value makes them."""
    c = Exact(gpu, oracle, A, B, C, nt)
    dts = np.sort(np.random.default_rng(A).uniform(0.0, 1.5, nt)).astype(np.float32)[::-1]
    c.check_fused(weights=(None, weights_for(A, B, 3 * A + B)), dts=dts)
    prove_fused_passes(c, record_property, passes, dts=dts)
    c.close()


@pytest.mark.parametrize("A,B,C,nt", [(37, 21, 3, 48), (130, 3, 4, 32)])
def test_fused_kernel_time_offset_and_times_by_value(gpu, oracle, A, B, C, nt):
    c = Exact(gpu, oracle, A, B, C, nt)
    w = weights_for(A, B, 3 * A + B)
    c.check_fused(weights=(None, w), t0=32)
    dts = np.sort(np.random.default_rng(A).uniform(0.0, 1.5, nt)).astype(np.float32)[::-1]  # off the grid, descending
    c.check_fused(weights=(None, w), dts=dts)
    c.close()


def test_fused_kernel_more_time_steps_than_ride_in_the_kernel_arguments(gpu, oracle):
    """288 > 256 time steps: the fDeltaTime values are staged through pinned memory."""
    A, B, C, nt = 20, 18, 3, 288
    c = Exact(gpu, oracle, A, B, C, nt)
    w = weights_for(A, B, 11)
    c.check_fused(weights=(None, w), t0=16)
    c.check_fused(weights=(None, w), dts=np.linspace(0.0, 0.9, nt).astype(np.float32))
    c.close()


# ---- d. structured inputs
def constant_table(n, phase):
    from oracle.bf_oracle import delay_vals_dtype

    t = np.zeros(n, dtype=delay_vals_dtype)
    t["fPhase_rad"] = np.float32(phase)
    return t


def full_scale_samples(pattern, C, nt, A):
    x = np.empty((C, nt // 16, A, 16, 2), dtype=np.int8)
    if pattern == "alternating":  # by antenna
        x[:] = np.where(np.arange(A) % 2 == 0, -128, 127).astype(np.int8)[None, None, :, None, None]
    else:
        x[:] = pattern
    return x


@pytest.mark.parametrize("kind,A,B,C,nt", bc.shapes_of(bc.EXACT + "test_full_scale_samples_against_unit_coefficients", raw=True))
def test_full_scale_samples_against_unit_coefficients(gpu, oracle, kind, A, B, C, nt):
    """Samples all -128, all 127 and alternating by antenna, against the coefficients of a zero table (cos = 1, sin = 0)
    and of fPhase_rad = fp32(pi) and fp32(pi / 2) (cos = -1, sin = 1: digits +-127, 127, 127): the largest integer sums the
    design allows, |s| = 128 * 128 * A for the low digits' -128 (2^22 at 256 antennas), and, in the fused kernel, the longest
    runs of equal-signed products."""
    c = Exact(gpu, oracle, A, B, C, nt)
    w = weights_for(A, B, A + B)
    for phase in (0.0, np.float32(np.pi), np.float32(np.pi / 2)):
        c.set_table(constant_table(A * B, phase))
        for pattern in (-128, 127, "alternating"):
            c.set_ant(full_scale_samples(pattern, C, nt, A))
            if kind == "acc":
                c.check_acc(weights=(None, w) if pattern == -128 else (None,), t_coeff=T_COEFF)
            else:
                c.check_fused(weights=(None, w) if pattern == -128 else (None,), t0=0)
    # ... and against the seeded random table (digits of every kind, -128 among the low ones)
    c.set_table(rand_table(A * B, seed=A + B))
    for pattern in (-128, "alternating"):
        c.set_ant(full_scale_samples(pattern, C, nt, A))
        if kind == "acc":
            c.check_acc(t_coeff=T_COEFF)
        else:
            c.check_fused(t0=0)
    c.close()


def one_hot_samples(C, A, value):
    """nt = 16 * A: block k, sample k % 16 carries `value` in antenna k (re) and in antenna A - 1 - k (im), nothing else."""
    x = np.zeros((C, A, A, 16, 2), dtype=np.int8)
    k = np.arange(A)
    x[:, k, k, k % 16, 0] = value
    x[:, k, A - 1 - k, k % 16, 1] = value
    return x


@pytest.mark.parametrize("kind,A,B,C", bc.shapes_of(bc.EXACT + "test_one_antenna_at_a_time", raw=True))
def test_one_antenna_at_a_time(gpu, oracle, kind, A, B, C):
    """One-hot samples: every output column is one antenna's (quantised) coefficient, times 1 and times -128 -- a wrong
    digit of a single antenna, or a permutation error of the contraction index, shows in the column of that antenna:
    the block index the failure message reports IS the antenna (re plane; A - 1 - block for the im plane)."""
    nt = 16 * A
    c = Exact(gpu, oracle, A, B, C, nt)
    for value in (1, -128):
        c.set_ant(one_hot_samples(C, A, value))
        if kind == "acc":
            c.check_acc(weights=(None, weights_for(A, B, A)), t_coeff=T_COEFF)
        else:
            c.check_fused(weights=(None, weights_for(A, B, A)), t0=0)
    c.close()


def test_seeded_fuzz_bit_for_bit(gpu, oracle):
    """40 seeded cases in the style of test_beamform_accumulated_seeded_fuzz (antennas <= 256, beams <= 90, 1 .. 40 sample
    blocks, time by index or by value), weighted every third case, the fused kernel as well every fourth: equality."""
    rng = np.random.default_rng(20261016)
    for case in range(40):
        A = int(rng.choice([1, 3, 17, 63, 64, 65, 100, 128, 129, 191, 192, 200, 255, 256])) if case % 2 else int(rng.integers(1, 257))
        B = int(rng.integers(1, 91))
        C = int(rng.integers(1, 5))
        nblk = int(rng.integers(1, 41))
        if A * B * C * nblk > 600000:
            nblk = max(1, 600000 // (A * B * C))
        nt = 16 * nblk
        c = Exact(gpu, oracle, A, B, C, nt, table=rand_table(A * B, seed=5000 + case),
                  ant=rng.integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8))
        weights = (None, weights_for(A, B, case)) if case % 3 == 0 else (None,)
        if rng.integers(0, 2):
            c.check_acc(weights=weights, dt_coeff=np.float32(rng.uniform(0.0, 1.5)))
        else:
            c.check_acc(weights=weights, t_coeff=int(rng.integers(0, 2000)))
        if case % 4 == 0:
            c.set_ant(np.ascontiguousarray(c.ant[:, :min(nblk, 4)]))
            c.nt = 16 * min(nblk, 4)
            c.shape = (C, c.nt // 16, B, 16, 2)
            c.nbytes = int(np.prod(c.shape)) * 4
            c.check_fused(weights=weights, t0=16 * int(rng.integers(0, 100)))
        c.close()
