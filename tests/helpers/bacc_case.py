"""What the GPU tests of the beamformers share (tests/test_gpu_parity.py, test_gpu_parity_fused.py,
test_gpu_beam_weights.py, test_gpu_beamformer_exact.py, test_gpu_beam_quant.py, test_gpu_beam_power.py): one context with its
samples and output buffer, the proof of a launch's depth, and seeded random weights.  The shapes: helpers/bacc_cases.py."""
import numpy as np

from conftest import rand_table
from helpers.bacc_cases import ACC_SHAPES, DEEP_SHAPES, DEEPEST_SHAPES, MIN_DEPTH  # noqa: F401  (the tests take them from here)
from helpers.device_buffers import Context

# (the matrix-core beamformer's tables: helpers/bacc_cases.py, with the declared list of what each is run with)
FUSED_SHAPES = [(64, 16, 64, 256), (8, 4, 5, 16), (37, 21, 9, 48), (130, 3, 4, 16), (4, 40, 7, 32), (129, 2, 2, 16),
                (258, 2, 5, 16), (1, 1, 1, 16), (3, 17, 2, 32)]
T_COEFF = 9


def blocks_on_some_wave(B, C, nt, grid, block):
    """A lower bound, from the launch geometry alone, on the sample blocks the busiest wave of a matrix-core beamformer
    launch works on.  A wave (64 lanes) works on one 16-beam tile and whole 16-sample blocks, so the launch's
    C * ceil(B / 16) * (nt / 16) (tile, block) units are spread over gridDim.x * blockDim.x / 64 waves: some wave has at
    least the quotient, rounded up.  Nothing of the launcher's arithmetic is restated: if it comes to give these shapes one
    block per wave again, the tests that assert this number fail instead of testing nothing."""
    assert grid[1] == grid[2] == 1 and block[1] == block[2] == 1 and block[0] % 64 == 0, (grid, block)
    waves = grid[0] * (block[0] // 64)
    units = C * -(-B // 16) * (nt // 16)
    return -(-units // waves)


def plan_of(shape, kind):
    """helpers/launch_forms.py: bacc_plan of (A, B, C, nt) for a call (output kind, weighted, math_mode) of helpers/bacc_cases.py."""
    from helpers import launch_forms as lf
    from helpers.bacc_cases import KINDS

    name, weighted, math_mode = kind
    quant, power, complex_ = KINDS[name]
    return lf.bacc_plan(*shape, fp32_chain=bool(math_mode & 8), weighted=weighted, quant=quant, power=power, complex_=complex_)


def passes_of_fused_launch(A, B, C, nt16, grid_x, shared_bytes):
    """(channels per workgroup, channels per pass CH, live channels in the last pass of the last workgroup) of ONE launch of
    the fused per-sample beamformer over nt16 sample blocks, from its geometry alone.  The kernel stages CH channels of
    min(A, 128) antennas, 16 samples and (re, im) as fp32, so its dynamic LDS is CH * min(A, 128) * 128 bytes; a workgroup
    takes one 16-beam tile, one sample block and one group of channels, so gridDim.x = ceil(B / 16) * nt16 * n_cblocks with
    n_cblocks = ceil(C / cpb).  Nothing of the launcher's decision is restated (which cpb it prefers, when it narrows the
    pass): if it comes to choose otherwise, the tests that assert this triple fail instead of testing nothing.  A geometry
    that is not this kernel's, or a shape at which two values of cpb give the same grid, is an AssertionError."""
    row = min(A, 128) * 128
    assert shared_bytes % row == 0 and shared_bytes // row in (1, 2, 4), \
        f"{shared_bytes} bytes of LDS are not 1, 2 or 4 channels of {row} bytes"
    ch = shared_bytes // row
    per_cblock = -(-B // 16) * nt16
    assert grid_x % per_cblock == 0, f"{grid_x} workgroups are no whole number of channel groups ({per_cblock} workgroups each)"
    n_cblocks = grid_x // per_cblock
    fits = [cpb for cpb in (1, 2, 4) if -(-C // cpb) == n_cblocks]
    assert len(fits) == 1, f"{n_cblocks} channel groups of {C} channels: channels per workgroup {fits or 'none'} of 1, 2, 4"
    cpb = fits[0]
    last = C - (n_cblocks - 1) * cpb  # channels of the last workgroup: 1 .. cpb
    live = last - (-(-last // ch) - 1) * ch
    return cpb, ch, live


class Case(Context):
    """One context, its samples and output buffer (0xFF with a 0xFF canary: unwritten floats read as NaN), and both
    beamformers with and without weights.  ``table`` and ``ant`` replace the seeded table [b*A + a] and samples;
    ``parameters`` are further fields of the context's BeamformerParameters."""

    def __init__(self, gpu, oracle, A, B, C, nt, seed=0, table=None, ant=None, **parameters):
        super().__init__(gpu, C, A, B, **{"NR_SAMPLES_PER_CHANNEL": nt, **parameters})
        self.oracle, self.nt = oracle, nt
        self.op = oracle.params_from(self.bp)
        self.table = rand_table(self.bp.n_pairs, seed=A + B + seed) if table is None else table  # [b*A + a]
        if ant is None:
            ant = np.random.default_rng(A + seed).integers(-128, 128, size=(C, nt // 16, A, 16, 2), dtype=np.int8)
        assert ant.shape == (C, nt // 16, A, 16, 2) and ant.dtype == np.int8
        self.ant = ant
        self.g.upload_delays(self.table)
        self.d_ant = self.upload(self.ant)
        self.shape = (C, nt // 16, B, 16, 2)
        self.nbytes = int(np.prod(self.shape)) * 4
        self.d_beams = self.out(self.nbytes, 0xFF, 0xFF)
        self.d_w = self.alloc(B * A * 4)

    def set_ant(self, ant):
        self.ant = ant
        self.gpu.memcpy_htod(self.d_ant, ant)

    def set_table(self, table):
        self.table = table
        self.g.upload_delays(table)

    def run(self, kind, w=None, stream=None):
        """kind 'acc' / 'fused'; w: None (unweighted) or a [B][A] array (copied to the device first)."""
        gpu = self.gpu
        self.refill(self.d_beams)
        if w is not None:
            gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
        if kind == "acc":
            if w is None:
                self.g.beamform_accumulated(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, self.nt, t_coeff=T_COEFF)
            else:
                self.g.beamform_accumulated_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, self.nt,
                                                     t_coeff=T_COEFF)
        else:
            if w is None:
                self.g.generate_and_beamform(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, t0=0, nt=self.nt)
            else:
                self.g.generate_and_beamform_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, t0=0,
                                                      nt=self.nt)
        return self.read_beams()

    def floats(self, w=None, dt=None, t_coeff=T_COEFF):
        """What the float call returns (index entry point, or with dt the _dt one)."""
        gpu = self.gpu
        self.refill(self.d_beams)
        kw = {"t_coeff": t_coeff} if dt is None else {"dt_coeff": dt}
        if w is None:
            self.g.beamform_accumulated(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, self.nt, **kw)
        else:
            gpu.memcpy_htod(self.d_w, np.ascontiguousarray(w, dtype=np.float32))
            self.g.beamform_accumulated_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, self.nt, **kw)
        return self.read_beams()

    def enqueue_floats(self, weighted, stream):
        """The float call (by index) on ``stream`` and nothing else: what prove_depth captures."""
        if weighted:
            self.g.beamform_accumulated_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, self.nt,
                                                 t_coeff=T_COEFF, stream=stream)
        else:
            self.g.beamform_accumulated(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, self.nt, t_coeff=T_COEFF, stream=stream)

    def prove_depth(self, depth, call, kind=None):
        """Asserts that the beamformer launch of ``call(stream)`` gives some wave at least ``depth`` sample blocks
        (blocks_on_some_wave); ``call`` must have been made once already, since a first call allocates.  Nothing runs.
        With ``kind`` = (output kind of helpers/bacc_cases.py, weighted, math_mode) the captured (gridDim.x, blockDim.x,
        dynamic LDS bytes) must also be what helpers/launch_forms.py: bacc_plan restates for this shape and kind -- the link
        between the CPU census and what the library launches.  Returns (gridDim.x, blockDim.x, proven blocks)."""
        from helpers import hip_graph

        s = self.gpu.Stream()
        grid, block, shared = hip_graph.largest_launch(hip_graph.launches(s, lambda: call(s.handle), shared=True))
        s.synchronize()
        proven = blocks_on_some_wave(self.B, self.C, self.nt, grid, block)
        assert proven >= depth, (f"(A, B, C, nt) = {(self.A, self.B, self.C, self.nt)} launches {grid[0]} workgroups of {block[0]} lanes: "
                                 f"only {proven} block(s) proven on some wave, {depth} wanted -- raise the shape's channel count")
        if kind is not None:
            plan = plan_of((self.A, self.B, self.C, self.nt), kind)
            assert (grid[0], block[0], shared) == (plan["grid"], plan["block"], plan["lds"]), \
                (f"(A, B, C, nt) = {(self.A, self.B, self.C, self.nt)}, {kind}: the launch is (grid, block, LDS bytes) = "
                 f"{(grid[0], block[0], shared)}, the plan {(plan['grid'], plan['block'], plan['lds'])}")
            assert proven <= max(plan["blocks_full"][-1], plan["blocks_last"][-1])
        return grid[0], block[0], proven

    def enqueue_fused(self, weighted, stream, dts=None):
        """The fused call (from time index 0, or at the fDeltaTime values dts) on ``stream`` and nothing else: what
        prove_passes captures.  Weighted, it reads the weights the last weighted call left in d_w."""
        kw = {"t0": 0, "nt": self.nt} if dts is None else {"dt": dts}
        if weighted:
            self.g.generate_and_beamform_weighted(self.d_ant, self.ant.nbytes, self.d_w, self.d_beams, self.nbytes, stream=stream, **kw)
        elif dts is None:
            self.g.generate_and_beamform(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, stream=stream, **kw)
        else:
            self.g.generate_and_beamform_dt(self.d_ant, self.ant.nbytes, self.d_beams, self.nbytes, dts, stream=stream)

    def prove_passes(self, passes, call):
        """Asserts that the fused beamformer launch of ``call(stream)`` is ``passes`` = (channels per workgroup, channels per
        pass, live channels in the last workgroup's last pass), read from the launch (passes_of_fused_launch); ``call``
        must have been made once already, since a first call allocates, and covers at most 256 time steps (one launch: a
        longer call refuses the capture).  Nothing runs.  Returns the proven triple."""
        from helpers import hip_graph

        s = self.gpu.Stream()
        nodes = hip_graph.launches(s, lambda: call(s.handle), shared=True)
        s.synchronize()
        grid, block, shared_bytes = hip_graph.largest_launch(nodes)  # asserts that the maximum is unique
        assert grid[1] == grid[2] == 1 and block[1] == block[2] == 1, (grid, block)
        proven = passes_of_fused_launch(self.A, self.B, self.C, self.nt // 16, grid[0], shared_bytes)
        assert proven == tuple(passes), (f"(A, B, C, nt) = {(self.A, self.B, self.C, self.nt)} launches {grid[0]} workgroups with {shared_bytes} "
                                         f"bytes of LDS: (cpb, CH, live in the last pass) = {proven}, {tuple(passes)} wanted")
        return proven

    def read_beams(self):
        return self.read(self.d_beams, self.nbytes, np.float32, self.shape)

    def coefficients(self, dts):
        """The oracle's fp32 coefficients [t][c][a][b][2] (the table turned to the generator's [a*B + b])."""
        t_ab = np.ascontiguousarray(self.table.reshape(self.B, self.A).T).ravel()
        return self.oracle.generate_dt(self.op, t_ab, dts)


def random_weights(rng, B, A, zero_beam=True):
    w = (rng.choice([-1.0, 1.0], size=(B, A)) * 10.0 ** rng.uniform(-3, 3, size=(B, A))).astype(np.float32)
    if zero_beam:
        w[rng.integers(0, B)] = 0.0
    return w
