"""What the parity tests share (tests/test_gpu_parity.py, test_gpu_parity_fused.py, test_gpu_streaming.py): one
generator with its delay table and guarded output tensors, and each comparison with its reasoning, stated once.  The
beamformer tests take their samples and beams from helpers.bacc_case.Case.  tests/test_parity_case.py drives this file on
the CPU."""
import dataclasses

import numpy as np

from helpers.device_buffers import Context

FILL = 0xFF  # a float or a half that no kernel wrote reads as NaN


class Tensor:
    """A tensor of ``shape`` and ``dtype`` that begins ``offset`` bytes into an out() buffer of ``bufs`` (a DeviceBuffers):
    FILL in the body, FILL in the guard behind it.  ``ptr`` and ``nbytes`` are what a call takes."""

    def __init__(self, bufs, shape, dtype=np.float32, offset=0):
        self.bufs, self.shape, self.dtype, self.offset = bufs, tuple(shape), np.dtype(dtype), offset
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.d = bufs.out(offset + self.nbytes, FILL, FILL)
        self.ptr = int(self.d) + offset

    def refill(self, stream=None):
        self.bufs.refill(self.d, stream=stream)

    def read(self):
        """The tensor on the host; the bytes before it and the guard behind it must be as they were made."""
        body = self.bufs.read(self.d)
        assert np.all(body[:self.offset] == FILL), "written before the tensor"
        return body[self.offset:].copy().view(self.dtype).reshape(self.shape)

    def guard_untouched(self):
        """For a tensor that never reaches the host as a whole."""
        self.bufs.guard_untouched(self.d)


class GeneratorCase(Context):
    """The generator of ``bp`` with ``tuning`` set and ``table`` uploaded (None: the test brings the table in itself).
    Every generate*() runs its call into a freshly refilled Tensor and returns it through read(): [nt][nc][A][B][2], floats
    (bitwidth 1) or halves (0).  The calls of one case share a Tensor per (nt, nc, bitwidth, offset), so a loop over
    generate() holds one; what read() returns is a copy.  A test that makes a case per loop turn holds them all until the
    fixture closes them: keep such cases small."""

    def __init__(self, gpu, bp, table=None, tuning=None):
        shape = ("NR_CHANNELS", "NR_STATIONS", "NR_BEAMS")
        super().__init__(gpu, *(getattr(bp, k) for k in shape), **{k: v for k, v in dataclasses.asdict(bp).items() if k not in shape})
        assert self.bp == bp
        self.table, self.reused = table, {}
        if tuning:
            self.g.set_tuning(**tuning)
        if table is not None:
            self.g.upload_delays(table)

    def tensor(self, nt=1, nc=None, bitwidth=1, offset=0):
        return Tensor(self, (nt, self.C if nc is None else nc, self.A, self.B, 2), np.float32 if bitwidth == 1 else np.float16, offset)

    def refilled(self, *key):
        """The Tensor that the generate*() calls of this case share for tensor(*key), as it was made."""
        if key in self.reused:
            self.reused[key].refill()
        else:
            self.reused[key] = self.tensor(*key)
        return self.reused[key]

    def generate(self, t0, nt, kernel=2, bitwidth=1, offset=0):
        t = self.refilled(nt, None, bitwidth, offset)
        self.g.generate(t.ptr, t.nbytes, t0=t0, nt=nt, kernel=kernel, bitwidth=bitwidth)
        return t.read()

    def generate_slab(self, c0, nc, t0, nt, bitwidth=1, offset=0):
        t = self.refilled(nt, nc, bitwidth, offset)
        self.g.generate_slab(t.ptr, t.nbytes, c0, nc, t0=t0, nt=nt, bitwidth=bitwidth)
        return t.read()

    def generate_dt(self, dts, kernel=2, bitwidth=1):
        t = self.refilled(len(dts), None, bitwidth, 0)
        self.g.generate_dt(t.ptr, t.nbytes, dts, kernel=kernel, bitwidth=bitwidth)
        return t.read()

    def generate_slab_dt(self, c0, nc, dts):
        t = self.refilled(len(dts), nc, 1, 0)
        self.g.generate_slab_dt(t.ptr, t.nbytes, c0, nc, dts)
        return t.read()

    def generate_at(self, current_times, reference_time, kernel=2):
        t = self.refilled(len(current_times), None, 1, 0)
        self.g.generate_at(t.ptr, t.nbytes, current_times, reference_time, kernel=kernel)
        return t.read()


def check_1ulp(oracle, got, exp, tol=1e-4, tag=None):
    """The bar of the generator: every fp32 element within 1 ULP of the oracle (ordered-integer distance of the bit
    patterns; a NaN is at no such distance of a number, so an element that nothing wrote fails), and the reference's own
    rule |gpu - cpu| <= 1e-4 (runBeamformerTests.cpp:30,61).  ``tol=None`` where |fRotation| is too large for an absolute
    1e-4 to mean anything, or where the verifier itself has NaNs.  Returns the largest distance."""
    mx, n_over, first = oracle.max_ulp(got, exp, 1)
    assert n_over == 0, f"{'' if tag is None else f'{tag}: '}max ULP {mx}, {n_over} elements over 1 ULP, first flat index {first}"
    if tol is not None:
        assert oracle.compare(got, exp, tol) == -1, tag
    return mx


def check_float_reading(oracle, got, op, table, t0, nt, limit=1):
    """The verifier's other reading (oracle/bf_oracle.c): ``cosf`` / ``sinf`` of the host libm, which is what
    nvcc's headers bind ``cos(fRotation)`` to.  Proven <= 1 ULP for every argument below 256 (and for the
    low-degree set below 512) against this glibc in tests/test_numerics.py; here on the tensor."""
    with oracle.trig_reading(oracle.FLOAT_LIBM):
        exp = oracle.generate(op, table, t0, nt)
    mx, n_over, first = oracle.max_ulp(got, exp, limit)
    assert n_over == 0, f"float-libm reading: max ULP {mx}, {n_over} elements over {limit} ULP, first flat index {first}"
    assert oracle.compare(got, exp, 1e-4) == -1
    return mx


def ordered_distance(got, exp):
    """The largest distance between two arrays of halves, or of floats, in units of the last place: each bit pattern is
    read as sign and magnitude and turned into the integer -magnitude or +magnitude, so that neighbouring values are
    neighbouring integers also across zero (+0 and -0 are the same integer), and the integers are subtracted.  Finite
    values only: a test that expects NaNs compares their places first and zeroes them."""
    def ordered(x):
        x = np.ascontiguousarray(x)
        u = x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize]).astype(np.int64)
        top = 1 << (8 * x.dtype.itemsize - 1)
        return np.where(u & top, -(u & (top - 1)), u)

    assert got.dtype == exp.dtype and got.dtype in (np.float16, np.float32), (got.dtype, exp.dtype)
    return int(np.max(np.abs(ordered(got) - ordered(exp))))


def fused_bound(A):
    """|fused beams - verifier's| over A antennas (BeamformerCoefficientTest.cu:363-414).  The summation order is the
    verifier's, so the only difference is each coefficient's <= 1 ULP: sum|sample| * 2^-23 ~ 2e-3 at 64 antennas of full
    scale; held at 2e-5 * A.  The reference's own tolerance is 1e-1 (runBeamformerTests.cpp:15)."""
    return 2e-5 * A + 1e-6


def accumulated_bound(A):
    """|matrix-core beams - verifier's loop with the coefficient held| over A antennas.  The verifier multiplies and adds
    with separate roundings, and each coefficient is within 1 ULP: 1 ulp of the coefficient + quantisation + the roundings
    of either side <= 3e-7 per unit of sample, samples <= 128 -- 4e-5 * A, reached at A = 1, ten times less at 64
    antennas.  The reference's own tolerance is 1e-1 (runBeamformerTests.cpp:15)."""
    return 4e-5 * A + 1e-6


def check_exact_sum(c, got, dt, tag=None):
    """The fixed-point form of the matrix-core beamformer (24-bit coefficients as three signed digits; sums exact) against
    its own, much tighter, bound: the sum in exact (fp64) arithmetic of the oracle's fp32 coefficients at fDeltaTime ``dt``
    over the samples of the bacc_case.Case ``c``, within 2.5e-7 * sum_a |sample_a| + 2e-7 * |sum|."""
    coef = c.coefficients(dt)[0].astype(np.float64)  # [c][a][b][re, im]
    x = c.ant.astype(np.float64)
    exact = np.einsum("cabk,ctaik->ctbik", coef, x)  # [c][t/16][b][t%16][re, im]
    mag = np.abs(x).sum(axis=2)[:, :, None, :, :]    # sum_a |sample|, per (c, t/16, t%16, plane)
    assert np.all(np.abs(got - exact) <= 2.5e-7 * mag + 2e-7 * np.abs(exact) + 1e-30), tag
