"""helpers/parity_case.py on the CPU: GeneratorCase driven with the host stand-in for dc_sand_amd.device
(helpers/host_device.py) and a stand-in generator whose "kernel" is a numpy fill, so that what the parity tests rely on
-- a write outside the tensor is caught, an element nothing wrote fails the comparison, the ordered-integer distance is the
distance in last places, everything is freed whatever the test's end -- is itself tested, without a device."""
from functools import partial

import numpy as np
import pytest

from helpers.device_buffers import closed_after
from helpers.host_device import HostDevice
from helpers.parity_case import GeneratorCase, check_1ulp, ordered_distance

VALUE = 0.75


class _FillGenerator:
    """The calls GeneratorCase makes on a SteeringCoefficientGenerator.  Every generate* fills its tensor with VALUE, but
    leaves the last ``unwritten`` elements alone, writes ``before`` zero bytes in front of the tensor and ``behind`` of them
    after its end."""
    dev = None
    unwritten = before = behind = 0

    def __init__(self, bp):
        self.bp, self.calls, self.closed = bp, [], 0

    def set_tuning(self, **tuning):
        self.calls.append(("set_tuning", tuning))

    def upload_delays(self, table):
        self.calls.append(("upload_delays", table))

    def _fill(self, name, d_out, out_bytes, bitwidth=1, **kw):
        self.calls.append((name, out_bytes, bitwidth, kw))
        body = self.dev._bytes(d_out, out_bytes).view(np.float32 if bitwidth == 1 else np.float16)
        body[:body.size - self.unwritten] = VALUE
        if self.before:
            self.dev._bytes(d_out - self.before, self.before)[:] = 0
        if self.behind:
            self.dev._bytes(d_out + out_bytes, self.behind)[:] = 0

    def generate(self, d_out, out_bytes, t0, nt, kernel, bitwidth):
        self._fill("generate", d_out, out_bytes, bitwidth, t0=t0, nt=nt, kernel=kernel)

    def generate_slab(self, d_out, out_bytes, c0, nc, t0, nt, bitwidth):
        self._fill("generate_slab", d_out, out_bytes, bitwidth, c0=c0, nc=nc, t0=t0, nt=nt)

    def generate_dt(self, d_out, out_bytes, dt, kernel, bitwidth):
        self._fill("generate_dt", d_out, out_bytes, bitwidth, nt=len(dt), kernel=kernel)

    def generate_slab_dt(self, d_out, out_bytes, c0, nc, dt):
        self._fill("generate_slab_dt", d_out, out_bytes, c0=c0, nc=nc, nt=len(dt))

    def generate_at(self, d_out, out_bytes, current_times, reference_time, kernel):
        self._fill("generate_at", d_out, out_bytes, nt=len(current_times), kernel=kernel)

    def close(self):
        self.closed += 1


@pytest.fixture
def dev(monkeypatch):
    d = HostDevice()
    monkeypatch.setattr("dc_sand_amd.generator.SteeringCoefficientGenerator", type("G", (_FillGenerator,), {"dev": d}))
    return d


def _bp(C=5, A=3, B=7, **more):
    from dc_sand_amd import BeamformerParameters

    return BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, **more)


def test_every_call_returns_its_tensor_and_the_context_is_the_tests_own(dev):
    bp = _bp(SAMPLING_PERIOD=3e-8, FFT_SIZE=1024)
    table = np.zeros(21)
    c = GeneratorCase(dev, bp, table, dict(form=2))
    assert c.g.bp == bp and [k[0] for k in c.g.calls] == ["set_tuning", "upload_delays"] and c.g.calls[1][1] is table
    for got, shape, dtype in ((c.generate(4, 2), (2, 5, 3, 7, 2), np.float32),
                              (c.generate(4, 2, kernel=1, bitwidth=0, offset=4), (2, 5, 3, 7, 2), np.float16),
                              (c.generate_slab(1, 3, 9, 1, offset=8), (1, 3, 3, 7, 2), np.float32),
                              (c.generate_dt(np.zeros(4, np.float32), bitwidth=0), (4, 5, 3, 7, 2), np.float16),
                              (c.generate_slab_dt(2, 2, np.zeros(3, np.float32)), (3, 2, 3, 7, 2), np.float32),
                              (c.generate_at([(1, 0), (1, 5)], (0, 0)), (2, 5, 3, 7, 2), np.float32)):
        assert got.shape == shape and got.dtype == dtype and np.all(got == VALUE)
    assert c.g.calls[2] == ("generate", 2 * 5 * 21 * 8, 1, dict(t0=4, nt=2, kernel=2))
    assert c.g.calls[3] == ("generate", 2 * 5 * 21 * 4, 0, dict(t0=4, nt=2, kernel=1))
    assert c.g.calls[4] == ("generate_slab", 3 * 21 * 8, 1, dict(c0=1, nc=3, t0=9, nt=1))
    assert len(dev.live) == 5  # generate_at's tensor is the first generate's, refilled: one per (nt, nc, bitwidth, offset)
    assert np.all(c.generate(4, 2) == VALUE) and len(dev.live) == 5
    c.close()
    assert not dev.live and c.g.closed == 1


@pytest.mark.parametrize("where,message", [("behind", "written past the tensor"), ("before", "written before the tensor")])
def test_a_write_outside_the_tensor_fails_the_read(dev, where, message):
    c = GeneratorCase(dev, _bp())
    c.generate(0, 1, offset=8)
    setattr(type(c.g), where, 1)
    with pytest.raises(AssertionError, match=message):
        c.generate(0, 1, offset=8)
    c.close()


def test_an_element_left_unwritten_reads_as_nan_and_fails_the_1_ulp_check(dev, oracle):
    c = GeneratorCase(dev, _bp())
    exp = np.full((1, 5, 3, 7, 2), VALUE, np.float32)
    assert check_1ulp(oracle, c.generate(0, 1), exp) == 0
    type(c.g).unwritten = 1
    for bitwidth in (1, 0):
        got = c.generate(0, 1, bitwidth=bitwidth)
        assert np.isnan(got).sum() == 1 and np.isnan(got.ravel()[-1])
    with pytest.raises(AssertionError, match="1 elements over 1 ULP, first flat index 209"):
        check_1ulp(oracle, c.generate(0, 1), exp, tol=None, tag="tagged")
    c.close()


def test_ordered_distance_is_the_distance_in_last_places():
    for f, u, top, largest in ((np.float16, np.uint16, 0x8000, 0x7BFF), (np.float32, np.uint32, 0x80000000, 0x7F7FFFFF)):
        def bits(*patterns):
            return np.array(patterns, dtype=u).view(f)

        assert bits(largest)[0] == np.finfo(f).max  # the largest finite magnitude
        assert ordered_distance(bits(0), bits(top)) == 0                      # +0 and -0
        assert ordered_distance(bits(1), bits(top | 1)) == 2                  # the smallest subnormals of either sign
        assert ordered_distance(bits(0, 5), bits(top | 3, 5)) == 3            # across the sign, the largest of the array
        assert ordered_distance(f([1.0]), np.nextafter(f([1.0]), f(2.0))) == 1
        assert ordered_distance(f([-1.0]), np.nextafter(f([-1.0]), f(0.0))) == 1
        assert ordered_distance(bits(largest), bits(largest - 1)) == 1
        assert ordered_distance(bits(largest), bits(top | largest)) == 2 * largest  # the extremes: no overflow
    with pytest.raises(AssertionError):
        ordered_distance(np.zeros(1, np.float32), np.zeros(1, np.float16))


def test_close_frees_everything_after_a_raised_assertion(dev):
    fixture = closed_after(partial(GeneratorCase, dev))
    make = next(fixture)
    cases = [make(_bp()), make(_bp(B=2), np.zeros(6))]
    cases[0].generate(0, 3)
    cases[1].tensor(2, bitwidth=0)
    assert len(dev.live) == 2
    with pytest.raises(AssertionError, match="the test failed"):
        fixture.throw(AssertionError("the test failed"))
    assert not dev.live and len(dev.freed) == 2 and [c.g.closed for c in cases] == [1, 1]
