"""The channeliser held to its 64-bit offsets (include/dcs_channeliser.h): an input and a float output past 2^32 bytes, which
never exist on the host (helpers/large_tensor.py, helpers/channeliser_large.py).  A byte offset worked out in 32 bits wraps
inside the same allocation, 4 GiB lower: nothing faults, so the input holds a pattern in which the pairs 4 GiB apart differ
and the outputs are prefilled.  Every other test of the channeliser passes with 32-bit offsets; this one does not
(tests/test_channeliser_large_plan.py shows it without a device).  The quantised call runs at the same shape: its output stays
below the line, its input offsets pass it."""
import numpy as np
import pytest

from dc_sand_amd import channeliser
from helpers import channeliser_large as cl
from helpers import channeliser_model as model
from helpers import large_tensor as lt
from helpers.device_buffers import Context

pytestmark = pytest.mark.gpu


def test_input_and_outputs_past_the_line(gpu):
    c = Context(gpu, 1, NR_SAMPLES_PER_CHANNEL=16)
    g = c.g
    pat, h, W, gains = cl.pattern(61), cl.taps(62), channeliser.twiddles(cl.N), cl.gains()
    assert cl.IN_BYTES > lt.LINE and cl.OUT_BYTES > lt.LINE
    try:
        d_in = c.alloc(cl.IN_BYTES)
        d_out, d_q8 = c.out(cl.OUT_BYTES, cl.PREFILL, cl.PREFILL), c.out(cl.OUT_Q8_BYTES, cl.PREFILL, cl.PREFILL)
        d_h, d_w, d_g, d_n = c.upload(h), c.upload(W), c.upload(gains), c.upload(np.zeros(cl.NI, dtype=np.uint64))
        lt.fill(gpu, d_in, cl.IN_BYTES, pat)
        g.channelise(d_in, cl.IN_BYTES, cl.IN_STRIDE, cl.NI, cl.NR_SPECTRA, cl.N, cl.P, d_h, d_w, d_out, cl.OUT_BYTES, cl.BLOCKS, cl.NI)
        g.channelise_q8(d_in, cl.IN_BYTES, cl.IN_STRIDE, cl.NI, cl.NR_SPECTRA, cl.N, cl.P, d_h, d_w, d_g, d_q8, cl.OUT_Q8_BYTES,
                        cl.BLOCKS, cl.NI, d_clip_count=d_n)
        gpu.synchronize()
        run, run8 = np.empty((16, 2), dtype=np.float32), np.empty((16, 2), dtype=np.int8)
        for i, b in cl.plan(63):
            exp = cl.expected(pat, h, W, i, b)
            exp8, _ = cl.expected_q8(pat, h, W, i, b)
            for ch in range(cl.N):
                gpu.memcpy_dtoh(run, int(d_out) + cl.out_offset(ch, b, i))
                assert model.same_bits(run, exp[ch]) is None, (i, b, ch, model.same_bits(run, exp[ch]))
                gpu.memcpy_dtoh(run8, int(d_q8) + cl.out_offset(ch, b, i, elem=1))
                assert np.array_equal(run8, exp8[ch]), (i, b, ch)
        c.guard_untouched(d_out)
        c.guard_untouched(d_q8)
        counts = np.empty(cl.NI, dtype=np.uint64)
        gpu.memcpy_dtoh(counts, d_n)
        assert np.all(counts > 0) and np.all(counts < np.uint64(cl.NR_SPECTRA * cl.N * 2))
        # what the device holds is the pattern, on both sides of the input's line
        edge = np.empty(2048, dtype=np.float32)
        gpu.memcpy_dtoh(edge, int(d_in) + lt.LINE - 4096)
        assert np.array_equal(edge, lt.elements_of(pat, (lt.LINE - 4096) // 4 + np.arange(2048)))
    finally:
        c.close()
