"""The down-converter held to its 64-bit offsets (include/dcs_ddc.h): a sample tensor and an output tensor past 2^32 bytes,
which never exist on the host (helpers/large_tensor.py, helpers/ddc_large.py).  A byte offset worked out in 32 bits wraps
inside the same allocation, 4 GiB lower: nothing faults, so the samples hold a pattern in which the bytes 4 GiB apart differ
and the output is prefilled.  Every other test of the down-converter passes with 32-bit offsets; this one does not
(tests/test_ddc_large_plan.py shows it without a device)."""
import numpy as np
import pytest

from helpers import ddc_large as dl
from helpers import ddc_model as model
from helpers import large_tensor as lt
from helpers.device_buffers import Context

pytestmark = pytest.mark.gpu


def test_samples_and_outputs_past_the_line(gpu):
    from dc_sand_amd.generator import ddc_digits_bytes

    c = Context(gpu, 1, NR_SAMPLES_PER_CHANNEL=16)
    g = c.g
    pat, tp = dl.pattern(51), dl.taps(52).astype(np.int32)
    assert dl.SAMPLES_BYTES > lt.LINE and dl.OUT_BYTES > lt.LINE
    try:
        d_x, d_out = c.alloc(dl.SAMPLES_BYTES), c.out(dl.OUT_BYTES, dl.PREFILL, dl.PREFILL)
        d_taps, d_digits = c.upload(tp), c.alloc(ddc_digits_bytes(dl.T))
        lt.fill(gpu, d_x, dl.SAMPLES_BYTES, pat)
        g.ddc_tap_digits(d_taps, dl.T, dl.NB, d_digits, ddc_digits_bytes(dl.T))
        g.ddc(d_x, dl.SAMPLES_BYTES, dl.IN_STRIDE, dl.NI, dl.NR_OUT, d_digits, ddc_digits_bytes(dl.T), dl.T, dl.BANDS, d_out, dl.OUT_BYTES,
              dl.OUT_STRIDE)
        gpu.synchronize()
        got = np.empty((dl.WINDOW, 2), dtype=np.float32)
        for i, m0 in dl.plan(53):
            exp = dl.expected(pat, tp, i, m0)
            for b in range(dl.NB):
                gpu.memcpy_dtoh(got, int(d_out) + dl.out_offset(b, i, m0))
                assert model.same_bits(got, exp[b]) is None, (b, i, m0, model.same_bits(got, exp[b]))
        pad = np.empty(64, dtype=np.uint8)
        for b in range(dl.NB):
            for i in range(dl.NI):
                gpu.memcpy_dtoh(pad, int(d_out) + dl.out_offset(b, i, dl.NR_OUT))  # behind a row: padding, or the canary
                assert np.all(pad == dl.PREFILL), (b, i)
        # what the device holds is the pattern, on both sides of the samples' line
        edge = np.empty(8192, dtype=np.int8)
        gpu.memcpy_dtoh(edge, int(d_x) + lt.LINE - 4096)
        assert np.array_equal(edge, lt.elements_of(pat, lt.LINE - 4096 + np.arange(8192)))
    finally:
        c.close()
