"""The plan of tests/test_gpu_ddc_large.py, without a device: that both tensors pass 2^32 bytes where the plan says, that the
sample pattern's period does not divide 2^32, and -- the CPU stand-in for "would fail if the kernel's offsets were 32-bit" --
that for every sampled window that reads at or above the samples' line the bytes 4 GiB lower give other outputs, and that a
store 4 GiB low would land in a sampled window that holds other values."""
import numpy as np

from helpers import ddc_large as dl
from helpers import ddc_model as model
from helpers import large_tensor as lt


def test_sizes_lines_and_period():
    assert dl.ROW == (1 << 31) + 16 <= dl.IN_STRIDE and dl.IN_STRIDE % 16 == 0
    assert dl.SAMPLES_BYTES == (1 << 32) + (1 << 20) + 16 > lt.LINE
    assert dl.OUT_BYTES == (1 << 32) + 3 * (1 << 19) - 16 > lt.LINE
    # two rows of the fewest outputs that pass the line even without padding (by 32 bytes; one output fewer and they do not)
    assert 2 * dl.ROW == lt.LINE + 32 and 2 * (dl.ROW - 16) <= lt.LINE
    assert (dl.M_LINE_IN, dl.M_LINE_OUT) == ((1 << 27) - (1 << 16), (1 << 27) - 3 * (1 << 16))
    assert dl.IN_STRIDE + 16 * dl.M_LINE_IN == lt.LINE and dl.out_offset(1, 1, dl.M_LINE_OUT) == lt.LINE
    assert 0 < dl.M_LINE_OUT < dl.M_LINE_IN < dl.NR_OUT
    pat = dl.pattern(51)
    assert pat.shape[0] % 2 == 1 and lt.LINE % pat.nbytes != 0 and pat.nbytes <= lt.HOST_LIMIT
    assert np.abs(dl.taps(52)).sum(axis=1).max() <= model.MAX_ABS_SUM
    assert -(-dl.NR_OUT // 512) * dl.NI < 1 << 20  # one workgroup per span: the grid-stride loop is not what is tested here


def test_the_plan_covers_both_lines_and_their_aliases():
    plan = dl.plan(53)
    assert len(plan) <= 24 and len(set(plan)) == len(plan)
    for m in (dl.M_LINE_IN, dl.M_LINE_OUT):
        assert {(1, m - dl.WINDOW), (1, m - dl.WINDOW // 2), (1, m)} <= set(plan)
    assert {(0, 0), (0, 4 * dl.WINDOW), (1, dl.NR_OUT - dl.WINDOW)} <= set(plan)


def test_a_wrapped_sample_offset_would_show():
    pat, tp = dl.pattern(51), dl.taps(52)
    seen = 0
    for i, m0 in dl.plan(53):
        last = i * dl.IN_STRIDE + 16 * (m0 + dl.WINDOW - 1) + dl.T - 1
        if last < lt.LINE:
            assert np.array_equal(dl.window_samples(pat, i, m0), dl.window_samples(pat, i, m0, wrapped=True))
            continue
        seen += 1
        own, low = dl.expected(pat, tp, i, m0), dl.expected(pat, tp, i, m0, wrapped=True)
        reads_above = 16 * (m0 + np.arange(dl.WINDOW)) + dl.T - 1 + i * dl.IN_STRIDE >= lt.LINE
        differs = np.any(own.view(np.uint32) != low.view(np.uint32), axis=(0, 2))
        assert np.array_equal(differs, reads_above), (i, m0)
    assert seen >= 5


def test_a_wrapped_store_would_show():
    """Outputs of (band 1, input 1) from M_LINE_OUT on lie above the output's line; 4 GiB lower is (band 0, input 0) from
    output 0 on, a sampled window whose own values differ."""
    pat, tp = dl.pattern(51), dl.taps(52)
    assert dl.out_offset(1, 1, dl.M_LINE_OUT) - lt.LINE == dl.out_offset(0, 0, 0)
    above, below = dl.expected(pat, tp, 1, dl.M_LINE_OUT)[1], dl.expected(pat, tp, 0, 0)[0]
    assert not np.any(above.view(np.uint32) == below.view(np.uint32))
    prefill = np.uint32(0xA5A5A5A5)
    assert not np.any(above.view(np.uint32) == prefill)  # a store that went 4 GiB low leaves the prefill, which no output equals
