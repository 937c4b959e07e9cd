"""The plan of tests/test_gpu_channeliser_large.py, without a device: that both tensors pass 2^32 bytes where the plan says,
that the input pattern's period does not divide 2^32, and -- the CPU stand-in for "would fail if the kernel's offsets were
32-bit" -- that for every sampled window that reads at or above the input's line the pairs 4 GiB lower give other outputs,
and that a store 4 GiB low would land in a sampled window that holds other values."""
import re
from pathlib import Path

import numpy as np

from dc_sand_amd import channeliser
from helpers import channeliser_large as cl
from helpers import channeliser_model as model
from helpers import large_tensor as lt

ROOT = Path(__file__).resolve().parents[1]


def test_sizes_lines_and_period():
    assert cl.IN_BYTES == cl.OUT_BYTES == lt.LINE + 16384
    # one block fewer and neither tensor passes the line
    assert cl.NI * 16 * (cl.BLOCKS - 1) * cl.N * 8 <= lt.LINE and cl.N * (cl.BLOCKS - 1) * cl.NI * 128 <= lt.LINE
    assert cl.OUT_Q8_BYTES < lt.LINE
    assert cl.BLOCK_LINE_IN == (1 << 18) - 1 and cl.in_offset(1, cl.BLOCK_LINE_IN) == lt.LINE
    assert (cl.C_LINE_OUT, cl.BLOCK_LINE_OUT) == (63, (1 << 18) - 63) and cl.out_offset(63, cl.BLOCK_LINE_OUT, 0) == lt.LINE
    assert cl.out_offset(cl.N - 1, cl.BLOCKS - 1, cl.NI - 1) + 128 == cl.OUT_BYTES
    assert cl.in_offset(cl.NI - 1, cl.BLOCKS - 1) + 16 * cl.N * 8 == cl.IN_BYTES
    pat = cl.pattern(61)
    assert pat.shape[0] % 2 == 1 and lt.LINE % pat.nbytes != 0 and pat.nbytes <= lt.HOST_LIMIT
    # an item is one block of both inputs (up to 4 share one at N = 64), and the grid is capped: the workgroups of the large
    # test walk four items and a fifth, so the loop over items is held to the model too
    grid = re.search(r"constexpr uint32_t kGrid = 1u << (\d+);", (ROOT / "dc_sand_amd" / "csrc" / "bf_channeliser.hip").read_text())
    assert 4 << int(grid.group(1)) < cl.BLOCKS


def test_the_plan_covers_both_lines_and_their_aliases():
    plan = cl.plan(63)
    assert len(plan) <= 16 and len(set(plan)) == len(plan)
    assert {(1, cl.BLOCK_LINE_IN - 1), (1, cl.BLOCK_LINE_IN), (1, cl.BLOCK_LINE_IN + 1), (0, 0), (0, 1)} <= set(plan)
    assert {(i, b) for i in range(cl.NI) for b in (cl.BLOCK_LINE_OUT - 1, cl.BLOCK_LINE_OUT, 0, cl.BLOCKS - 1)} <= set(plan)
    assert cl.in_offset(1, cl.BLOCK_LINE_IN + 1) - lt.LINE == cl.in_offset(0, 1)


def test_a_wrapped_input_offset_would_show():
    pat, h, W = cl.pattern(61), cl.taps(62), channeliser.twiddles(cl.N)
    seen = 0
    for i, b in cl.plan(63):
        if cl.in_offset(i, b) + 16 * cl.N * 8 <= lt.LINE:
            assert np.array_equal(cl.window_pairs(pat, i, b), cl.window_pairs(pat, i, b, wrapped=True))
            continue
        seen += 1
        own, low = cl.expected(pat, h, W, i, b), cl.expected(pat, h, W, i, b, wrapped=True)
        assert np.all(np.any(own.view(np.uint32) != low.view(np.uint32), axis=(0, 2))), (i, b)  # every spectrum of the window
    assert seen == 2  # the smallest shape: the two last blocks of input 1 are all that lies above the line


def test_a_wrapped_store_would_show():
    """The runs of channel 63 from (block BLOCK_LINE_OUT, input 0) on lie above the float output's line; 4 GiB lower are the
    runs of channel 0 from (block 0, input 0) on, of sampled windows whose own values differ."""
    pat, h, W = cl.pattern(61), cl.taps(62), channeliser.twiddles(cl.N)
    for i in range(cl.NI):
        assert cl.out_offset(63, cl.BLOCK_LINE_OUT, i) - lt.LINE == cl.out_offset(0, 0, i)
        above, below = cl.expected(pat, h, W, i, cl.BLOCK_LINE_OUT)[63], cl.expected(pat, h, W, i, 0)[0]
        assert not np.any(above.view(np.uint32) == below.view(np.uint32))
        assert not np.any(above.view(np.uint32) == np.uint32(0xA5A5A5A5))  # a store that went 4 GiB low leaves the prefill


def test_the_quantised_windows_are_no_trivial_expectation():
    pat, h, W = cl.pattern(61), cl.taps(62), channeliser.twiddles(cl.N)
    q, n = cl.expected_q8(pat, h, W, 1, cl.BLOCK_LINE_IN)
    assert np.unique(q).size >= 100 and 0 < n < q.size // 2
    assert model.same_bits(cl.expected(pat, h, W, 1, cl.BLOCK_LINE_IN), cl.expected(pat, h, W, 0, 0)) is not None
