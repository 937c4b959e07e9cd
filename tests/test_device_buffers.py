"""helpers/device_buffers.py on the CPU: DeviceBuffers driven with a host stand-in for dc_sand_amd.device, so that what the
GPU tests rely on -- a byte written behind a tensor is caught, the memory is freed whatever the test's end -- is itself
tested, without a device."""
import numpy as np
import pytest

from helpers.device_buffers import CANARY, DeviceBuffers
from helpers.host_device import HostDevice


@pytest.fixture
def dev():
    return HostDevice()


def test_read_returns_the_body_as_a_copy(dev):
    m = DeviceBuffers(dev)
    d = m.out(24)
    values = np.arange(6, dtype=np.float32).reshape(2, 3)
    dev.memcpy_htod(d, values)
    got = m.read(d, 24, np.float32, (2, 3))
    assert got.dtype == np.float32 and got.shape == (2, 3) and np.array_equal(got, values)
    got[:] = 0  # a copy: the buffer keeps its values
    assert np.array_equal(m.read(d, dtype=np.float32), values.ravel())
    assert m.read(d).dtype == np.uint8 and m.read(d).shape == (24,)
    m.guard_untouched(d)
    m.close()


@pytest.mark.parametrize("offset", [0, CANARY - 1])
def test_a_byte_behind_the_tensor_is_caught(dev, offset):
    """Directly behind the tensor, and the last byte of the guard."""
    m = DeviceBuffers(dev)
    d = m.out(40, prefill=0x3C)
    m.read(d, 40)
    m.guard_untouched(d)
    dev.memset(int(d) + 40 + offset, 0xA4, 1)
    with pytest.raises(AssertionError, match="written past the tensor"):
        m.read(d, 40)
    with pytest.raises(AssertionError, match="written past the tensor"):
        m.guard_untouched(d)
    m.refill(d)
    m.read(d, 40)
    m.close()


def test_read_of_a_part_covers_the_unused_remainder(dev):
    m = DeviceBuffers(dev)
    d = m.out(200)
    dev.memset(d, 7, 16)
    assert np.all(m.read(d, 16) == 7)
    m.guard_untouched(d, 16)
    dev.memset(int(d) + 150, 0, 1)  # inside the body, behind the 16 bytes in use and the CANARY bytes behind them
    m.guard_untouched(d)
    m.guard_untouched(d, 16)
    with pytest.raises(AssertionError, match="written past the tensor"):
        m.read(d, 16)
    dev.memset(int(d) + 150, 0xA5, 1)
    dev.memset(int(d) + 16, 0, 1)
    with pytest.raises(AssertionError, match="written past the tensor"):
        m.guard_untouched(d, 16)
    with pytest.raises(AssertionError):
        m.read(d, 201)  # more than the buffer holds
    m.close()


def test_prefill_and_guard_are_distinct_and_refill_restores_both(dev):
    m = DeviceBuffers(dev)
    d = m.out(32, prefill=0x3C)
    whole = np.empty(32 + CANARY, np.uint8)
    dev.memcpy_dtoh(whole, d)
    assert np.all(whole[:32] == 0x3C) and np.all(whole[32:] == 0xA5)
    dev.memset(d, 0, 32 + CANARY)
    m.refill(d)
    dev.memcpy_dtoh(whole, d)
    assert np.all(whole[:32] == 0x3C) and np.all(whole[32:] == 0xA5)
    e = m.out(8, prefill=0xFF, guard=0xFF)
    assert np.all(m.read(e) == 0xFF)
    dev.memset(int(e) + 8, 0xA5, 1)  # the other buffers' guard byte is no guard byte here
    with pytest.raises(AssertionError):
        m.read(e)
    m.close()


def test_upload_is_exactly_sized_and_an_empty_allocation_is_usable(dev):
    m = DeviceBuffers(dev)
    a = np.arange(30, dtype=np.int16).reshape(5, 6)[:, ::2]  # not contiguous
    d = m.upload(a)
    assert d.nbytes == a.nbytes == 30
    back = np.empty((5, 3), np.int16)
    dev.memcpy_dtoh(back, d)
    assert np.array_equal(back, a)
    z, e = m.alloc(0), m.upload(np.empty(0, np.float32))
    assert int(z) and int(e) and len({int(d), int(z), int(e)}) == 3
    m.close()


def test_close_frees_everything_once_also_after_a_failure(dev):
    def fixture_style():
        m = DeviceBuffers(dev)
        try:
            yield m
        finally:
            m.close()

    it = fixture_style()
    m = next(it)
    handed_out = [int(m.alloc(10)), int(m.upload(np.zeros(3))), int(m.out(5))]
    with pytest.raises(AssertionError):
        it.throw(AssertionError("the test failed"))
    assert sorted(dev.freed) == sorted(handed_out) and not dev.live and dev.synchronized == 1
    m.close()
    assert len(dev.freed) == 3


def test_the_limit_refuses_the_allocation_that_passes_it(dev):
    m = DeviceBuffers(dev, limit=200)
    m.alloc(100)
    m.out(100 - CANARY)
    assert m.total == 200
    with pytest.raises(AssertionError):
        m.alloc(1)
    assert len(dev.live) == 2
    m.close()
