"""A host stand-in for dc_sand_amd.device, for the CPU tests of the GPU tests' helpers (tests/test_device_buffers.py,
tests/test_parity_case.py)."""
import ctypes

import numpy as np


class HostAllocation:
    def __init__(self, device, nbytes):
        assert nbytes >= 1
        self.device, self.nbytes, self.buf = device, nbytes, (ctypes.c_uint8 * nbytes)()

    def __int__(self):
        return ctypes.addressof(self.buf)

    def free(self):
        self.device.freed.append(int(self))
        del self.device.live[int(self)]


class HostDevice:
    """mem_alloc, memset, memcpy_htod, memcpy_dtoh and synchronize over ctypes buffers; every access is checked to lie inside
    one live allocation, and free() is counted."""

    def __init__(self):
        self.live, self.freed, self.synchronized = {}, [], 0

    def mem_alloc(self, nbytes):
        a = HostAllocation(self, nbytes)
        self.live[int(a)] = a
        return a

    def _bytes(self, address, nbytes):
        address = int(address)
        for base, a in self.live.items():
            if base <= address and address + nbytes <= base + a.nbytes:
                return np.frombuffer(a.buf, np.uint8)[address - base:address - base + nbytes]
        raise AssertionError(f"{nbytes} bytes at {address:#x} lie in no live allocation")

    def memset(self, dst, value, nbytes, stream=None):
        self._bytes(dst, nbytes)[:] = value

    def memcpy_htod(self, dst, src):
        self._bytes(dst, src.nbytes)[:] = src.view(np.uint8).ravel()

    def memcpy_dtoh(self, dst, src):
        dst.view(np.uint8).ravel()[:] = self._bytes(src, dst.nbytes)

    def synchronize(self):
        self.synchronized += 1
