"""The device memory of one GPU test, and the guard that shows whether a kernel wrote out of bounds.  Inputs are exactly
sized (upload), so that a tensor's last row ends where its allocation ends; an output (out) has CANARY guard bytes behind
it, which read and guard_untouched assert.  Everything handed out is freed by close(), whatever the test's end: use it
from a fixture that yields and closes, or in a try/finally.  tests/test_device_buffers.py drives it on the CPU."""
import numpy as np

CANARY = 64
GUARD = 0xA5


class DeviceBuffers:
    """``gpu`` is dc_sand_amd.device, or a stand-in with its mem_alloc, memset, memcpy_htod, memcpy_dtoh and synchronize.
    With ``limit`` the bytes asked for are counted in ``total`` and may not pass it."""

    def __init__(self, gpu, limit=None):
        self.gpu, self.limit, self.total = gpu, limit, 0
        self.held = []
        self.outs = {}  # address -> (nbytes, prefill, guard) of the buffers out() made

    def alloc(self, nbytes):
        self.total += nbytes
        assert self.limit is None or self.total <= self.limit, (self.total, self.limit)
        a = self.gpu.mem_alloc(max(nbytes, 1))
        self.held.append(a)
        return a

    def upload(self, array):
        """Exactly array.nbytes: the last row ends where the allocation ends."""
        array = np.ascontiguousarray(array)
        d = self.alloc(array.nbytes)
        if array.nbytes:
            self.gpu.memcpy_htod(d, array)
        return d

    def out(self, nbytes, prefill=GUARD, guard=GUARD):
        """nbytes of ``prefill`` and CANARY bytes of ``guard`` behind them."""
        d = self.alloc(nbytes + CANARY)
        self.outs[int(d)] = (nbytes, prefill, guard)
        self.refill(d)
        return d

    def refill(self, d, stream=None):
        """The body and the guard of an out() buffer as they were made, for the next call on it."""
        nbytes, prefill, guard = self.outs[int(d)]
        self.gpu.memset(d, prefill, nbytes, stream=stream)
        self.gpu.memset(int(d) + nbytes, guard, CANARY, stream=stream)

    def read(self, d, nbytes=None, dtype=np.uint8, shape=None):
        """A copy of the first ``nbytes`` (default: all) of an out() buffer; every byte from there to the end of the
        allocation must hold the guard byte.  With nbytes below the buffer's size that covers the unused remainder of the
        body as well, so it is only meaningful where prefill == guard."""
        size, _, guard = self.outs[int(d)]
        nbytes = size if nbytes is None else nbytes
        assert 0 <= nbytes <= size, (nbytes, size)
        host = np.empty(size + CANARY, dtype=np.uint8)
        self.gpu.memcpy_dtoh(host, d)
        assert np.all(host[nbytes:] == guard), "written past the tensor"
        body = host[:nbytes].view(dtype)
        return body.copy() if shape is None else body.reshape(shape).copy()

    def guard_untouched(self, d, nbytes=None):
        """Only the CANARY bytes behind the first ``nbytes`` (default: the whole body) are downloaded and asserted: for
        tensors past 4 GiB, which never exist on the host."""
        size, _, guard = self.outs[int(d)]
        nbytes = size if nbytes is None else nbytes
        assert 0 <= nbytes <= size, (nbytes, size)
        tail = np.empty(CANARY, dtype=np.uint8)
        self.gpu.memcpy_dtoh(tail, int(d) + nbytes)
        assert np.all(tail == guard), "written past the tensor"

    def close(self):
        self.gpu.synchronize()
        for a in self.held:
            a.free()
        self.held, self.outs = [], {}


class Context(DeviceBuffers):
    """The buffers of one test with the SteeringCoefficientGenerator ``g`` of C channels, A antennas and B beams (``bp``)
    whose calls they serve; close() closes both."""

    def __init__(self, gpu, C, A=1, B=1, **parameters):
        from dc_sand_amd import BeamformerParameters
        from dc_sand_amd.generator import SteeringCoefficientGenerator

        super().__init__(gpu)
        self.C, self.A, self.B = C, A, B
        self.bp = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, **parameters)
        self.g = SteeringCoefficientGenerator(self.bp)

    def close(self):
        try:
            super().close()
        finally:
            self.g.close()


def closed_after(make):
    """For a fixture of a test that makes its own cases: ``yield from closed_after(partial(Case, gpu))`` gives the test a
    function that makes a case, and closes every case it made whatever the test's end."""
    made = []

    def tracked(*args, **kwargs):
        made.append(make(*args, **kwargs))
        return made[-1]

    try:
        yield tracked
    finally:
        for m in reversed(made):
            m.close()
