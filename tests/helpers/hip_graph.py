"""Stream capture into a hipGraph for the GPU tests, through the HIP runtime itself: the one the product library is linked
to, reached through that library's handle ("Which runtime the tests use").  The capture mode is 0
(hipStreamCaptureModeGlobal).  A stream is a ``device.Stream`` or a raw ``hipStream_t``; the caller
makes it.

``with capture(s) as g:`` begins a capture on ``s`` and always ends it, also when the body raises -- the graph is then
destroyed and the exception goes on, so the stream is not left capturing for the next test.  After the block ``g`` is
the instantiated graph: ``g.launch(s)`` as often as wanted, then ``g.close()``.  ``begin`` / ``end`` / ``destroy`` are
for the sites that do not instantiate what they capture.

``launches(s, fn)`` captures what ``fn()`` enqueues on ``s`` and returns the (gridDim, blockDim) of every kernel node without
running anything: how a test proves the geometry a launcher chose instead of restating the launcher's arithmetic.  With a
list ``others`` it also names the types of the nodes that are no kernels (a memset node, say).  With ``shared=True`` every
kernel node is (gridDim, blockDim, sharedMemBytes): the dynamic LDS a launcher asked for tells which instantiation of a
kernel template it took where the grid alone does not.

While a stream captures, Python's cyclic collector is off.  It runs wherever an allocation count happens to cross its
threshold, and a test object it collects frees its device memory: hipFree under a global-mode capture invalidates the
capture, and the next launch of the innocent test that captures fails with hipErrorStreamCaptureInvalidated (901)."""
import ctypes
import gc

V = ctypes.c_void_p
_HIP = None
_CAPTURING = 0   # captures begun here and not yet ended
_GC_WAS_ON = False


class _Dim3(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint), ("y", ctypes.c_uint), ("z", ctypes.c_uint)]


class _KernelNodeParams(ctypes.Structure):  # hipKernelNodeParams (hip_runtime_api.h)
    _fields_ = [("blockDim", _Dim3), ("extra", V), ("func", V), ("gridDim", _Dim3), ("kernelParams", V),
                ("sharedMemBytes", ctypes.c_uint)]


_NODE_TYPE_KERNEL = 0  # hipGraphNodeTypeKernel
NODE_TYPE_MEMSET = 2   # hipGraphNodeTypeMemset


# every HIP entry point this module calls, with its argument types (tests/test_hip_runtime.py looks each of them up)
ENTRY_POINTS = {
    "hipStreamBeginCapture": [V, ctypes.c_int],
    "hipStreamEndCapture": [V, ctypes.POINTER(V)],
    "hipGraphInstantiate": [ctypes.POINTER(V), V, V, V, ctypes.c_size_t],
    "hipGraphLaunch": [V, V],
    "hipGraphExecDestroy": [V],
    "hipGraphDestroy": [V],
    "hipGraphGetNodes": [V, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)],
    "hipGraphNodeGetType": [V, ctypes.POINTER(ctypes.c_int)],
    "hipGraphKernelNodeGetParams": [V, ctypes.POINTER(_KernelNodeParams)],
}


class _Entries:
    pass


def _hip():
    """The entry points above, looked up through the handle of the product library: a lookup on that handle searches the
    library and what it depends on, so it finds the HIP runtime the library itself calls -- the one that made every stream
    a test hands in -- whatever else the process has mapped.  No library is opened by name here."""
    global _HIP
    if _HIP is None:
        from dc_sand_amd import _lib

        lib = _lib.lib()
        hip = _Entries()
        for name, argtypes in ENTRY_POINTS.items():
            fn = lib[name]  # a function object of its own: nothing is cached on the product library's handle
            fn.restype = ctypes.c_int
            fn.argtypes = argtypes
            setattr(hip, name, fn)
        _HIP = hip
    return _HIP


def _stream(stream):
    return V(getattr(stream, "handle", stream))


def begin(stream):
    global _CAPTURING, _GC_WAS_ON
    assert _hip().hipStreamBeginCapture(_stream(stream), 0) == 0
    if _CAPTURING == 0:
        _GC_WAS_ON = gc.isenabled()
        gc.disable()
    _CAPTURING += 1


def _end(stream):
    global _CAPTURING
    graph = V()
    rc = _hip().hipStreamEndCapture(_stream(stream), ctypes.byref(graph))
    _CAPTURING -= 1
    if _CAPTURING == 0 and _GC_WAS_ON:
        gc.enable()
    return rc, graph


def end(stream):
    """Ends the capture, which must have stayed valid; the graph (``destroy`` it)."""
    rc, graph = _end(stream)
    assert rc == 0 and graph.value, f"hipStreamEndCapture: {rc} (an unjoined fork, or a call that invalidated the capture?)"
    return graph


def destroy(graph):
    _hip().hipGraphDestroy(graph)


class capture:
    def __init__(self, stream):
        self._s = stream
        self._graph = self._exec = None

    def __enter__(self):
        begin(self._s)
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            _, graph = _end(self._s)
            if graph.value:
                destroy(graph)
            return False
        self._graph = end(self._s)
        self._exec = V()
        assert _hip().hipGraphInstantiate(ctypes.byref(self._exec), self._graph, None, None, 0) == 0
        return False

    def launch(self, stream):
        assert _hip().hipGraphLaunch(self._exec, _stream(stream)) == 0

    def close(self):
        _hip().hipGraphExecDestroy(self._exec)
        destroy(self._graph)


def kernel_nodes(graph, others=None, shared=False):
    """[((grid x, y, z), (block x, y, z))] of every kernel node of a captured (not instantiated) graph; read-only.  The
    hipGraphNodeType of every other node is appended to ``others`` where a list is given.  ``shared=True``: every entry is
    ((grid x, y, z), (block x, y, z), sharedMemBytes), the dynamic LDS of the launch in bytes."""
    hip = _hip()
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (V * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    out = []
    for node in nodes[:n.value]:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(V(node), ctypes.byref(kind)) == 0
        if kind.value != _NODE_TYPE_KERNEL:
            if others is not None:
                others.append(kind.value)
            continue
        p = _KernelNodeParams()
        rc = hip.hipGraphKernelNodeGetParams(V(node), ctypes.byref(p))
        assert rc == 0, f"hipGraphKernelNodeGetParams: {rc}"
        g, b = p.gridDim, p.blockDim
        assert g.x >= 1 and g.y >= 1 and g.z >= 1 and 1 <= b.x * b.y * b.z <= 1024, ((g.x, g.y, g.z), (b.x, b.y, b.z))
        dims = ((g.x, g.y, g.z), (b.x, b.y, b.z))
        out.append(dims + (int(p.sharedMemBytes),) if shared else dims)
    return out


def launches(stream, fn, others=None, shared=False):
    """The kernel launches ``fn()`` enqueues on ``stream``, captured and thrown away: nothing runs.  ``fn`` must only
    launch (a call that allocates on first use is made once, plainly, beforehand).  ``others``, ``shared``: as kernel_nodes
    takes them."""
    begin(stream)
    try:
        fn()
    except BaseException:
        _, graph = _end(stream)
        if graph.value:
            destroy(graph)
        raise
    graph = end(stream)
    try:
        return kernel_nodes(graph, others, shared)
    finally:
        destroy(graph)


def largest_launch(nodes):
    """The rule that names a call's main kernel among its launches: the node with the most workgroups.  (A beamformer
    call is the small kernel that makes the table's terms, one lane per pair, and the beamformer itself, whose every
    workgroup takes a few sample blocks of one channel: at the shapes that use this rule it has at least five times the
    terms kernel's workgroups, and the caller asserts that the maximum is unique.  The fused beamformer's shapes that use
    it launch 2048 workgroups and more against the 514 at the most of their terms kernel, which has a row of workgroups
    per time step.)  The nodes as kernel_nodes returns them, with or without their sharedMemBytes."""
    assert nodes, "no kernel node was captured"
    sizes = sorted((n[0][0] * n[0][1] * n[0][2] for n in nodes), reverse=True)
    assert len(sizes) == 1 or sizes[0] > sizes[1], nodes
    return max(nodes, key=lambda n: n[0][0] * n[0][1] * n[0][2])
