"""Stream capture into a hipGraph for the GPU tests, through the HIP runtime itself (libamdhip64.so, loaded once).  The
capture mode is 0 (hipStreamCaptureModeGlobal).  A stream is a ``device.Stream`` or a raw ``hipStream_t``; the caller
makes it.

``with capture(s) as g:`` begins a capture on ``s`` and always ends it, also when the body raises -- the graph is then
destroyed and the exception goes on, so the stream is not left capturing for the next test.  After the block ``g`` is
the instantiated graph: ``g.launch(s)`` as often as wanted, then ``g.close()``.  ``begin`` / ``end`` / ``destroy`` are
for the sites that do not instantiate what they capture."""
import ctypes

V = ctypes.c_void_p
_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipStreamBeginCapture.argtypes = [V, ctypes.c_int]
        hip.hipStreamEndCapture.argtypes = [V, ctypes.POINTER(V)]
        hip.hipGraphInstantiate.argtypes = [ctypes.POINTER(V), V, V, V, ctypes.c_size_t]
        hip.hipGraphLaunch.argtypes = [V, V]
        hip.hipGraphExecDestroy.argtypes = [V]
        hip.hipGraphDestroy.argtypes = [V]
        _HIP = hip
    return _HIP


def _stream(stream):
    return V(getattr(stream, "handle", stream))


def begin(stream):
    assert _hip().hipStreamBeginCapture(_stream(stream), 0) == 0


def _end(stream):
    graph = V()
    return _hip().hipStreamEndCapture(_stream(stream), ctypes.byref(graph)), graph


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
