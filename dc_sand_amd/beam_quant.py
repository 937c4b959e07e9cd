"""Quantised int8 beam output (``include/dcs_beam_quant.h``): the host side of a deployed beamformer's per-beam
quantisation gain and its clip counter.  :class:`BeamQuantGains` holds the ``[nr_beams]`` gains (all ones at first), their
device copy and a device array of ``[nr_beams]`` 64-bit clip counters, which
:meth:`dc_sand_amd.generator.SteeringCoefficientGenerator.beamform_accumulated_q8` (and, for the complex product,
``beamform_accumulated_complex_q8``: ``include/dcs_beam_complex_quant.h``) reads and adds to when its work runs.
"""
from __future__ import annotations

import numpy as np

from . import device
from .parameters import BeamformerParameters


class BeamQuantGains:
    def __init__(self, params: BeamformerParameters):
        self.params = params
        self.n_beams = int(params.NR_BEAMS)
        self.host = np.ones(self.n_beams, dtype=np.float32)
        self._dev = None
        self._clips = None

    def _beam(self, beam: int, what: str = "beam") -> int:
        if not 0 <= int(beam) < self.n_beams:
            raise ValueError(f"{what} {beam} out of range [0, {self.n_beams})")
        return int(beam)

    def set(self, beam: int, gain: float) -> None:
        """The quantisation gain of one beam: the int8 output is ``clamp(rint(v * gain), -127, 127)``."""
        self.host[self._beam(beam)] = np.float32(gain)

    def upload(self, stream=None) -> None:
        """Copy the gains to the device on ``stream`` (the calls queued after it on that stream see them).  The first
        upload also makes the clip counters, zeroed."""
        if self._dev is None:
            self._dev = device.mem_alloc(self.host.nbytes)
            self._clips = device.mem_alloc(self.n_beams * 8)
            device.memset(self._clips, 0, self.n_beams * 8, stream=stream)
        device.memcpy_htod(self._dev, self.host, stream=stream)

    def device_ptr(self, beam_offset: int = 0) -> int:
        """The device address of beam ``beam_offset``'s gain: what a context that holds the beams from ``beam_offset`` on
        passes as ``d_quant_gains``."""
        if self._dev is None:
            raise RuntimeError("BeamQuantGains.upload() first")
        return int(self._dev) + self._beam(beam_offset, "beam_offset") * 4

    def clip_count_ptr(self, beam_offset: int = 0) -> int:
        """The device address of beam ``beam_offset``'s clip counter (``d_clip_count`` of the same context)."""
        if self._clips is None:
            raise RuntimeError("BeamQuantGains.upload() first")
        return int(self._clips) + self._beam(beam_offset, "beam_offset") * 8

    def clip_counts(self, reset: bool = False, stream=None) -> np.ndarray:
        """The ``[nr_beams]`` clip counters (clipped components per beam, re and im counted separately, summed over the
        calls since the last reset), downloaded after the work queued on ``stream``; ``reset`` zeroes them afterwards."""
        if self._clips is None:
            raise RuntimeError("BeamQuantGains.upload() first")
        out = np.empty(self.n_beams, dtype=np.uint64)
        device.memcpy_dtoh(out, self._clips, stream=stream)
        if reset:
            device.memset(self._clips, 0, self.n_beams * 8, stream=stream)
            device.stream_synchronize(stream)
        return out

    def free(self) -> None:
        for name in ("_dev", "_clips"):
            buf = getattr(self, name)
            if buf is not None:
                buf.free()
                setattr(self, name, None)
