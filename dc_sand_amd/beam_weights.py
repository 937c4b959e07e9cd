"""Per-input beam weights (``include/dcs_beam_weights.h``): the host side of the reference control plane's one data-path
command, ``?beam-weights <beam-stream> w_1 ... w_A`` -- one real weight per antenna for one beam, refused when the count
is not the number of antennas.  :class:`BeamWeights` holds the ``[nr_beams][nr_stations]`` array (all ones at first) and
its device copy, which the weighted beamformers of
:class:`dc_sand_amd.generator.SteeringCoefficientGenerator` read when their work runs.
"""
from __future__ import annotations

import numpy as np

from . import device
from .parameters import BeamformerParameters


class BeamWeights:
    def __init__(self, params: BeamformerParameters):
        self.params = params
        self.n_beams = int(params.NR_BEAMS)
        self.n_antennas = int(params.NR_STATIONS)
        self.host = np.ones((self.n_beams, self.n_antennas), dtype=np.float32)
        self._dev = None

    def set(self, beam: int, *weights) -> None:
        """One ``?beam-weights`` request: the weights of every antenna of ``beam``, in antenna order."""
        if len(weights) != self.n_antennas:
            raise ValueError(f"{len(weights)} weights received, expected {self.n_antennas}")
        if not 0 <= int(beam) < self.n_beams:
            raise ValueError(f"beam {beam} out of range [0, {self.n_beams})")
        self.host[int(beam)] = np.asarray(weights, dtype=np.float32)

    def upload(self, stream=None) -> None:
        """Copy the array to the device on ``stream`` (the beamformer calls queued after it on that stream see it)."""
        if self._dev is None:
            self._dev = device.mem_alloc(self.host.nbytes)
        device.memcpy_htod(self._dev, self.host, stream=stream)

    def device_ptr(self, beam_offset: int = 0) -> int:
        """The device address of beam ``beam_offset``'s row: what a context that holds the beams from ``beam_offset`` on
        passes as ``d_weights``."""
        if self._dev is None:
            raise RuntimeError("BeamWeights.upload() first")
        if not 0 <= int(beam_offset) < self.n_beams:
            raise ValueError(f"beam_offset {beam_offset} out of range [0, {self.n_beams})")
        return int(self._dev) + int(beam_offset) * self.n_antennas * 4

    def free(self) -> None:
        if self._dev is not None:
            self._dev.free()
            self._dev = None
