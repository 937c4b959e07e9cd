"""Host-side design of the pulsar folder (include/dcs_fold.h): the phase models ``dcs_bf_fold_model [nr_subints]`` of a spin
frequency, its derivative and a phase at sample 0 that
:meth:`dc_sand_amd.generator.SteeringCoefficientGenerator.fold_q8` takes, the advance of a model by whole spectra, and the
bin of a phase.  numpy and exact rational arithmetic only; needs no built library and no device.

A phase is an unsigned 64-bit integer in units of 2^-64 turn, and every operation on it is modulo 2^64.  For spectrum ``k`` of
a sub-integration ``phi(k) = phase0 + k step + (k (k - 1) / 2) accel`` and ``bin(k) = ((phi(k) >> 32) nbin) >> 32``.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

TURN = 1 << 64
MAX_BINS = 1024
MAX_SUBINT_LEN = 1 << 24

#: ``dcs_bf_fold_model``: 24 bytes, little-endian, no padding
model_dtype = np.dtype([("phase0", "<u8"), ("step", "<u8"), ("accel", "<u8")])


def _units(turns: Fraction) -> int:
    """A phase in turns to the nearest 2^-64 turn, modulo one turn; a negative value is its two's complement."""
    return int(round(turns * TURN)) % TURN


def fold_models(f0_hz, f1_hz_per_s, phase0_turns, sample_time_s, subint_len: int, nr_subints: int, first_sample: int = 0) -> np.ndarray:
    """The models of ``nr_subints`` consecutive sub-integrations of ``subint_len`` spectra, the first beginning at spectrum
    ``first_sample``, for the phase ``phi0 + f0 t + f1 t^2 / 2`` turns at ``t`` seconds after spectrum 0.  Evaluated in exact
    rational arithmetic on the given floats and rounded once per member to the nearest 2^-64 turn: with ``tau = (first_sample
    + s subint_len) dt``, ``phase0 = frac(phi0 + f0 tau + f1 tau^2 / 2)``, ``step = f0 dt + f1 tau dt + f1 dt^2 / 2`` and
    ``accel = f1 dt^2``.  So the device's phase at spectrum ``k`` lies within ``(1 + k + k (k - 1) / 2) 2^-65`` turn of the
    exact one."""
    f0, f1, phi0, dt = Fraction(f0_hz), Fraction(f1_hz_per_s), Fraction(phase0_turns), Fraction(sample_time_s)
    if not 1 <= int(subint_len) <= MAX_SUBINT_LEN or int(nr_subints) < 0 or int(first_sample) < 0 or dt <= 0:
        raise ValueError("subint_len is 1 .. 2^24, nr_subints and first_sample are not negative, sample_time_s is positive")
    out = np.zeros(int(nr_subints), dtype=model_dtype)
    for s in range(int(nr_subints)):
        tau = (int(first_sample) + s * int(subint_len)) * dt
        out[s] = (_units(phi0 + f0 * tau + f1 * tau * tau / 2), _units(f0 * dt + f1 * tau * dt + f1 * dt * dt / 2), _units(f1 * dt * dt))
    return out


def advance(model, m: int):
    """The model ``m`` spectra on, ``{phi(m), step + m accel, accel}``, exactly modulo 2^64: its ``phi'(k)`` is ``phi(m + k)``.
    ``model`` is one element of a :data:`model_dtype` array (or any ``(phase0, step, accel)``); returns such an element."""
    names = getattr(getattr(model, "dtype", None), "names", None)
    phase0, step, accel = (int(model[n]) for n in names) if names else (int(x) for x in model)
    m = int(m)
    if m < 0:
        raise ValueError("m is not negative")
    out = np.zeros((), dtype=model_dtype)
    out[()] = ((phase0 + m * step + (m * (m - 1) // 2) * accel) % TURN, (step + m * accel) % TURN, accel % TURN)
    return out


def bin_of(phase, nbin: int):
    """``((phase >> 32) nbin) >> 32`` for a phase (an int, or a uint64 array) in units of 2^-64 turn: 0 .. nbin - 1."""
    if not 1 <= int(nbin) <= MAX_BINS:
        raise ValueError("nbin is 1 .. 1024")
    if isinstance(phase, np.ndarray):
        return (((phase.astype(np.uint64) >> np.uint64(32)) * np.uint64(nbin)) >> np.uint64(32)).astype(np.uint32)
    return (((int(phase) % TURN) >> 32) * int(nbin)) >> 32
