"""Host-side design of the narrowband digital down-converter (include/dcs_ddc.h): the oscillator's 32-bit phase step, the
integers behind a printed low-pass design, and the complex band-pass integer taps with their gain that
:meth:`dc_sand_amd.generator.SteeringCoefficientGenerator.ddc_tap_digits` and ``.ddc`` take.  numpy only; needs no built
library and no device.

The mixer folds into the filter: ``sum_j h[j] x[n + j] e^(-i w (n + j)) = e^(-i w n) sum_j (h[j] e^(-i w j)) x[n + j]``.  The
taps ``g[j] = rint(h[j] 2^s e^(-i w j))`` are fixed integers, the sum over the raw int8 samples is exact, and the rotation
``e^(-i w n)`` is a phase accumulator of 32 bits: ``w = 2 pi phase_step / 2^32`` per input sample.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

DECIMATION = 16
MAX_ABS_TAP = 127 * 65793  # 8 355 711: three balanced base-256 digits hold every integer up to it exactly
MAX_ABS_SUM = (1 << 24) - 1  # sum_j |g[j]| per component: no int8 input can then take a sum out of int32


def phase_step(f_mix, f_s) -> int:
    """The 32-bit phase step per input sample of a mixing frequency: ``rint(f_mix / f_s 2^32) mod 2^32``, the quotient taken
    exactly (both frequencies as the rationals their floats or integers are).  Negative frequencies wrap."""
    q = Fraction(f_mix) / Fraction(f_s) * (1 << 32)
    return int(round(q)) % (1 << 32)


def integer_taps(values, bits: int = 17) -> np.ndarray:
    """The integers ``h`` behind a printed filter design ``c = h / 2^bits`` (the reference's coefficient files are integers
    over 2^17 printed to five significant digits): ``rint(c 2^bits)`` as int64.  Raises if a value is further than 0.1 from
    its integer: then the design is no such print."""
    c = np.asarray(values, dtype=np.float64).reshape(-1)
    scaled = c * float(1 << bits)
    h = np.rint(scaled)
    residue = float(np.max(np.abs(scaled - h))) if c.size else 0.0
    if not residue <= 0.1:
        raise ValueError(f"values are no integers over 2^{bits}: residue {residue:.3f} > 0.1")
    return h.astype(np.int64)


def band_taps(h, step: int, scale_bits: int):
    """``(taps, gain)`` of one band: ``taps`` int32 ``[T][{re, im}]`` in correlation order (tap ``j`` multiplies sample
    ``16 m + j``) with ``re = rint(h[j] 2^s cos(w j))`` and ``im = -rint(h[j] 2^s sin(w j))``, ``w j = 2 pi (j step mod 2^32) /
    2^32`` computed in fp64, and ``gain = 1 / (sum(h) 2^s)`` so that a tone at the mixing frequency comes out with the
    amplitude it went in with, halved (a real tone is two complex ones).  ``h`` are integers in correlation order.  Raises if
    ``sum |g|`` of a component exceeds 2^24 - 1 -- the bound under which the kernel's int32 sums cannot wrap -- or a tap
    leaves the exact digit range."""
    h = np.asarray(h)
    if h.ndim != 1 or not np.issubdtype(h.dtype, np.integer):
        raise ValueError("h must be a vector of integers")
    hsum = int(h.astype(object).sum()) if h.size else 0
    if hsum == 0:
        raise ValueError("sum(h) is zero: the gain is undefined")
    j = np.arange(h.size, dtype=np.uint64)
    turns = ((j * np.uint64(int(step) % (1 << 32))) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
    amp = h.astype(np.float64) * float(1 << int(scale_bits))
    g = np.stack([np.rint(amp * np.cos(2.0 * np.pi * turns)), -np.rint(amp * np.sin(2.0 * np.pi * turns))], axis=1)
    if np.abs(g).max(initial=0.0) > MAX_ABS_TAP:
        raise ValueError(f"a tap exceeds {MAX_ABS_TAP}: lower scale_bits")
    if np.abs(g).sum(axis=0).max(initial=0.0) > MAX_ABS_SUM:
        raise ValueError("sum |g| of a component exceeds 2^24 - 1: lower scale_bits")
    return g.astype(np.int32), 1.0 / (float(hsum) * float(1 << int(scale_bits)))
