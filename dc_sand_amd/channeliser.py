"""Host-side design of the polyphase channeliser (include/dcs_channeliser.h): the twiddle table of its butterfly network, the
prototype filter of a polyphase filterbank, and the channel an FFT bin comes out in.  What
:meth:`dc_sand_amd.generator.SteeringCoefficientGenerator.channelise` and ``.channelise_q8`` take as ``d_twiddles`` and
``d_taps``.  numpy only; needs no built library and no device.
"""
from __future__ import annotations

import numpy as np

MIN_CHANNELS, MAX_CHANNELS, MAX_TAPS = 64, 2048, 16
ORDER_FFT, ORDER_ASCENDING = 0, 1


def _check_channels(N) -> int:
    if int(N) != N or not MIN_CHANNELS <= N <= MAX_CHANNELS or int(N) & (int(N) - 1):
        raise ValueError(f"N must be a power of two in [{MIN_CHANNELS}, {MAX_CHANNELS}]")
    return int(N)


def twiddles(N: int) -> np.ndarray:
    """``float32 [N / 2][{re, im}]``: entry ``j`` is ``(cos, -sin)`` of ``2 pi j / N``, evaluated in fp64 and rounded to fp32;
    entries 0 and ``N / 4``, which the network never uses, are exactly ``(1, 0)`` and ``(0, -1)``.  With this table the
    network is the DFT ``X[k] = sum_r y[r] e^(-2 pi i k r / N)``."""
    N = _check_channels(N)
    ang = 2.0 * np.pi * np.arange(N // 2, dtype=np.float64) / N
    w = np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)
    w[0] = (1.0, 0.0)
    w[N // 4] = (0.0, -1.0)
    return w


def pfb_taps(N: int, P: int, w_cutoff: float = 1.0) -> np.ndarray:
    """``float32 [P N]``: the prototype low-pass of a polyphase filterbank of ``N`` channels and ``P`` taps per branch, a Hann
    window of length ``P N`` times ``sinc(w_cutoff (i - (P N - 1) / 2) / N)`` (``sinc(x) = sin(pi x) / (pi x)``), made exactly
    symmetric and normalised to ``sum h = 1`` in fp64, then rounded to fp32.  Tap ``p N + r`` multiplies pair ``(n + p) N + r``
    of spectrum ``n``; ``w_cutoff`` scales the channel width (1: channels that cross at the half-channel point)."""
    N = _check_channels(N)
    if int(P) != P or not 1 <= P <= MAX_TAPS:
        raise ValueError(f"P must be in [1, {MAX_TAPS}]")
    if not (np.isfinite(w_cutoff) and w_cutoff > 0.0):
        raise ValueError("w_cutoff must be finite and positive")
    M = int(P) * N
    i = np.arange(M, dtype=np.float64)
    h = np.hanning(M) * np.sinc(float(w_cutoff) * (i - (M - 1) / 2.0) / N)
    h = 0.5 * (h + h[::-1])  # exactly symmetric, whatever the evaluation of either half
    return (h / h.sum()).astype(np.float32)


def channel_of(k, N: int, order: int = ORDER_FFT):
    """The output channel of FFT bin ``k`` (any integer or integer array, taken modulo ``N``: bin -1 is bin ``N - 1``):
    ``k`` for ``order`` 0, ``(k + N / 2) mod N`` for ``order`` 1, which ascends in frequency from ``-N / 2`` to ``N / 2 - 1``."""
    N = _check_channels(N)
    if order not in (ORDER_FFT, ORDER_ASCENDING):
        raise ValueError("order must be 0 or 1")
    k = np.asarray(k)
    if not np.issubdtype(k.dtype, np.integer):
        raise ValueError("k must be an integer")
    c = (k + (N // 2 if order else 0)) % N
    return int(c) if c.ndim == 0 else c
