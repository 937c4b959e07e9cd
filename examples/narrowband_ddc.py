#!/usr/bin/env python3
"""The narrowband digital down-converter (include/dcs_ddc.h) on an MI355X: two bands, mixed at 100 MHz and at 300 MHz, of one
digitiser stream at 1712 MHz that holds four tones, each filtered by a 256-tap low-pass (a windowed sinc made here, integers
over 2^17 as an F-engine's coefficient files are) and decimated by 16 to 107 MHz.

    python examples/narrowband_ddc.py [samples]

Prints, per band, the bin of a 1024-point spectrum in which each in-band tone lands and how far below the tones the strongest
other bin lies (what the filter leaves of the out-of-band tones, and the int8 quantisation's spurs).  The checks at the end:
every tone is in the bin its frequency says, the rest is more than 50 dB down, and the stream processed in three calls, with
first_output carried, gives the bits of one call."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters, ddc  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import SteeringCoefficientGenerator, ddc_digits_bytes, ddc_out_bytes  # noqa: E402

F_S, T, FFT, SCALE_BITS = 1712e6, 256, 1024, 5
N = int(sys.argv[1]) if len(sys.argv) > 1 else 16 * (2 * FFT - 1) + T
NR_OUT = (N - T) // 16 + 1
assert NR_OUT >= 2 * FFT
WIDTH = F_S / 16 / FFT                                       # of a bin of the decimated spectrum
MIX = (100e6, 300e6)
# per band, the offsets of its tones from the mixing frequency in whole bins; the other band's tones are out of band for it
TONE_BINS = ((0, 37), (-101, 200))
require_device()
set_device(0)
gen = SteeringCoefficientGenerator(BeamformerParameters(NR_CHANNELS=1, NR_STATIONS=1, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=16))

# the stream: four tones of amplitude 30, rounded to int8, in a row 16-byte aligned and a multiple of 16 long
t = np.arange(N)
freqs = [MIX[b] + k * WIDTH for b in range(2) for k in TONE_BINS[b]]
x = np.rint(sum(30.0 * np.cos(2 * np.pi * f / F_S * t + 0.3 * i) for i, f in enumerate(freqs))).astype(np.int8)
in_stride = -(-N // 16) * 16
row = np.zeros(in_stride, dtype=np.int8)
row[:N] = x

# the low-pass: a Blackman-Harris windowed sinc with its cutoff at 0.4 of the output band, as integers over 2^17
j = np.arange(T) - (T - 1) / 2
w = np.zeros(T)
for a, k in zip((0.35875, -0.48829, 0.14128, -0.01168), range(4)):
    w += a * np.cos(2 * np.pi * k * np.arange(T) / (T - 1))
lowpass = np.sinc(2 * 0.4 / 16 * j) * w
h = ddc.integer_taps(np.rint(lowpass / lowpass.sum() * 1.4 * 131072) / 131072)
steps = [ddc.phase_step(f, F_S) for f in MIX]
designs = [ddc.band_taps(h, s, SCALE_BITS) for s in steps]
taps = np.stack([g for g, _ in designs]).astype(np.int32)    # [band][T][{re, im}]
bands = [(s, 0, gain) for s, (_, gain) in zip(steps, designs)]

dbytes, obytes = ddc_digits_bytes(T), ddc_out_bytes(1, NR_OUT, 2)
d_x, d_taps, d_digits, d_out, d_parts = mem_alloc(in_stride), mem_alloc(taps.nbytes), mem_alloc(dbytes), mem_alloc(obytes), mem_alloc(obytes)
memcpy_htod(d_x, row)
memcpy_htod(d_taps, taps)
gen.ddc_tap_digits(d_taps, T, 2, d_digits, dbytes)
gen.ddc(d_x, in_stride, in_stride, 1, NR_OUT, d_digits, dbytes, T, bands, d_out, obytes, NR_OUT)
# the same stream in three calls: outputs [0, c1), [c1, c2), [c2, NR_OUT), each from its first sample on
cuts = (0, NR_OUT // 3, NR_OUT // 3 + 1001, NR_OUT)
for lo, hi in zip(cuts[:-1], cuts[1:]):
    gen.ddc(int(d_x) + 16 * lo, in_stride - 16 * lo, in_stride - 16 * lo, 1, hi - lo, d_digits, dbytes, T, bands,
            int(d_parts) + 8 * lo, obytes - 8 * lo, NR_OUT, first_output=lo)
synchronize()
out, parts = np.empty((2, 1, NR_OUT, 2), np.float32), np.empty((2, 1, NR_OUT, 2), np.float32)
memcpy_dtoh(out, d_out)
memcpy_dtoh(parts, d_parts)

ok = bool(np.array_equal(out.view(np.uint32), parts.view(np.uint32)))
print(f"{N} samples at {F_S / 1e6:.0f} MHz -> {NR_OUT} outputs at {F_S / 16e6:.0f} MHz per band; three calls give the bits of one: {ok}")
for b in range(2):
    y = out[b, 0, -FFT:, 0].astype(np.float64) + 1j * out[b, 0, -FFT:, 1]
    p = np.abs(np.fft.fft(y * np.blackman(FFT))) ** 2
    want = sorted(k % FFT for k in TONE_BINS[b])
    near = sorted({(k + d) % FFT for k in want for d in (-2, -1, 0, 1, 2)})  # the window's main lobe
    top = sorted(np.argsort(p)[-2:].tolist())
    rejection = 10 * np.log10(p[want].min() / np.delete(p, near).max())
    print(f"band {b}: mixed at {MIX[b] / 1e6:.0f} MHz, tones in bins {top} (expected {want}), everything else {rejection:.1f} dB below")
    ok &= top == want and bool(rejection > 50.0)
gen.close()
print("OK" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
