#!/usr/bin/env python3
"""An F-engine and a correlator on an MI355X, digitiser bytes to visibilities without leaving the device: a digitiser
stream with one CW tone per input -> the narrowband down-converter (include/dcs_ddc.h) -> the polyphase channeliser with 8-bit
requantisation (include/dcs_channeliser.h), whose output IS the sample tensor -> the correlator (include/dcs_correlator.h) ->
its integrator.

    python examples/f_engine.py

Every input carries a tone at its own offset from the mixing frequency.  The channel it must land in is predicted from the
down-converter's phase step and the channeliser's channel order (dc_sand_amd.ddc.phase_step, dc_sand_amd.channeliser
.channel_of); the check at the end is that every input's autocorrelation peaks in exactly that channel, far above the rest,
and that no component was clipped."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dc_sand_amd import BeamformerParameters, channeliser, ddc  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, memset, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, block_visibilities_bytes, channelised_bytes,  # noqa: E402
                                   channeliser_in_pairs, ddc_digits_bytes, ddc_out_bytes, nr_baselines, visibilities_bytes)

F_S, T, SCALE_BITS = 1712e6, 256, 5         # the digitiser's rate, the down-converter's taps and their scale
N, P, A, NS = 256, 8, 4, 64                 # channels, taps per branch, inputs (stations), spectra
ORDER = channeliser.ORDER_ASCENDING
F_MIX = 400e6
NR_OUT = channeliser_in_pairs(N, P, NS)     # the down-converter's outputs per row: the pairs the channeliser reads
SAMPLES = 16 * (NR_OUT - 1) + T
WIDTH = F_S / 16 / N                        # of a channel
TONE_BINS = (-60, -3, 0, 77)                # per input: its tone's offset from the mixing frequency in whole channels
require_device()
set_device(0)
params = BeamformerParameters(NR_CHANNELS=N, NR_STATIONS=A, NR_BEAMS=1, NR_SAMPLES_PER_CHANNEL=NS)
gen = SteeringCoefficientGenerator(params)

# the stream: one tone of amplitude 50 per input and a little seeded noise, rounded to int8
rng = np.random.default_rng(1)
t = np.arange(SAMPLES)
x = np.stack([np.rint(50.0 * np.cos(2 * np.pi * (F_MIX + k * WIDTH) / F_S * t + 0.7 * i) + rng.normal(0.0, 2.0, SAMPLES))
              for i, k in enumerate(TONE_BINS)]).astype(np.int8)

# the down-converter's low-pass (as examples/narrowband_ddc.py makes it) and its band
j = np.arange(T) - (T - 1) / 2
w = sum(a * np.cos(2 * np.pi * k * np.arange(T) / (T - 1)) for k, a in enumerate((0.35875, -0.48829, 0.14128, -0.01168)))
lowpass = np.sinc(2 * 0.45 / 16 * j) * w
h_ddc = ddc.integer_taps(np.rint(lowpass / lowpass.sum() * 1.4 * 131072) / 131072)
step = ddc.phase_step(F_MIX, F_S)
g_ddc, gain_ddc = ddc.band_taps(h_ddc, step, SCALE_BITS)

# where each tone must come out: its frequency in units of the phase step's 2^-32 of the sampling rate, less the mixer's,
# is its offset from the band centre; a channel is 2^32 / (16 N) of those units wide
units = [ddc.phase_step(F_MIX + k * WIDTH, F_S) - step for k in TONE_BINS]
bins = [int(round(u / (2 ** 32 / (16 * N)))) for u in units]
expected = [channeliser.channel_of(b, N, ORDER) for b in bins]

taps, twiddles = channeliser.pfb_taps(N, P), channeliser.twiddles(N)
# a tone of amplitude 50 comes out of the down-converter with amplitude 25 (a real tone is two complex ones) and of the
# filterbank, whose taps sum to 1, with the same: a gain of 4 puts it at 100 of 127
gains = np.full((A, N), 4.0, dtype=np.float32)

dbytes, ybytes = ddc_digits_bytes(T), ddc_out_bytes(A, NR_OUT)
abytes = channelised_bytes(N, NS // 16, A, q8=True)
vbytes, ibytes = block_visibilities_bytes(params, NS, NS // 16), visibilities_bytes(params, 1, 1)
d_x, d_g, d_digits, d_y = mem_alloc(x.nbytes), mem_alloc(g_ddc.nbytes), mem_alloc(dbytes), mem_alloc(ybytes)
d_taps, d_tw, d_gains, d_clip = mem_alloc(taps.nbytes), mem_alloc(twiddles.nbytes), mem_alloc(gains.nbytes), mem_alloc(8 * A)
d_ant, d_vis, d_int = mem_alloc(abytes), mem_alloc(vbytes), mem_alloc(ibytes)
memcpy_htod(d_x, x)
memcpy_htod(d_g, np.ascontiguousarray(g_ddc[None].astype(np.int32)))
memcpy_htod(d_taps, taps)
memcpy_htod(d_tw, twiddles)
memcpy_htod(d_gains, gains)
memset(d_clip, 0, 8 * A)

gen.ddc_tap_digits(d_g, T, 1, d_digits, dbytes)
gen.ddc(d_x, x.nbytes, SAMPLES, A, NR_OUT, d_digits, dbytes, T, [(step, 0, gain_ddc)], d_y, ybytes, NR_OUT)
gen.channelise_q8(d_y, ybytes, NR_OUT, A, NS, N, P, d_taps, d_tw, d_gains, d_ant, abytes, NS // 16, A, order=ORDER,
                  d_clip_count=d_clip)
gen.correlate_block(d_ant, abytes, d_vis, vbytes, NS, NS // 16)
gen.integrate_visibilities(d_vis, vbytes, 1, 1, d_int, ibytes)
synchronize()
vis, clipped = np.empty((1, N, nr_baselines(A), 2), np.float32), np.empty(A, np.uint64)
memcpy_dtoh(vis, d_int)
memcpy_dtoh(clipped, d_clip)

ok = not clipped.any()
print(f"{A} inputs x {SAMPLES} samples at {F_S / 1e6:.0f} MHz -> {NS} spectra of {N} channels of {WIDTH / 1e3:.1f} kHz; "
      f"clipped components: {clipped.tolist()}")
for i in range(A):
    auto = vis[0, :, i * (i + 1) // 2 + i, 0].astype(np.float64)  # baseline (i, i): the input's power per channel
    peak = int(auto.argmax())
    rest = 10 * np.log10(auto[peak] / max(np.delete(auto, peak).max(), 1.0))
    print(f"input {i}: tone {TONE_BINS[i]:+d} channels from {F_MIX / 1e6:.0f} MHz -> channel {peak} (expected {expected[i]}), "
          f"the next channel {rest:.1f} dB below; amplitude {np.sqrt(auto[peak] / NS):.1f}")
    ok &= peak == expected[i] and bool(rest > 20.0)
gen.close()
print("OK" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
