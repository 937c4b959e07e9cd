#!/usr/bin/env python3
"""Incoherent dedispersion (include/dcs_dedisperse.h) on an MI355X, from float spectra to the DM-time plane a search
thresholds:

    spectra -> spectra_sums -> filterbank_scales -> filterbank_q8 -> dm_delays -> dedisperse_q8

A dispersed pulse is put into noise spectra of beam 0: in every channel it arrives later by the delay of its DM, placed
with the same delay arithmetic (tests/helpers/dedisperse_model.py).  Channel c lies at f0 + c df and the bytes are written
in descending frequency order, so the band is stated per filterbank column: first f0 + (C - 1) df, step -df.

    python examples/dedispersed_pulse.py [chan beams dms spectra]

The check at the end restates both contracts in numpy on the bytes the device made: the delay table and the plane must
agree bit for bit, and the plane's maximum must lie at the injected DM and time."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, dm_delays_bytes, dm_time_bytes, filterbank_bytes,  # noqa: E402
                                   filterbank_scales_bytes, spectra_sums_bytes)
from helpers.dedisperse_model import dedisperse, dm_delays  # noqa: E402

C, B, NR_DM, T = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (256, 4, 64, 4096)
F0, F_TOP, TS = 830.0, 1500.0, 306.24e-6                       # MHz, MHz, seconds per spectrum
DF = (F_TOP - F0) / max(C - 1, 1)
BAND = (F0 + (C - 1) * DF, -DF, TS)                            # per filterbank column: descending
DMS = np.linspace(0.0, 97.5, NR_DM)
M_PULSE, T_PULSE = (2 * NR_DM) // 3, T // 3
TARGET_STD, LEVEL = 24.0, 128.0
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
gen = SteeringCoefficientGenerator(p)

table = dm_delays(C, *BAND, DMS)                               # int32 [NR_DM][C], per column
max_delay = int(table.max())
rows = T + max_delay                                           # the spectra a call of T outputs reads
rng = np.random.default_rng(1)
spectra = (1000.0 * (1.0 + 0.05 * rng.standard_normal((rows, C, B)))).astype(np.float32)
for ch in range(C):                                            # channel ch is column C - 1 - ch
    spectra[T_PULSE + table[M_PULSE, C - 1 - ch], ch, 0] += 200.0  # four standard deviations

xbytes = spectra.nbytes
nsums, nscales, nfb = spectra_sums_bytes(p, B), filterbank_scales_bytes(p, B), filterbank_bytes(p, B, rows)
ndelays, nplane = dm_delays_bytes(p, NR_DM), dm_time_bytes(B, NR_DM, T)
d_x, d_sums, d_scales, d_fb = mem_alloc(xbytes), mem_alloc(nsums), mem_alloc(nscales), mem_alloc(nfb)
d_dms, d_delays, d_plane = mem_alloc(DMS.nbytes), mem_alloc(ndelays), mem_alloc(nplane)
memcpy_htod(d_x, spectra)
memcpy_htod(d_dms, DMS)
gen.spectra_sums(d_x, xbytes, rows, B, d_sums, nsums)
gen.filterbank_scales(d_sums, nsums, rows, B, TARGET_STD, d_scales, nscales)
gen.filterbank_q8(d_x, xbytes, rows, B, d_scales, LEVEL, d_fb, nfb, rows, descending=True)
gen.dm_delays(*BAND, d_dms, NR_DM, d_delays, ndelays)
gen.dedisperse_q8(d_fb, nfb, rows, 0, T, B, d_delays, NR_DM, max_delay, d_plane, nplane, T)
synchronize()

fb, delays, plane = np.empty((B, rows, C), np.uint8), np.empty((NR_DM, C), np.int32), np.empty((B, NR_DM, T), np.uint32)
for host, dev in ((fb, d_fb), (delays, d_delays), (plane, d_plane)):
    memcpy_dtoh(host, dev)
same = bool(np.array_equal(delays, table) and np.array_equal(plane, dedisperse(fb, table, 0, T, max_delay)))
m, t = np.unravel_index(int(np.argmax(plane[0])), plane[0].shape)
noise = plane[1] if B > 1 else plane[0, 0]
found = bool((m, t) == (M_PULSE, T_PULSE))
print(f"{B} beams x {C} columns x {rows} spectra, {NR_DM} DMs to {DMS[-1]:.1f} (delays to {max_delay} spectra): plane uint32 "
      f"[{B}][{NR_DM}][{T}], noise mean {noise.mean():.1f}, standard deviation {noise.std():.1f}")
print(f"pulse at DM {DMS[M_PULSE]:.2f}, spectrum {T_PULSE}: maximum {int(plane[0, m, t])} at DM {DMS[m]:.2f}, spectrum {t}, "
      f"{(int(plane[0, m, t]) - noise.mean()) / noise.std():.1f} standard deviations above the noise")
print("bit-identical to the model:", same)
print("the maximum lies at the injected DM and time:", found)
sys.exit(0 if same and found else 1)
