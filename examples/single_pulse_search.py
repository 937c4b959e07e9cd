#!/usr/bin/env python3
"""A single-pulse search (include/dcs_single_pulse.h) on an MI355X, from 8-bit filterbanks to the cell of the search that
holds a pulse:

    filterbank bytes -> dm_delays -> dedisperse_q8 -> dm_time_sums -> boxcar_peaks -> peak_snr

A dispersed pulse of 8 spectra is put into the noise bytes of beam 0: in every column it arrives later by the delay of its
DM (tests/helpers/dedisperse_model.py).  The planes stay on the device; what comes back is the peak plane, a few hundred
times smaller, with the signal-to-noise of every (beam, DM, width, block of 256 spectra) and the best width per block.

    python examples/single_pulse_search.py [chan beams dms spectra]

The check at the end restates the contracts in numpy on the planes the device made: sums, peaks and signal-to-noise must
agree bit for bit, and the largest signal-to-noise must lie at the injected DM, width and time."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, best_width_bytes, boxcar_peaks_bytes, dm_delays_bytes,  # noqa: E402
                                   dm_time_bytes, dm_time_sums_bytes, filterbank_bytes, peak_snr_bytes)
from helpers.dedisperse_model import dm_delays  # noqa: E402
from helpers.single_pulse_model import nr_blocks_of, peaks, snr, sums  # noqa: E402

C, B, NR_DM, T = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (256, 4, 64, 4096)
F0, F_TOP, TS = 830.0, 1500.0, 306.24e-6                       # MHz, MHz, seconds per spectrum
DF = (F_TOP - F0) / max(C - 1, 1)
BAND = (F_TOP, -DF, TS)                                        # per filterbank column: descending
DMS = np.linspace(0.0, 97.5, NR_DM)
WIDTHS = np.array([1, 2, 4, 8, 16, 32], np.uint32)
MAX_WIDTH, BLOCK_LEN = 32, 256
M_PULSE, T_PULSE, W_PULSE, HEIGHT = (2 * NR_DM) // 3, T // 3, 8, 24
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
gen = SteeringCoefficientGenerator(p)

table = dm_delays(C, *BAND, DMS)                               # int32 [NR_DM][C], per column
max_delay = int(table.max())
rows = T + max_delay                                           # the spectra a call of T outputs reads
x = np.random.default_rng(1).normal(128.0, 16.0, size=(B, rows, C))
for col in range(C):
    r = T_PULSE + int(table[M_PULSE, col])
    x[0, r:r + W_PULSE, col] += HEIGHT                         # one and a half standard deviations per byte
fb = np.clip(np.rint(x), 0, 255).astype(np.uint8)

nt = T - MAX_WIDTH + 1                                         # the times whose widest boxcar lies inside the plane
nb = nr_blocks_of(nt, BLOCK_LEN)
nfb, ndelays, nplane = filterbank_bytes(p, B, rows), dm_delays_bytes(p, NR_DM), dm_time_bytes(B, NR_DM, T)
nsums, npeaks = dm_time_sums_bytes(B, NR_DM), boxcar_peaks_bytes(B, NR_DM, WIDTHS.size, nb)
nsnr, nbest = peak_snr_bytes(B, NR_DM, WIDTHS.size, nb), best_width_bytes(B, NR_DM, nb)
d_fb, d_dms, d_delays, d_plane, d_widths = mem_alloc(nfb), mem_alloc(DMS.nbytes), mem_alloc(ndelays), mem_alloc(nplane), mem_alloc(WIDTHS.nbytes)
d_sums, d_peaks, d_snr, d_best = mem_alloc(nsums), mem_alloc(npeaks), mem_alloc(nsnr), mem_alloc(nbest)
memcpy_htod(d_fb, fb)
memcpy_htod(d_dms, DMS)
memcpy_htod(d_widths, WIDTHS)
gen.dm_delays(*BAND, d_dms, NR_DM, d_delays, ndelays)
gen.dedisperse_q8(d_fb, nfb, rows, 0, T, B, d_delays, NR_DM, max_delay, d_plane, nplane, T)
gen.dm_time_sums(d_plane, nplane, T, 0, T, B, NR_DM, d_sums, nsums)
gen.boxcar_peaks(d_plane, nplane, T, 0, nt, B, NR_DM, d_widths, WIDTHS.size, MAX_WIDTH, BLOCK_LEN, d_peaks, npeaks, nb)
gen.peak_snr(d_peaks, npeaks, nb, 0, nb, B, NR_DM, d_widths, WIDTHS.size, MAX_WIDTH, d_sums, nsums, T, d_snr, nsnr, d_best, nbest)
synchronize()

plane, got_sums = np.empty((B, NR_DM, T), np.uint32), np.empty((B, NR_DM, 2), np.uint64)
got_peaks, got_snr = np.empty((B, NR_DM, WIDTHS.size, nb, 2), np.uint32), np.empty((B, NR_DM, WIDTHS.size, nb), np.float32)
got_best = np.empty((B, NR_DM, nb), np.uint32)
for host, dev in ((plane, d_plane), (got_sums, d_sums), (got_peaks, d_peaks), (got_snr, d_snr), (got_best, d_best)):
    memcpy_dtoh(host, dev)
exp_sums, exp_peaks = sums(plane, 0, T), peaks(plane, 0, nt, WIDTHS, MAX_WIDTH, BLOCK_LEN)
exp_snr, exp_best = snr(exp_peaks, WIDTHS, MAX_WIDTH, exp_sums, T)
same = bool(np.array_equal(got_sums, exp_sums) and np.array_equal(got_peaks, exp_peaks) and np.array_equal(got_best, exp_best)
            and np.array_equal(got_snr.view(np.uint32), exp_snr.view(np.uint32)))
b, m, i, k = (int(v) for v in np.unravel_index(int(np.argmax(got_snr)), got_snr.shape))
t = int(got_peaks[b, m, i, k, 1])
found = bool((b, m, int(WIDTHS[i]), t) == (0, M_PULSE, W_PULSE, T_PULSE) and int(got_best[b, m, k]) == i and k == T_PULSE // BLOCK_LEN)
others = np.delete(got_snr[0], M_PULSE, axis=0)
print(f"{B} beams x {NR_DM} DMs x {T} spectra of planes ({nplane} bytes) -> peaks uint32 [{B}][{NR_DM}][{WIDTHS.size}][{nb}][2] "
      f"({npeaks} bytes), signal-to-noise and best width ({nsnr + nbest} bytes)")
print(f"pulse at DM {DMS[M_PULSE]:.2f}, width {W_PULSE}, spectrum {T_PULSE}: recovered DM {DMS[m]:.2f}, width {int(WIDTHS[i])}, "
      f"spectrum {t} (block {k}), S/N {got_snr[b, m, i, k]:.1f}; the best at any other DM of the beam: {others.max():.1f}")
print("bit-identical to the model:", same)
print("the pulse is recovered:", found)
sys.exit(0 if same and found else 1)
