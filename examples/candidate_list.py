#!/usr/bin/env python3
"""From 8-bit filterbanks to a list of single-pulse candidates (include/dcs_candidates.h) on an MI355X: the chain of
examples/single_pulse_search.py with the sifter behind it,

    filterbank bytes -> dm_delays -> dedisperse_q8 -> dm_time_sums -> boxcar_peaks -> peak_snr -> find_candidates

Two dispersed pulses are put into the noise bytes: 8 spectra wide at two thirds of the DM range in beam 0, and 2 spectra
wide at a quarter of it in the last beam.  Each lights up its neighbouring DMs, widths and blocks of the signal-to-noise
plane; the sifter keeps, per neighbourhood of 8 DMs and 2 blocks, the one cell nothing beats.  What comes back from the
device is two count words and two records of 32 bytes.

    python examples/candidate_list.py [chan beams dms spectra]

The check at the end restates the sifter's contract in numpy (tests/helpers/candidates_model.py) on the planes the device
made: the list must agree bit for bit, and it must be exactly the two injected pulses at their DM rows and blocks."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, boxcar_peaks_bytes, candidate_dtype, candidates_bytes,  # noqa: E402
                                   candidates_workspace_bytes, dm_delays_bytes, dm_time_bytes, dm_time_sums_bytes,
                                   filterbank_bytes, peak_snr_bytes)
from helpers.candidates_model import find_candidates, same_bits  # noqa: E402
from helpers.dedisperse_model import dm_delays  # noqa: E402
from helpers.single_pulse_model import nr_blocks_of  # noqa: E402

C, B, NR_DM, T = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (256, 4, 64, 4096)
F0, F_TOP, TS = 830.0, 1500.0, 306.24e-6                       # MHz, MHz, seconds per spectrum
DF = (F_TOP - F0) / max(C - 1, 1)
BAND = (F_TOP, -DF, TS)                                        # per filterbank column: descending
DMS = np.linspace(0.0, 97.5, NR_DM)
WIDTHS = np.array([1, 2, 4, 8, 16, 32], np.uint32)
MAX_WIDTH, BLOCK_LEN = 32, 256
# (beam, DM index, first spectrum, spectra, height per byte)
PULSES = [(0, (2 * NR_DM) // 3, T // 3, 8, 24), (B - 1, NR_DM // 4, (2 * T) // 3, 2, 40)]
THRESHOLD, DM_RADIUS, BLOCK_RADIUS, MAX_CANDIDATES = 10.0, 8, 2, 16
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
gen = SteeringCoefficientGenerator(p)

table = dm_delays(C, *BAND, DMS)                               # int32 [NR_DM][C], per column
max_delay = int(table.max())
rows = T + max_delay                                           # the spectra a call of T outputs reads
x = np.random.default_rng(1).normal(128.0, 16.0, size=(B, rows, C))
for beam, m, t0, w, height in PULSES:
    for col in range(C):
        r = t0 + int(table[m, col])
        x[beam, r:r + w, col] += height
fb = np.clip(np.rint(x), 0, 255).astype(np.uint8)

nt = T - MAX_WIDTH + 1                                         # the times whose widest boxcar lies inside the plane
nb = nr_blocks_of(nt, BLOCK_LEN)
nfb, ndelays, nplane = filterbank_bytes(p, B, rows), dm_delays_bytes(p, NR_DM), dm_time_bytes(B, NR_DM, T)
nsums, npeaks, nsnr = dm_time_sums_bytes(B, NR_DM), boxcar_peaks_bytes(B, NR_DM, WIDTHS.size, nb), peak_snr_bytes(B, NR_DM, WIDTHS.size, nb)
ncands, nwork = candidates_bytes(MAX_CANDIDATES), candidates_workspace_bytes(B, NR_DM, nb)
d_fb, d_dms, d_delays, d_plane, d_widths = mem_alloc(nfb), mem_alloc(DMS.nbytes), mem_alloc(ndelays), mem_alloc(nplane), mem_alloc(WIDTHS.nbytes)
d_sums, d_peaks, d_snr = mem_alloc(nsums), mem_alloc(npeaks), mem_alloc(nsnr)
d_cands, d_count, d_work = mem_alloc(ncands), mem_alloc(8), mem_alloc(nwork)
memcpy_htod(d_fb, fb)
memcpy_htod(d_dms, DMS)
memcpy_htod(d_widths, WIDTHS)
gen.dm_delays(*BAND, d_dms, NR_DM, d_delays, ndelays)
gen.dedisperse_q8(d_fb, nfb, rows, 0, T, B, d_delays, NR_DM, max_delay, d_plane, nplane, T)
gen.dm_time_sums(d_plane, nplane, T, 0, T, B, NR_DM, d_sums, nsums)
gen.boxcar_peaks(d_plane, nplane, T, 0, nt, B, NR_DM, d_widths, WIDTHS.size, MAX_WIDTH, BLOCK_LEN, d_peaks, npeaks, nb)
gen.peak_snr(d_peaks, npeaks, nb, 0, nb, B, NR_DM, d_widths, WIDTHS.size, MAX_WIDTH, d_sums, nsums, T, d_snr, nsnr)
gen.find_candidates(d_snr, nsnr, d_peaks, npeaks, nb, 0, nb, B, NR_DM, WIDTHS.size, THRESHOLD, DM_RADIUS, BLOCK_RADIUS, d_cands, ncands,
                    MAX_CANDIDATES, d_count, d_work, nwork)
synchronize()

count, cands = np.empty(2, np.uint32), np.empty(MAX_CANDIDATES, candidate_dtype)
memcpy_dtoh(count, d_count)                                    # all a user of the search needs to copy: 8 bytes, then the records
memcpy_dtoh(cands, d_cands)
cands = cands[:count[1]]
got_peaks, got_snr = np.empty((B, NR_DM, WIDTHS.size, nb, 2), np.uint32), np.empty((B, NR_DM, WIDTHS.size, nb), np.float32)
memcpy_dtoh(got_peaks, d_peaks)                                # for the check alone
memcpy_dtoh(got_snr, d_snr)
exp, exp_count = find_candidates(got_snr, got_peaks, 0, nb, THRESHOLD, DM_RADIUS, BLOCK_RADIUS, MAX_CANDIDATES)
same = bool(np.array_equal(count, exp_count) and same_bits(cands, exp[:exp_count[1]]))
want = sorted((beam, m, t0 // BLOCK_LEN) for beam, m, t0, _, _ in PULSES)
found = bool(count.tolist() == [2, 2] and [(int(r["beam"]), int(r["dm"]), int(r["block"])) for r in cands] == want)
print(f"{B} beams x {NR_DM} DMs x {WIDTHS.size} widths x {nb} blocks of signal-to-noise ({nsnr} bytes) -> {int(count[0])} candidates "
      f"({int(count[1]) * candidate_dtype.itemsize} bytes) with threshold {THRESHOLD}, radii {DM_RADIUS} DMs and {BLOCK_RADIUS} blocks")
for r in cands:
    print(f"  beam {r['beam']}, DM {DMS[r['dm']]:.2f} (row {r['dm']}), width {int(WIDTHS[r['width_index']])}, spectrum {r['time']} "
          f"(block {r['block']}), S/N {r['snr']:.1f}, {r['members']} cells of its neighbourhood above the threshold")
print("bit-identical to the model:", same)
print("two candidates at the injected pulses:", found)
sys.exit(0 if same and found else 1)
