#!/usr/bin/env python3
"""RFI excision (include/dcs_rfi.h) in front of a single-pulse search on an MI355X:

    filterbank bytes -> rfi_moments -> rfi_flags -> rfi_clean_q8 -> dm_delays / dedisperse_q8
                     -> dm_time_sums / boxcar_peaks / peak_snr

The filterbank is noise as filterbank_q8 leaves it (mean 128, standard deviation 16 in every channel) with four plants: a
channel of doubled noise, a dead channel, a broadband burst of four spectra, and a dispersed pulse of eight spectra, weaker
per sample than the burst.  The search runs twice, on the bytes as they are and on the cleaned bytes.  Without the cleaning
the burst is the strongest peak of the search, in the DM 0 series, and a candidate list would begin with it; with it the
flagged spectra hold the channels' mean, the burst is gone, and the strongest peak is the pulse at its DM and time.

    python examples/rfi_excision.py

The script asserts both and prints one summary line."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, memset, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (RfiThresholds, SteeringCoefficientGenerator, boxcar_peaks_bytes, dm_delays_bytes,  # noqa: E402
                                   dm_time_bytes, dm_time_sums_bytes, filterbank_bytes, peak_snr_bytes, rfi_cell_flags_bytes,
                                   rfi_cell_sums_bytes, rfi_channel_mask_bytes, rfi_counts_bytes, rfi_spectrum_flags_bytes,
                                   rfi_zero_dm_bytes)
from helpers.dedisperse_model import dm_delays  # noqa: E402
from helpers.single_pulse_model import nr_blocks_of  # noqa: E402

C, B, NR_DM, T = 256, 1, 32, 2048
F_TOP, F0, TS = 1500.0, 830.0, 306.24e-6                       # MHz, MHz, seconds per spectrum
BAND = (F_TOP, -(F_TOP - F0) / (C - 1), TS)                    # per filterbank column: descending
DMS = np.linspace(0.0, 97.5, NR_DM)
WIDTHS = np.array([1, 2, 4, 8, 16, 32], np.uint32)
MAX_WIDTH, PEAK_BLOCK, RFI_BLOCK, LEVEL = 32, 256, 64, 128.0
LOUD, DEAD = 37, 90                                            # the channels of doubled noise and of none
T_BURST, W_BURST, H_BURST = 1500, 4, 10                        # a broadband burst: every channel at once
M_PULSE, T_PULSE, W_PULSE, H_PULSE = 20, 600, 8, 4             # a dispersed pulse, a quarter of a standard deviation per byte


def make_filterbank(rows, table):
    rng = np.random.default_rng(20261021)
    x = rng.normal(LEVEL, 16.0, size=(B, rows, C))
    x[0, :, LOUD] = rng.normal(LEVEL, 32.0, size=rows)
    x[0, :, DEAD] = LEVEL
    x[0, T_BURST:T_BURST + W_BURST, :] += H_BURST
    for col in range(C):
        r = T_PULSE + int(table[M_PULSE, col])
        x[0, r:r + W_PULSE, col] += H_PULSE
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def strongest(snr, peaks):
    """(DM index, width, time, signal-to-noise) of the largest signal-to-noise of beam 0."""
    m, i, k = (int(v) for v in np.unravel_index(int(np.argmax(snr[0])), snr[0].shape))
    return m, int(WIDTHS[i]), int(peaks[0, m, i, k, 1]), float(snr[0, m, i, k])


def main():
    require_device()
    set_device(0)
    p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
    gen = SteeringCoefficientGenerator(p)
    table = dm_delays(C, *BAND, DMS)
    max_delay = int(table.max())
    nr_blocks = (T + max_delay + RFI_BLOCK - 1) // RFI_BLOCK     # the RFI window: every row that the search reads
    rows = nr_blocks * RFI_BLOCK
    fb = make_filterbank(rows, table)

    nt = T - MAX_WIDTH + 1
    nb = nr_blocks_of(nt, PEAK_BLOCK)
    nfb, ndelays, nplane = filterbank_bytes(p, B, rows), dm_delays_bytes(p, NR_DM), dm_time_bytes(B, NR_DM, T)
    nsums, npeaks, nsnr = dm_time_sums_bytes(B, NR_DM), boxcar_peaks_bytes(B, NR_DM, WIDTHS.size, nb), peak_snr_bytes(B, NR_DM, WIDTHS.size, nb)
    ncs, nz = rfi_cell_sums_bytes(p, B, nr_blocks), rfi_zero_dm_bytes(B, rows)
    ncf, ncm, nsf, ncnt = rfi_cell_flags_bytes(p, B, nr_blocks), rfi_channel_mask_bytes(p, B), rfi_spectrum_flags_bytes(B, rows), rfi_counts_bytes(B)
    d_fb, d_clean, d_dms, d_delays, d_widths = mem_alloc(nfb), mem_alloc(nfb), mem_alloc(DMS.nbytes), mem_alloc(ndelays), mem_alloc(WIDTHS.nbytes)
    d_plane, d_sums, d_peaks, d_snr = mem_alloc(nplane), mem_alloc(nsums), mem_alloc(npeaks), mem_alloc(nsnr)
    d_cs, d_z, d_cf, d_cm, d_sf, d_cnt, d_rep = (mem_alloc(n) for n in (ncs, nz, ncf, ncm, nsf, ncnt, 8 * B))
    memcpy_htod(d_fb, fb)
    memcpy_htod(d_dms, DMS)
    memcpy_htod(d_widths, WIDTHS)
    memset(d_rep, 0, 8 * B)
    gen.dm_delays(*BAND, d_dms, NR_DM, d_delays, ndelays)

    # the RFI stage: statistics, flags (6 MADs everywhere; a channel goes with more than 2 bad blocks), cleaned bytes
    gen.rfi_moments(d_fb, nfb, rows, 0, nr_blocks, RFI_BLOCK, B, d_cs, ncs, d_z, nz)
    gen.rfi_flags(d_cs, ncs, nr_blocks, RFI_BLOCK, B, d_cf, ncf, d_cm, ncm, d_cnt, ncnt, thresholds=RfiThresholds(max_bad_blocks=2),
                  d_zero_dm=d_z, zero_dm_bytes=nz, d_spectrum_flags=d_sf, spectrum_flags_bytes=nsf)
    gen.rfi_clean_q8(d_fb, nfb, rows, 0, nr_blocks, RFI_BLOCK, B, int(np.rint(LEVEL)), d_clean, nfb, rows, d_cell_flags=d_cf,
                     d_channel_mask=d_cm, d_spectrum_flags=d_sf, d_replaced=d_rep)

    def search(d_bytes):
        gen.dedisperse_q8(d_bytes, nfb, rows, 0, T, B, d_delays, NR_DM, max_delay, d_plane, nplane, T)
        gen.dm_time_sums(d_plane, nplane, T, 0, T, B, NR_DM, d_sums, nsums)
        gen.boxcar_peaks(d_plane, nplane, T, 0, nt, B, NR_DM, d_widths, WIDTHS.size, MAX_WIDTH, PEAK_BLOCK, d_peaks, npeaks, nb)
        gen.peak_snr(d_peaks, npeaks, nb, 0, nb, B, NR_DM, d_widths, WIDTHS.size, MAX_WIDTH, d_sums, nsums, T, d_snr, nsnr)
        synchronize()
        peaks, snr = np.empty((B, NR_DM, WIDTHS.size, nb, 2), np.uint32), np.empty((B, NR_DM, WIDTHS.size, nb), np.float32)
        memcpy_dtoh(peaks, d_peaks)
        memcpy_dtoh(snr, d_snr)
        return strongest(snr, peaks)

    raw, cleaned = search(d_fb), search(d_clean)
    mask, spectrum, counts, replaced = np.empty((B, C), np.uint8), np.empty((B, rows), np.uint8), np.empty((B, 3), np.uint32), np.empty(B, np.uint64)
    for host, dev in ((mask, d_cm), (spectrum, d_sf), (counts, d_cnt), (replaced, d_rep)):
        memcpy_dtoh(host, dev)
    gen.close()

    burst_found = raw[0] == 0 and T_BURST - raw[1] < raw[2] < T_BURST + W_BURST
    pulse_found = cleaned[0] == M_PULSE and abs(cleaned[2] - T_PULSE) <= 2
    flagged_right = (np.flatnonzero(mask[0] == 0).tolist() == [LOUD, DEAD]
                     and np.flatnonzero(spectrum[0]).tolist() == list(range(T_BURST, T_BURST + W_BURST)))
    print(f"RFI excision of {B} x {rows} x {C} bytes: {int(counts[0, 0])} cells, channels {np.flatnonzero(mask[0] == 0).tolist()} and "
          f"spectra {np.flatnonzero(spectrum[0]).tolist()} flagged, {int(replaced[0])} bytes replaced; "
          f"without cleaning the strongest peak is the burst at DM 0: {burst_found} (DM index {raw[0]}, width {raw[1]}, spectrum {raw[2]}, "
          f"S/N {raw[3]:.1f}); with cleaning it is the pulse: {pulse_found} (DM index {cleaned[0]}, width {cleaned[1]}, spectrum "
          f"{cleaned[2]}, S/N {cleaned[3]:.1f}; planted at DM index {M_PULSE}, width {W_PULSE}, spectrum {T_PULSE})")
    assert burst_found, raw
    assert pulse_found, cleaned
    assert flagged_right
    return 0


if __name__ == "__main__":
    sys.exit(main())
