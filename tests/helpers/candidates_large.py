"""The shape of tests/test_gpu_candidates_large.py, and what the host can say about planes that exist on the device only.
tests/test_candidates_large_plan.py walks the same plan without a device and shows that an offset into d_snr or d_peaks
worked out in 32 bits gives another list.

The shape is that of the signal-to-noise test of helpers/single_pulse_large.py, the smallest of this suite at which d_snr
passes 2^32 bytes: 4 DMs, 4 widths, peak_blocks = 2^26 + 256, so 4,294,983,680 bytes of signal-to-noise and twice that of
peaks.  The call takes the last NR_BLOCKS blocks of every (DM, width) row.  Of the 16 rows of d_snr the last one's window
lies past the line; of d_peaks the windows of the last nine do.  The planes are a byte fill (one memset each: no kernel of
the tests) with the windows copied in; SNR_DECOY is copied where a 32-bit offset into d_snr would land."""
import numpy as np

from helpers import large_tensor as lt
from helpers.candidates_model import find_candidates, seeded_planes

B, NR_DM, NR_WIDTHS, PEAK_BLOCKS, NR_BLOCKS = 1, 4, 4, (1 << 26) + 256, 128
FIRST_BLOCK = PEAK_BLOCKS - NR_BLOCKS
THRESHOLD, RADII, MAX_CANDIDATES = 6.0, (1, 1), 256
SNR_BYTES, PEAKS_BYTES = B * NR_DM * NR_WIDTHS * PEAK_BLOCKS * 4, B * NR_DM * NR_WIDTHS * PEAK_BLOCKS * 8
FILL = 0xA5                       # every byte outside the windows: as a float -2.9e-16, below the threshold
FILL_WORD = 0xA5A5A5A5
FILL_FLOAT = np.frombuffer(bytes([FILL] * 4), np.float32)[0]
SNR_DECOY = np.float32(50.0)      # where the window of the last row of d_snr would be read 4 GiB low


def window_planes():
    """(snr float32 [1][4][4][128], peaks uint32 [1][4][4][128][2]): the call's windows, with one sure candidate in the row
    of d_snr past the line (DM 3, width 3), one in the row before it (DM 3, width 2: its other side), and one in the row 4
    GiB below (DM 0, width 0)."""
    snr, peaks = seeded_planes(B, NR_DM, NR_WIDTHS, NR_BLOCKS, seed=71)
    snr[0, 3, 3, 40], snr[0, 3, 2, 100], snr[0, 0, 0, 70] = 30.0, 31.0, 32.0
    return snr, peaks


def row_entry(m, i):
    """The entry (a float of d_snr, a pair of d_peaks) at which the window of row (m, i) begins."""
    return (m * NR_WIDTHS + i) * PEAK_BLOCKS + FIRST_BLOCK


def wrapped_entry(entry, entry_bytes):
    """Where a kernel whose byte offsets are 32-bit would go for ``entry``."""
    return (entry * entry_bytes) % lt.LINE // entry_bytes


def planted_entries():
    """Every entry of the windows, as a set of (first, last + 1) ranges -- the same for d_snr and d_peaks."""
    return [(row_entry(m, i), row_entry(m, i) + NR_BLOCKS) for m in range(NR_DM) for i in range(NR_WIDTHS)]


def decoy_entry():
    """The float of d_snr at which the decoys begin: the last row's window, 4 GiB low."""
    return wrapped_entry(row_entry(NR_DM - 1, NR_WIDTHS - 1), 4)


def as_read(wrap_snr=False, wrap_peaks=False):
    """The windows as the kernels read them; with ``wrap_*`` as kernels would whose byte offsets into that plane came out
    mod 2^32: the decoys for the last row of d_snr, the fill for the peaks of the last nine rows."""
    snr, peaks = window_planes()
    for m in range(NR_DM):
        for i in range(NR_WIDTHS):
            e = row_entry(m, i)
            if wrap_snr and e * 4 >= lt.LINE:
                snr[0, m, i] = SNR_DECOY
            if wrap_peaks and e * 8 >= lt.LINE:
                peaks[0, m, i] = FILL_WORD
    return snr, peaks


def expected(wrap_snr=False, wrap_peaks=False):
    """(records, count) of the call, the records' block counted from the plane's first."""
    snr, peaks = as_read(wrap_snr, wrap_peaks)
    rec, count = find_candidates(snr, peaks, 0, NR_BLOCKS, THRESHOLD, *RADII, MAX_CANDIDATES)
    rec["block"] += np.uint32(FIRST_BLOCK)
    return rec, count
