"""The shapes of tests/test_gpu_single_pulse_large.py, and what the host can say about tensors that exist on the device
only (helpers/large_tensor.py).  tests/test_single_pulse_large_plan.py walks the same plans without a device and shows
that a byte offset worked out in 32 bits cannot pass them."""
import numpy as np

from helpers import large_tensor as lt
from helpers.single_pulse_model import nr_blocks_of

# -- a plane past 2^32 bytes: 4 series of 2^28 + 4096 words; the line falls into series 3
PLANE = dict(B=1, nr_dm=4, plane_spectra=(1 << 28) + 4096, T=5000, widths=(1, 300, 17, 64), max_width=300, block_len=256)
PLANE_BYTES = PLANE["B"] * PLANE["nr_dm"] * PLANE["plane_spectra"] * 4
PLANE_WINDOW = PLANE["T"] + PLANE["max_width"] - 1
LINE_WORD = lt.LINE // 4 - 3 * PLANE["plane_spectra"]  # the word of series 3 that begins at the line


def plane_pattern():
    """uint32 [1025][1024]: full-range words; 1025 rows of 4096 bytes do not divide 2^32."""
    return lt.int8_pattern(4096, seed=31).view(np.uint32)


def plane_firsts():
    """first_spectrum of the windows: series 3's ends below the line, straddles it twice, begins on it and above it, and
    ends with the series."""
    w, ps = PLANE_WINDOW, PLANE["plane_spectra"]
    return [LINE_WORD - w, LINE_WORD - w // 2, LINE_WORD - 1, LINE_WORD, LINE_WORD + 100, ps - w]


def plane_window(pattern, first, wrapped=False):
    """uint32 [1][4][window]: the words first .. of every series of the device plane; ``wrapped``: as a kernel would read them
    whose byte offsets at or above 2^32 came out 2^32 lower."""
    rows = []
    for s in range(PLANE["nr_dm"]):
        word = s * PLANE["plane_spectra"] + first + np.arange(PLANE_WINDOW, dtype=np.int64)
        if wrapped:
            word = np.where(word * 4 >= lt.LINE, word - lt.LINE // 4, word)
        rows.append(lt.elements_of(pattern, word))
    return np.stack(rows)[None]


# -- outputs past 2^32 bytes, written at the end of every (DM, width) row only.  A row of the checks is the nr_blocks entries
# that a call writes: ROW_BLOCKS * 8 bytes of peaks, ROW_BLOCKS * 4 bytes of signal-to-noise
ROW_BLOCKS = 16
WIDTHS_OUT = (1, 5, 64, 0)
PEAKS_OUT = dict(B=1, nr_dm=4, peak_blocks=(1 << 25) + 512, T=ROW_BLOCKS * 64, block_len=64, max_width=64)   # peaks past 2^32
SNR_OUT = dict(B=1, nr_dm=4, peak_blocks=(1 << 26) + 256, count=ROW_BLOCKS * 64, max_width=64)               # snr past 2^32, peaks 2^33
assert nr_blocks_of(PEAKS_OUT["T"], PEAKS_OUT["block_len"]) == ROW_BLOCKS


def out_rows(peak_blocks, entry_bytes):
    """(row_bytes, rows per (DM, width) row, the rows a call writes, the rows 2^32 and 2^33 bytes below them that exist)."""
    row_bytes = ROW_BLOCKS * entry_bytes
    assert (peak_blocks * entry_bytes) % row_bytes == 0
    per = peak_blocks * entry_bytes // row_bytes
    written = np.array([(s + 1) * per - 1 for s in range(4 * len(WIDTHS_OUT))], dtype=np.int64)
    assert lt.LINE % row_bytes == 0
    alias = sorted({int(w) - k * (lt.LINE // row_bytes) for w in written for k in (1, 2) if w - k * (lt.LINE // row_bytes) >= 0})
    return row_bytes, per, written, np.array(alias, dtype=np.int64)
