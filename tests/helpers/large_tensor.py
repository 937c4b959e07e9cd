"""Sparse checks of device tensors past 4 GiB, which never exist on the host (tests/test_gpu_large_tensors.py; the plan
itself is tested without a device by tests/test_large_tensor_plan.py).

A tensor is filled with a seeded pattern of a whole number of rows, uploaded once and doubled over the device tensor with
device-to-device copies: the byte at offset o is pattern[o mod P], so the host can produce any row without holding the
tensor.  The period P is an ODD number of rows greater than 1 and therefore does not divide 2^32: a row and the bytes
4 GiB below it differ, and a kernel whose offset wrapped at 2^32 reads or writes something the model does not expect.
In every kernel concerned input row r gives output row r (or a fixed permutation of it), so a sample of rows is modelled
by itself with the numpy models of the small tests."""
import numpy as np

LINE = 1 << 32            # a 32-bit byte offset wraps here
PATTERN_BYTES = 4 << 20   # about the size of a pattern
RANDOM_ROWS = 64
HOST_LIMIT = 256 << 20    # no host array of a test may pass this


def period_rows(row_bytes):
    """An odd number of rows greater than 1, about PATTERN_BYTES of them."""
    p = max(3, PATTERN_BYTES // row_bytes) | 1
    assert p % 2 == 1 and p > 1 and LINE % (p * row_bytes) != 0
    return p


def int8_pattern(row_bytes, seed):
    """Full-range int8 [period_rows][row_bytes] with -128 at the first and 127 at the last byte."""
    p = period_rows(row_bytes)
    pat = np.random.default_rng(seed).integers(-128, 128, size=(p, row_bytes), dtype=np.int8)
    pat[0, 0], pat[-1, -1] = -128, 127
    return pat


def lines_of(row_bytes, rows):
    """The multiples of 2^32 strictly inside a tensor of ``rows`` rows."""
    return list(range(LINE, rows * row_bytes, LINE))


def alias_rows(row_bytes, rows, r):
    """The rows that hold the bytes 2^32, 2 * 2^32, ... below the bytes of row r (none where row r lies below the first
    line altogether)."""
    out = []
    lo, hi = r * row_bytes, (r + 1) * row_bytes - 1
    k = 1
    while hi - k * LINE >= 0:
        first, last = max(lo - k * LINE, 0) // row_bytes, (hi - k * LINE) // row_bytes
        out.extend(range(first, last + 1))
        k += 1
    return out


def plan(row_bytes_in, row_bytes_out, rows, seed, extra=()):
    """The sorted row sample: the first and last two rows; for every multiple of 2^32 inside either tensor the row that
    holds (or begins at) the line and its two neighbours; 64 seeded rows; ``extra``; and for every one of these at or above
    a line of either tensor its alias rows in that tensor."""
    assert rows >= 4
    base = {0, 1, rows - 2, rows - 1} | {int(r) for r in extra}
    for rb in (row_bytes_in, row_bytes_out):
        for line in lines_of(rb, rows):
            r = line // rb  # straddles the line unless it begins there
            base |= {r - 1, r, min(r + 1, rows - 1)}
    base |= {int(r) for r in np.random.default_rng(seed).integers(0, rows, size=RANDOM_ROWS)}
    assert all(0 <= r < rows for r in base)
    sample = set(base)
    for rb in (row_bytes_in, row_bytes_out):
        for r in base:
            sample |= set(alias_rows(rb, rows, r))
    return np.array(sorted(sample), dtype=np.int64)


def fill(gpu, d_ptr, nbytes, pattern):
    """Replicates ``pattern`` over the device bytes [d_ptr, d_ptr + nbytes): one upload, then doubling copies."""
    pat = np.ascontiguousarray(pattern).reshape(-1).view(np.uint8)
    P = pat.nbytes
    assert P <= HOST_LIMIT
    base = int(d_ptr)
    gpu.memcpy_htod(base, pat[:min(P, nbytes)])
    done = P
    while done < nbytes:  # done stays a multiple of P: the copy continues the period
        n = min(done, nbytes - done)
        gpu.memcpy_dtod(base + done, base, n)
        done += n
    gpu.synchronize()


def rows_of(pattern, rows):
    """uint8 [len(rows)][row_bytes]: the bytes of the given rows of a tensor filled with ``pattern`` ([period][...])."""
    pat = np.ascontiguousarray(pattern)
    pat = pat.reshape(pat.shape[0], -1).view(np.uint8)
    return pat[np.asarray(rows, dtype=np.int64) % pat.shape[0]]


def elements_of(pattern, index):
    """The elements at flat ``index`` (any shape) of a tensor of pattern's dtype filled with ``pattern``."""
    flat = np.ascontiguousarray(pattern).reshape(-1)
    return flat[np.asarray(index, dtype=np.int64) % flat.size]


def read_rows(gpu, d_ptr, row_bytes, rows):
    """uint8 [len(rows)][row_bytes] from the device; ``rows`` ascending and distinct; a run of adjacent rows is one copy."""
    rows = np.asarray(rows, dtype=np.int64)
    assert rows.ndim == 1 and (rows.size < 2 or np.all(np.diff(rows) > 0))
    out = np.empty((rows.size, row_bytes), dtype=np.uint8)
    assert out.nbytes <= HOST_LIMIT
    starts = np.flatnonzero(np.concatenate([[True], np.diff(rows) != 1])) if rows.size else []
    ends = list(starts[1:]) + [rows.size]
    for i, j in zip(starts, ends):
        gpu.memcpy_dtoh(out[i:j], int(d_ptr) + int(rows[i]) * row_bytes)
    return out


# ---- the cases of tests/test_gpu_large_tensors.py: the smallest shapes at which the named tensor passes 2^32 bytes with the
# kernel's ordinary geometry (nt = 16400 is 1025 sample blocks).  A row is one (channel, block): [A][16][2] int8 of samples
# in, [B] beams' worth of the output out.

FLOAT, Q8, POWER = 128, 32, 4  # bytes of one beam of one block: 16 complex floats; 16 complex int8; one float
# name: (A, B, C, nt, output bytes per beam and block, the tensors that pass a line)
BEAMFORMER_CASES = {
    "staged_whole": (64, 16, 2048, 16400, FLOAT, ("in", "out")),
    "chain_whole": (128, 32, 1024, 16400, FLOAT, ("in", "out")),
    "chain_ragged": (130, 33, 1024, 16400, FLOAT, ("in", "out")),
    "staged_ragged": (48, 24, 4096, 10928, FLOAT, ("in", "out")),
    "q8": (64, 256, 512, 16400, Q8, ("out",)),
    "power": (64, 1024, 1024, 16400, POWER, ("out",)),
    # kChain has stores of its own for the 8-bit beams and the block power: the same two outputs with 128 antennas
    "q8_chain": (128, 256, 512, 16400, Q8, ("out",)),
    "power_chain": (128, 1024, 1024, 16400, POWER, ("in", "out")),
    "fused_output": (4, 512, 2048, 528, FLOAT, ("out",)),
    "fused_samples": (256, 1, 8192, 1040, FLOAT, ("in",)),
}
STOKES_SHAPE = (64, 4096, 16400)                               # B, C, nt
INCOHERENT_SHAPES = [(256, 2048, 4112), (130, 2048, 8080)]     # A, C, nt
FILTERBANK_SHAPE = (4096, 64, 4100)                            # C, NB, T
RING_SHAPE = (4096, 64, 16400, 8, 16392)                       # C, NB, out_spectra, T, first_spectrum


def beamformer_rows(name):
    """(row_bytes_in, row_bytes_out, rows) of a beamformer case."""
    A, B, C, nt, per_beam, _ = BEAMFORMER_CASES[name]
    return A * 32, B * per_beam, C * (nt // 16)


def row_cases():
    """Every case as (name, row_bytes_in, row_bytes_out, rows, the tensors that pass a line): what the plan test walks."""
    out = [(name,) + beamformer_rows(name) + (BEAMFORMER_CASES[name][5],) for name in BEAMFORMER_CASES]
    B, C, nt = STOKES_SHAPE
    out.append(("stokes_iquv", B * 32, B * 16, C * (nt // 16), ("in", "out")))
    out.append(("stokes_i", B * 32, B * 4, C * (nt // 16), ("in",)))
    out.append(("integrate_stokes", B * 16, B * 16, C * (nt // 16), ("in", "out")))
    out.append(("integrate_block_power", 1024 * 4, 1024 * 4, 1024 * 1025, ("in", "out")))
    for A, C, nt in INCOHERENT_SHAPES:
        out.append((f"incoherent_{A}", A * 32, 4, C * (nt // 16), ("in",)))
    C, NB, T = FILTERBANK_SHAPE
    out.append(("filterbank", NB * 4, NB, T * C, ("in",)))           # rows (spectrum, channel): NB floats in, NB bytes out
    C, NB, out_spectra, T, first = RING_SHAPE
    out.append(("filterbank_ring", 1, C, NB * out_spectra, ("out",)))  # rows (beam, spectrum) of the bytes; no input row
    return out


def stokes_int32_pattern(row_elems, seed):
    """Block Stokes values as the block call makes them (|v| <= 2^20) with larger ones planted at the first and the last
    element of every row, whose sums pass 2^24 and are no floats: int32 [period_rows][row_elems]."""
    p = period_rows(row_elems * 4)
    pat = np.random.default_rng(seed).integers(-(1 << 20), (1 << 20) + 1, size=(p, row_elems), dtype=np.int64).astype(np.int32)
    k = np.arange(p) % 1024
    pat[:, 0] = (1 << 23) + 1 + k * k
    pat[:, -1] = -(1 << 23) - 1 - k * k
    return pat


def spectra_pattern(row_elems, seed):
    """Float spectra x = 1000 (1 + 0.25 g), g normal: float32 [period_rows][row_elems]."""
    p = period_rows(row_elems * 4)
    g = np.random.default_rng(seed).standard_normal((p, row_elems))
    return (1000.0 * (1.0 + 0.25 * g)).astype(np.float32)


def row_as_wrapped(pattern, row_bytes, r, k=1):
    """The bytes of row r as a kernel would read them whose byte offsets at or above k * 2^32 came out k * 2^32 lower (a
    row that straddles the line keeps its part below it); None where the row lies below the line altogether."""
    off = r * row_bytes + np.arange(row_bytes, dtype=np.int64)
    off = np.where(off >= k * LINE, off - k * LINE, off)
    if off[-1] == (r + 1) * row_bytes - 1:
        return None
    return elements_of(np.ascontiguousarray(pattern).reshape(-1).view(np.uint8), off)
