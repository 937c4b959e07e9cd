"""Which form the pulsar folder's kernels take for a shape (dc_sand_amd/csrc/bf_fold.hip; DESIGN.md section 5.24, "The forms"),
restated on the CPU.  The launcher picks the tile width W = 256 >> form from nbin and C alone, so a shape names its form.
tests/test_fold_forms.py holds these constants and rules to the kernel's source text and takes the census of the GPU tests'
table (helpers/fold_cases.py) with them."""
from dataclasses import dataclass

THREADS = 1024        # of a workgroup of bf_fold_kernel
TILE_WORDS = 16384    # 64 KiB of LDS: nbin * W words at the most
MAX_WIDTH = 256
MIN_WIDTH = 16
ROWS = 8              # spectra whose loads a lane has in flight: the unroll
HITS_THREADS = 256
SCRUNCH_THREADS = 256
MAX_BINS = 1024

ALL_FORMS = (0, 1, 2, 3, 4)                       # W = 256, 128, 64, 32, 16
NBIN_BOUNDARIES = (64, 128, 256, 512)             # the largest nbin of the forms 0 .. 3 at a wide band


def form_of(nbin, C):
    """The launcher's fold_form: as wide as nbin leaves room for, no wider than the band needs, down to MIN_WIDTH."""
    form = 0
    while (MAX_WIDTH >> form) * nbin > TILE_WORDS:
        form += 1
    while (MAX_WIDTH >> form) > MIN_WIDTH and (MAX_WIDTH >> (form + 1)) >= C:
        form += 1
    return form


def nbin_form(nbin):
    """The form of a band wide enough for any tile."""
    return form_of(nbin, MAX_WIDTH)


@dataclass(frozen=True)
class Form:
    form: int
    W: int             # channels of a tile
    T: int             # time slices of a workgroup
    uniform: bool      # a wave is one slice: the phase is scalar work (the kernel template's kUniform)
    tiles: int
    ragged: bool       # the last tile has fewer than W channels
    full: bool         # some tile has all W
    chunk: int         # spectra of a slice
    slices_on: int     # slices that have a spectrum at all
    tail: bool         # some slice's spectra are no multiple of the unroll


def fold_form(nbin, C, L):
    f = form_of(nbin, C)
    W = MAX_WIDTH >> f
    T = THREADS // W
    chunk = (L + T - 1) // T
    lens = [min(chunk, max(0, L - ts * chunk)) for ts in range(T)]
    return Form(f, W, T, W >= 64, (C - 1) // W + 1, C % W != 0, C >= W, chunk, sum(1 for n in lens if n), any(n % ROWS for n in lens))


def scrunch_form(nbin):
    """(lanes along the bins, groups of lanes along the channels, tiles of bins)."""
    jw = 1
    while jw < nbin and jw < SCRUNCH_THREADS:
        jw <<= 1
    return jw, SCRUNCH_THREADS // jw, (nbin - 1) // jw + 1


def census(cases):
    """What (C, nbin, subint_len) calls present to the fold kernel."""
    forms = [fold_form(nbin, C, L) for C, nbin, L in cases]
    return {"forms": {f.form for f in forms},
            "forms by nbin on a wide band": {f.form for f, (C, _, _) in zip(forms, cases) if C >= MAX_WIDTH},
            "full": {f.form for f in forms if f.full}, "ragged": {f.form for f in forms if f.ragged},
            "several tiles": {f.form for f in forms if f.tiles > 1},
            "tail": {f.form for f in forms if f.tail}, "no tail": {f.form for f in forms if not f.tail},
            "idle slices": {f.form for f in forms if f.slices_on < f.T}, "every slice": {f.form for f in forms if f.slices_on == f.T},
            "several trips": {f.form for f in forms if f.chunk > ROWS},
            "nbin": {nbin for _, nbin, _ in cases}}
