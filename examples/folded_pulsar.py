#!/usr/bin/env python3
"""Folding two pulsars (include/dcs_fold.h) on an MI355X, each in the Stokes filterbanks of its own pointing:

    filterbank bytes [4 * pointings] -> dm_delays (one DM per pointing) -> fold_q8 (beams_per_model = 4) -> fold_scrunch

The filterbanks are noise as filterbank_q8 leaves it (mean 128, standard deviation 16 in every channel).  Each pointing has four
of them, as the Stokes parameters I, Q, U, V; its I carries a dispersed pulsar: in every spectrum whose phase under the
pointing's model (dc_sand_amd.fold.fold_models of a spin frequency, its derivative and a phase) falls into the pulsar's bin,
every channel is raised by two counts -- an eighth of a standard deviation -- at the row its dispersion delay puts it.  The fold
reads every channel at that delay, so the pulse lands in one bin; the scrunch sums the channels.

    python examples/folded_pulsar.py

The script asserts that in every sub-integration the I profile of either pointing peaks in the predicted bin, and that every
other bin of all eight profiles is flat: within five standard deviations of hits * C * 128, the noise the bytes were made with.
It prints one summary line."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.fold import bin_of, fold_models, model_dtype  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, dm_delays_bytes, filterbank_bytes, fold_hits_bytes,  # noqa: E402
                                   fold_profiles_bytes, fold_scrunched_bytes)

C, POINTINGS, STOKES = 128, 2, 4
B = POINTINGS * STOKES
BAND = (1500.0, -300.0 / C, 256e-6)                # MHz of column 0, MHz per column, seconds per spectrum
SUBINT_LEN, NR_SUBINTS, NBIN = 8192, 4, 64
T = SUBINT_LEN * NR_SUBINTS
DMS = np.array([30.0, 55.0])                       # one per pointing
SPIN = [(7.2993, -1.0e-6, 0.10), (11.8671, 2.5e-6, 0.65)]  # f0 in Hz, f1 in Hz/s, phase in turns at spectrum 0
PEAK_BIN = [20, 47]
LEVEL, SIGMA, HEIGHT = 128.0, 16.0, 2.0


def bins_of(model, n):
    """The bins of spectra 0 .. n - 1 of one model, in the uint64 arithmetic of the device: it wraps."""
    k = np.arange(n, dtype=np.uint64)
    phi = np.uint64(model["phase0"]) + k * np.uint64(model["step"]) + (k * (k - np.uint64(1)) // np.uint64(2)) * np.uint64(model["accel"])
    return bin_of(phi, NBIN)


def make_filterbanks(rows, table, models):
    rng = np.random.default_rng(20261021)
    x = rng.normal(LEVEL, SIGMA, size=(B, rows, C)).astype(np.float32)
    cols = np.arange(C)
    for p in range(POINTINGS):
        for s in range(NR_SUBINTS):
            on = s * SUBINT_LEN + np.flatnonzero(bins_of(models[p, s], SUBINT_LEN) == PEAK_BIN[p])
            x[STOKES * p, on[:, None] + table[p][None, :], cols[None, :]] += HEIGHT  # Stokes I of the pointing, at the dispersed rows
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def main():
    require_device()
    set_device(0)
    p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=1, NR_BEAMS=1)
    gen = SteeringCoefficientGenerator(p)
    ndelays = dm_delays_bytes(p, POINTINGS)
    d_dms, d_delays = mem_alloc(DMS.nbytes), mem_alloc(ndelays)
    memcpy_htod(d_dms, DMS)
    gen.dm_delays(*BAND, d_dms, POINTINGS, d_delays, ndelays)  # row p: the delays of pointing p's DM, what the fold needs
    synchronize()
    table = np.empty((POINTINGS, C), np.int32)
    memcpy_dtoh(table, d_delays)
    max_delay = int(table.max())
    rows = T + max_delay

    models = np.stack([fold_models(f0, f1, phi0, BAND[2], SUBINT_LEN, NR_SUBINTS) for f0, f1, phi0 in SPIN])
    assert models.dtype == model_dtype and models.shape == (POINTINGS, NR_SUBINTS)
    fb = make_filterbanks(rows, table, models)

    nfb, nprof = filterbank_bytes(p, B, rows), fold_profiles_bytes(p, B, NR_SUBINTS, NBIN)
    nhits, nscr = fold_hits_bytes(POINTINGS, NR_SUBINTS, NBIN), fold_scrunched_bytes(B, NR_SUBINTS, NBIN)
    d_fb, d_models, d_prof, d_hits, d_scr = mem_alloc(nfb), mem_alloc(models.nbytes), mem_alloc(nprof), mem_alloc(nhits), mem_alloc(nscr)
    memcpy_htod(d_fb, fb)
    memcpy_htod(d_models, np.ascontiguousarray(models))
    gen.fold_q8(d_fb, nfb, rows, 0, SUBINT_LEN, NR_SUBINTS, B, d_models, models.nbytes, NBIN, d_prof, nprof, NR_SUBINTS,
                beams_per_model=STOKES, d_delays=d_delays, delays_bytes=ndelays, max_delay=max_delay, d_hits=d_hits, hits_bytes=nhits)
    gen.fold_scrunch(d_prof, nprof, B, NR_SUBINTS, 0, NR_SUBINTS, NBIN, d_scr, nscr)
    synchronize()
    hits, plane = np.empty((POINTINGS, NR_SUBINTS, NBIN), np.uint32), np.empty((B, NR_SUBINTS, NBIN), np.uint64)
    memcpy_dtoh(hits, d_hits)
    memcpy_dtoh(plane, d_scr)
    gen.close()

    # the noise model: a bin of h hits sums h * C bytes of mean LEVEL and variance SIGMA^2 + 1/12 (the rounding)
    n = np.repeat(hits.astype(np.float64), STOKES, axis=0) * C
    excess = (plane.astype(np.float64) - LEVEL * n) / np.sqrt(n * (SIGMA * SIGMA + 1.0 / 12.0))
    assert np.all(hits.sum(axis=-1) == SUBINT_LEN)
    off = np.ones(excess.shape, bool)
    peaks = []
    for q in range(POINTINGS):
        off[STOKES * q, :, PEAK_BIN[q]] = False
        peaks.append(np.argmax(excess[STOKES * q], axis=-1).tolist())
    peak_found = all(pk == [PEAK_BIN[q]] * NR_SUBINTS for q, pk in enumerate(peaks))
    flat = bool(np.all(np.abs(excess[off]) < 5.0))
    on_sigma = [float(excess[STOKES * q, :, PEAK_BIN[q]].min()) for q in range(POINTINGS)]
    print(f"folded {B} x {rows} x {C} bytes ({POINTINGS} pointings of {STOKES} Stokes filterbanks, DMs {DMS.tolist()}, delays up to "
          f"{max_delay} spectra) into {NR_SUBINTS} sub-integrations of {NBIN} bins: the peak bin of every sub-integration is the predicted "
          f"one: {peak_found} (found {peaks}, predicted {PEAK_BIN}, at {on_sigma[0]:.1f} and {on_sigma[1]:.1f} sigma or more); every "
          f"off-pulse bin is flat to the noise model: {flat} (largest {float(np.abs(excess[off]).max()):.2f} sigma of {int(off.sum())} bins)")
    assert peak_found, peaks
    assert flat
    return 0


if __name__ == "__main__":
    sys.exit(main())
