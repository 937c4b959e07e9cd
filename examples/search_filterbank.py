#!/usr/bin/env python3
"""8-bit search filterbanks (include/dcs_filterbank.h) on an MI355X, from samples to the bytes a search reads:

    samples -> beamform_accumulated_power -> integrate_block_power -> spectra_sums -> filterbank_scales -> filterbank_q8

for the detected beams, one [time][channel] byte series per beam in descending frequency order, and the incoherent spectra
of the same samples through the same three calls with ``nr_beams = 1``.

    python examples/search_filterbank.py [ant beams chan]

The check at the end restates the three contracts in numpy (tests/helpers/filterbank_model.py) on the float spectra the
device made: sums, scales, bytes and clip counts must agree bit for bit."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dc_sand_amd import BeamformerParameters  # noqa: E402
from dc_sand_amd.device import mem_alloc, memcpy_dtoh, memcpy_htod, memset, require_device, set_device, synchronize  # noqa: E402
from dc_sand_amd.generator import (SteeringCoefficientGenerator, block_power_bytes, filterbank_bytes,  # noqa: E402
                                   filterbank_scales_bytes, incoherent_block_power_bytes, incoherent_spectra_bytes,
                                   power_spectra_bytes, simulate_input, spectra_sums_bytes)
from helpers.filterbank_model import filterbank, same_bits, scales, spectra_sums  # noqa: E402

A, B, C = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 16, 64)
NT, N = 1024, 2                                               # samples per call; blocks of 16 samples per spectrum
TARGET_STD, LEVEL = 24.0, 128.0
require_device()
set_device(0)
p = BeamformerParameters(NR_CHANNELS=C, NR_STATIONS=A, NR_BEAMS=B, NR_SAMPLES_PER_CHANNEL=NT)
gen = SteeringCoefficientGenerator(p)
gen.upload_delays(simulate_input(p))

nblk = NT // 16
T = nblk // N                                                 # spectra per call
samples = np.random.default_rng(1).integers(-128, 128, size=(C, nblk, A, 16, 2), dtype=np.int8)
samples[C // 2] //= 4                                         # a bandpass for the scales to take out
d_ant = mem_alloc(samples.nbytes)
memcpy_htod(d_ant, samples)

# detected beams: float [T][C][B]; the incoherent beam: float [T][C]
pbytes, sbytes = block_power_bytes(p, NT), power_spectra_bytes(p, nblk, N)
ipbytes, isbytes = incoherent_block_power_bytes(p, NT), incoherent_spectra_bytes(p, nblk, N)
d_power, d_spectra, d_ipower, d_ispectra = mem_alloc(pbytes), mem_alloc(sbytes), mem_alloc(ipbytes), mem_alloc(isbytes)
gen.beamform_accumulated_power(d_ant, samples.nbytes, d_power, pbytes, NT, t_coeff=0)
gen.integrate_block_power(d_power, pbytes, nblk, N, d_spectra, sbytes)
gen.incoherent_block_power(d_ant, samples.nbytes, d_ipower, ipbytes, NT)
gen.integrate_incoherent_power(d_ipower, ipbytes, nblk, N, d_ispectra, isbytes)


def to_filterbank(d_x, xbytes, beams):
    """The three calls on spectra float [T][C][beams]; what the device made and what the model makes of the same spectra."""
    nsums, nscales, nfb = spectra_sums_bytes(p, beams), filterbank_scales_bytes(p, beams), filterbank_bytes(p, beams, T)
    d_sums, d_scales, d_fb, d_clips = mem_alloc(nsums), mem_alloc(nscales), mem_alloc(nfb), mem_alloc(beams * 8)
    memset(d_clips, 0, beams * 8)
    gen.spectra_sums(d_x, xbytes, T, beams, d_sums, nsums)
    gen.filterbank_scales(d_sums, nsums, T, beams, TARGET_STD, d_scales, nscales)
    gen.filterbank_q8(d_x, xbytes, T, beams, d_scales, LEVEL, d_fb, nfb, T, descending=True, d_clip_count=d_clips)
    synchronize()
    x, sums, sc = np.empty((T, C, beams), np.float32), np.empty((C, beams, 2), np.float64), np.empty((C, beams, 2), np.float32)
    fb, clips = np.empty((beams, T, C), np.uint8), np.empty(beams, np.uint64)
    for host, dev in ((x, d_x), (sums, d_sums), (sc, d_scales), (fb, d_fb), (clips, d_clips)):
        memcpy_dtoh(host, dev)
    m_sums = spectra_sums(x)
    m_sc = scales(m_sums, T, TARGET_STD)
    m_fb, m_clips = filterbank(x, m_sc, LEVEL, descending=True)
    same = (same_bits(sums, m_sums) is None and same_bits(sc, m_sc) is None and same_bits(fb, m_fb) is None
            and np.array_equal(clips, m_clips))
    return fb, clips, same


fb, clips, same_detected = to_filterbank(d_spectra, sbytes, B)
print(f"{A} ant x {B} beams x {C} chan: {T} spectra of {16 * N} samples per beam as uint8 [{B}][{T}][{C}], mean {fb.mean():.2f}, "
      f"standard deviation {fb.std():.2f}, {int(clips.sum())} clipped; {fb.nbytes} bytes instead of {sbytes} bytes of floats")
ifb, iclips, same_incoherent = to_filterbank(d_ispectra, isbytes, 1)
print(f"incoherent beam as uint8 [1][{T}][{C}], mean {ifb.mean():.2f}, standard deviation {ifb.std():.2f}, {int(iclips.sum())} clipped")
print("bit-identical to the model: detected beams", same_detected, "- incoherent beam", same_incoherent)
sys.exit(0 if same_detected and same_incoherent else 1)
