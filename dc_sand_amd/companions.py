"""The companion libraries of ``libdcs_beamformer.so``, one row each: the build (``build.py``) compiles ``source`` into
``lib`` and watches ``header``; the binding (``_lib.companion``) loads ``lib`` from beside the product library and gives
every function of ``signatures`` its ``(name, restype, argtypes)``.  Needs no built library to import.
"""
from __future__ import annotations

from ctypes import POINTER, c_float, c_int, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p
from typing import NamedTuple

_VP = c_void_p


class Companion(NamedTuple):
    header: str  # under include/
    source: str  # under dc_sand_amd/csrc/
    lib: str  # beside the product library
    signatures: list


COMPANIONS = {
    # staged delay tables for the streams of the product library
    "stream_staging": Companion("dcs_stream_staging.h", "bf_stream_staging.cpp", "libdcs_stream_staging.so", [
        ("dcs_bf_stream_stage_table", c_int, [_VP, _VP, c_int]),
        ("dcs_bf_stream_stage_table_from_global", c_int, [_VP, _VP, c_uint32, c_uint32, _VP]),
    ]),
    # per-input beam weights for the product library's beamformers
    "beam_weights": Companion("dcs_beam_weights.h", "bf_beam_weights.cpp", "libdcs_beam_weights.so", [
        ("dcs_bf_generate_and_beamform_weighted", c_int, [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
        ("dcs_bf_generate_and_beamform_weighted_dt", c_int,
         [_VP, POINTER(c_float), c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
        ("dcs_bf_beamform_accumulated_weighted", c_int, [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
        ("dcs_bf_beamform_accumulated_weighted_dt", c_int, [_VP, c_float, c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
    ]),
    # quantised int8 beam output of the product library's matrix-core beamformer
    "beam_quant": Companion("dcs_beam_quant.h", "bf_beam_quant.cpp", "libdcs_beam_quant.so", [
        ("dcs_bf_beamform_accumulated_q8", c_int, [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, _VP, _VP, c_size_t, _VP, _VP]),
        ("dcs_bf_beamform_accumulated_q8_dt", c_int, [_VP, c_float, c_uint32, _VP, c_size_t, _VP, _VP, _VP, c_size_t, _VP, _VP]),
    ]),
    # detected, time-integrated beam power of the same beamformer
    "beam_power": Companion("dcs_beam_power.h", "bf_beam_power.cpp", "libdcs_beam_power.so", [
        ("dcs_bf_beamform_accumulated_power", c_int, [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
        ("dcs_bf_beamform_accumulated_power_dt", c_int, [_VP, c_float, c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
        ("dcs_bf_integrate_block_power", c_int, [_VP, _VP, c_size_t, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP]),
    ]),
    # the incoherent beam: the antennas' own power, summed exactly and integrated like the detected beams
    "incoherent_beam": Companion("dcs_incoherent_beam.h", "bf_incoherent_beam.cpp", "libdcs_incoherent_beam.so", [
        ("dcs_bf_incoherent_block_power", c_int, [_VP, c_uint32, _VP, c_size_t, _VP, _VP, c_size_t, _VP]),
        ("dcs_bf_integrate_incoherent_power", c_int, [_VP, _VP, c_size_t, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP]),
    ]),
    # 8-bit search filterbanks from float spectra: running sums, scales, and the quantiser that transposes to beam-major bytes
    "filterbank": Companion("dcs_filterbank.h", "bf_filterbank.cpp", "libdcs_filterbank.so", [
        ("dcs_bf_spectra_sums", c_int, [_VP, _VP, c_size_t, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_filterbank_scales", c_int, [_VP, _VP, c_size_t, c_uint64, c_uint32, c_float, _VP, c_size_t, _VP]),
        ("dcs_bf_filterbank_q8", c_int,
         [_VP, _VP, c_size_t, c_uint32, c_uint32, _VP, c_float, c_uint32, _VP, c_size_t, c_uint64, c_uint64, _VP, _VP]),
    ]),
    # the true complex product (tied-array beams) of the matrix-core beamformer: float beams and detected block power
    "beam_complex": Companion("dcs_beam_complex.h", "bf_beam_complex.cpp", "libdcs_beam_complex.so", [
        ("dcs_bf_beamform_accumulated_complex", c_int, [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_beamform_accumulated_complex_dt", c_int, [_VP, c_float, c_uint32, _VP, c_size_t, _VP, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_beamform_accumulated_complex_power", c_int,
         [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_beamform_accumulated_complex_power_dt", c_int,
         [_VP, c_float, c_uint32, _VP, c_size_t, _VP, c_uint32, _VP, c_size_t, _VP]),
    ]),
    # the same product with the int8 output of beam_quant: 8-bit complex voltage beams out of the kernel's epilogue
    "beam_complex_quant": Companion("dcs_beam_complex_quant.h", "bf_beam_complex_quant.cpp", "libdcs_beam_complex_quant.so", [
        ("dcs_bf_beamform_accumulated_complex_q8", c_int,
         [_VP, c_uint64, c_uint32, _VP, c_size_t, _VP, c_uint32, _VP, _VP, c_size_t, _VP, _VP]),
        ("dcs_bf_beamform_accumulated_complex_q8_dt", c_int,
         [_VP, c_float, c_uint32, _VP, c_size_t, _VP, c_uint32, _VP, _VP, c_size_t, _VP, _VP]),
    ]),
    # full-Stokes detection of two polarisations' int8 beams: exact block I or I, Q, U, V, integrated like the incoherent beam
    "stokes": Companion("dcs_stokes.h", "bf_stokes.cpp", "libdcs_stokes.so", [
        ("dcs_bf_stokes_block", c_int, [_VP, c_uint32, _VP, _VP, c_size_t, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_integrate_stokes", c_int, [_VP, _VP, c_size_t, c_uint32, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP]),
    ]),
    # incoherent dedispersion of the 8-bit filterbanks: the delay table of a band and DMs, and exact uint32 DM-time planes
    "dedisperse": Companion("dcs_dedisperse.h", "bf_dedisperse.cpp", "libdcs_dedisperse.so", [
        ("dcs_bf_dm_delays", c_int, [_VP, _VP, _VP, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_dedisperse_q8", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, _VP, c_uint32, c_uint32, _VP, _VP, c_size_t, c_uint64,
          c_uint64, _VP]),
    ]),
    # the single-pulse search on those planes: exact sums per series, boxcar peaks per width and block, and their signal-to-noise
    "single_pulse": Companion("dcs_single_pulse.h", "bf_single_pulse.cpp", "libdcs_single_pulse.so", [
        ("dcs_bf_dm_time_sums", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_boxcar_peaks", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, _VP, c_uint32, c_uint32, c_uint32, _VP, c_size_t,
          c_uint64, c_uint64, _VP]),
        ("dcs_bf_peak_snr", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, _VP, c_uint32, c_uint32, _VP, c_size_t, c_uint64,
          _VP, c_size_t, _VP, c_size_t, _VP]),
    ]),
    # the correlator: the exact int32 visibilities of every antenna pair of the sample tensor, integrated like the Stokes parameters
    "correlator": Companion("dcs_correlator.h", "bf_correlator.cpp", "libdcs_correlator.so", [
        ("dcs_bf_correlate_block", c_int, [_VP, c_uint32, _VP, c_size_t, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_integrate_visibilities", c_int, [_VP, _VP, c_size_t, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP]),
    ]),
    # the narrowband digital down-converter: mixer, FIR of up to 256 integer taps and decimation by 16 of the digitiser's stream
    "ddc": Companion("dcs_ddc.h", "bf_ddc.cpp", "libdcs_ddc.so", [
        ("dcs_bf_ddc_tap_digits", c_int, [_VP, _VP, c_uint32, c_uint32, _VP, c_size_t, _VP]),
        ("dcs_bf_ddc", c_int, [_VP, c_uint32, c_uint32, _VP, c_size_t, c_uint64, _VP, c_size_t, c_uint32, c_uint32, _VP, c_uint64,
                               _VP, c_size_t, c_uint64, _VP]),
    ]),
    # the candidate sifter: the signal-to-noise planes of single_pulse as a compacted, ordered list of 32-byte records
    "candidates": Companion("dcs_candidates.h", "bf_candidates.cpp", "libdcs_candidates.so", [
        ("dcs_bf_candidates_workspace_bytes", c_size_t, [c_uint32, c_uint32, c_uint32]),
        ("dcs_bf_find_candidates", c_int,
         [_VP, _VP, c_size_t, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, c_float, c_uint32, c_uint32,
          _VP, c_size_t, c_uint32, _VP, _VP, c_size_t, _VP]),
    ]),
    # the polyphase channeliser: the down-converter's float series into the int8 sample tensor (FIR, FFT, gains, corner turn)
    "channeliser": Companion("dcs_channeliser.h", "bf_channeliser.cpp", "libdcs_channeliser.so", [
        ("dcs_bf_channelise", c_int,
         [_VP, c_uint32, c_uint32, c_uint32, c_uint32, _VP, c_size_t, c_uint64, _VP, _VP, c_uint32, _VP, c_size_t, c_uint64, c_uint64,
          c_uint32, c_uint32, _VP]),
        ("dcs_bf_channelise_q8", c_int,
         [_VP, c_uint32, c_uint32, c_uint32, c_uint32, _VP, c_size_t, c_uint64, _VP, _VP, c_uint32, _VP, _VP, c_size_t, c_uint64,
          c_uint64, c_uint32, c_uint32, _VP, _VP]),
    ]),
    # the RFI flagger between the filterbanks and the dedispersion: exact statistics, cell / channel / spectrum flags, cleaned bytes
    "rfi": Companion("dcs_rfi.h", "bf_rfi.cpp", "libdcs_rfi.so", [
        ("dcs_bf_rfi_moments", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP, c_size_t, _VP]),
        ("dcs_bf_rfi_flags", c_int,
         [_VP, _VP, c_size_t, _VP, c_size_t, c_uint32, c_uint32, c_uint32, _VP, _VP, c_size_t, _VP, c_size_t, _VP, c_size_t, _VP,
          c_size_t, _VP]),
        ("dcs_bf_rfi_clean_q8", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, _VP, _VP, _VP, c_uint8, _VP, c_size_t, c_uint64,
          c_uint64, _VP, _VP]),
    ]),
    # the pulsar folder: the 8-bit filterbanks folded at a phase model into exact uint32 profiles per sub-integration, channel and
    # bin, with their hits, and the profiles' sums over frequency
    "fold": Companion("dcs_fold.h", "bf_fold.cpp", "libdcs_fold.so", [
        ("dcs_bf_fold_q8", c_int,
         [_VP, _VP, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, _VP, c_size_t, _VP, c_size_t, c_uint32, _VP,
          c_uint32, _VP, c_size_t, _VP, c_size_t, c_uint64, c_uint64, c_uint32, _VP]),
        ("dcs_bf_fold_scrunch", c_int,
         [_VP, _VP, c_size_t, c_uint32, c_uint64, c_uint64, c_uint32, c_uint32, _VP, c_size_t, c_uint32, _VP]),
    ]),
}
