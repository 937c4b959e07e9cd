"""Object wrapper over the hot-path entry points of the C-ABI.

``SteeringCoefficientGenerator`` owns one ``dcs_bf_context`` (device delay
table, double-buffered) for a fixed shape; output buffers belong to the caller
(a :class:`dc_sand_amd.device.DeviceAllocation`, a raw device pointer, or a
torch CUDA tensor's ``data_ptr()``).
"""
from __future__ import annotations

import ctypes
import dataclasses
from ctypes import byref, c_float, c_size_t, c_void_p

import numpy as np

from . import _lib
from ._lib import B32, MULTIPLE_CHANNELS_AND_TIMESTAMPS, check
from .device import _s
from .parameters import BeamformerParameters, delay_vals_dtype


def delta_times(params: BeamformerParameters, t0: int, nt: int) -> np.ndarray:
    """fDeltaTime of the reference verifier for time indices [t0, t0+nt)
    (``BeamformerCoefficientTest.cu:299`` then ``:12-18``).  Host only."""
    out = np.empty(nt, dtype=np.float32)
    cp = params.to_c()
    check(
        _lib.lib().dcs_bf_delta_times(byref(cp), int(t0), int(nt), out.ctypes.data_as(ctypes.POINTER(c_float))),
        "dcs_bf_delta_times",
    )
    return out


def ts_diff(first, last) -> np.float32:
    """``ts_diff`` of the reference verifier (``BeamformerCoefficientTest.cu:12-18``); ``first`` / ``last`` are
    ``(tv_sec, tv_nsec)`` pairs.  Host only."""
    a, b = _lib.Timespec(int(first[0]), int(first[1])), _lib.Timespec(int(last[0]), int(last[1]))
    out = c_float(0.0)
    check(_lib.lib().dcs_bf_ts_diff(byref(a), byref(b), byref(out)), "dcs_bf_ts_diff")
    return np.float32(out.value)


def _dt_array(dt) -> np.ndarray:
    return np.ascontiguousarray(np.atleast_1d(np.asarray(dt, dtype=np.float32)))


def _p(ptr) -> c_void_p:
    """An address (device or host, anything ``int()`` takes) as the C-ABI's ``void *``."""
    return c_void_p(int(ptr))


def _p_or_null(ptr) -> c_void_p:
    """:func:`_p` for an optional argument: ``None`` is NULL."""
    return c_void_p(None if ptr is None else int(ptr))


def _fp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(c_float))


def _coeff_time_entry(key, name: str, t_coeff, dt_coeff):
    """The entry point that takes the coefficient time as given: ``name`` with the time index ``t_coeff``, or
    ``name + "_dt"`` with fDeltaTime ``dt_coeff`` rounded to fp32 here; of the companion library ``key``, or with
    ``None`` of the product library.  Returns (function, its time argument, its name for ``check``)."""
    if (t_coeff is None) == (dt_coeff is None):
        raise ValueError("give exactly one of t_coeff / dt_coeff")
    lib = _lib.lib() if key is None else _lib.companion(key)
    if dt_coeff is None:
        return getattr(lib, name), int(t_coeff), name
    return getattr(lib, name + "_dt"), float(np.float32(dt_coeff)), name + "_dt"


def _timespecs(times):
    arr = (_lib.Timespec * len(times))()
    for i, (sec, nsec) in enumerate(times):
        arr[i].tv_sec, arr[i].tv_nsec = int(sec), int(nsec)
    return arr


def simulate_input(params: BeamformerParameters) -> np.ndarray:
    """The reference's linear-ramp table (``BeamformerCoefficientTest.cu:185-196``)."""
    out = np.empty(params.n_pairs, dtype=delay_vals_dtype)
    cp = params.to_c()
    check(_lib.lib().dcs_bf_simulate_input(byref(cp), c_void_p(out.ctypes.data)), "dcs_bf_simulate_input")
    return out


def output_bytes(params: BeamformerParameters, bitwidth: int, nt: int) -> int:
    n = c_size_t(0)
    cp = params.to_c()
    check(_lib.lib().dcs_bf_output_bytes(byref(cp), int(bitwidth), int(nt), byref(n)), "dcs_bf_output_bytes")
    return int(n.value)


def quantised_beams_bytes(params: BeamformerParameters, nt: int) -> int:
    """Size of the int8 beam tensor ``[C][nt / 16][B][16][{re, im}]`` of :meth:`SteeringCoefficientGenerator.beamform_accumulated_q8`."""
    return int(params.NR_CHANNELS) * int(nt) * int(params.NR_BEAMS) * 2


def block_power_bytes(params: BeamformerParameters, nt: int) -> int:
    """Size of the block power tensor ``float [C][nt / 16][B]`` of :meth:`SteeringCoefficientGenerator.beamform_accumulated_power`."""
    return int(params.NR_CHANNELS) * (int(nt) // 16) * int(params.NR_BEAMS) * 4


def power_spectra_bytes(params: BeamformerParameters, nr_blocks: int, blocks_per_spectrum: int) -> int:
    """Size of the spectra ``float [nr_blocks / blocks_per_spectrum][C][B]`` of
    :meth:`SteeringCoefficientGenerator.integrate_block_power`."""
    if blocks_per_spectrum <= 0 or nr_blocks % blocks_per_spectrum:
        raise ValueError("nr_blocks must be a multiple of blocks_per_spectrum >= 1")
    return (int(nr_blocks) // int(blocks_per_spectrum)) * int(params.NR_CHANNELS) * int(params.NR_BEAMS) * 4


def incoherent_block_power_bytes(params: BeamformerParameters, nt: int) -> int:
    """Size of the block power tensor ``uint32 [C][nt / 16]`` of :meth:`SteeringCoefficientGenerator.incoherent_block_power`."""
    return int(params.NR_CHANNELS) * (int(nt) // 16) * 4


def incoherent_spectra_bytes(params: BeamformerParameters, nr_blocks: int, blocks_per_spectrum: int) -> int:
    """Size of the spectra ``float [nr_blocks / blocks_per_spectrum][C]`` of
    :meth:`SteeringCoefficientGenerator.integrate_incoherent_power`."""
    if blocks_per_spectrum <= 0 or nr_blocks % blocks_per_spectrum:
        raise ValueError("nr_blocks must be a multiple of blocks_per_spectrum >= 1")
    return (int(nr_blocks) // int(blocks_per_spectrum)) * int(params.NR_CHANNELS) * 4


def block_stokes_bytes(params: BeamformerParameters, nt: int, nr_stokes: int) -> int:
    """Size of the block Stokes tensor ``int32 [C][nt / 16][B][nr_stokes]`` of :meth:`SteeringCoefficientGenerator.stokes_block`."""
    if nr_stokes not in (1, 4):
        raise ValueError("nr_stokes must be 1 (I) or 4 (I, Q, U, V)")
    return int(params.NR_CHANNELS) * (int(nt) // 16) * int(params.NR_BEAMS) * int(nr_stokes) * 4


def stokes_spectra_bytes(params: BeamformerParameters, nr_blocks: int, blocks_per_spectrum: int, nr_stokes: int) -> int:
    """Size of the spectra ``float [nr_blocks / blocks_per_spectrum][C][B][nr_stokes]`` of
    :meth:`SteeringCoefficientGenerator.integrate_stokes`."""
    if blocks_per_spectrum <= 0 or nr_blocks % blocks_per_spectrum:
        raise ValueError("nr_blocks must be a multiple of blocks_per_spectrum >= 1")
    if nr_stokes not in (1, 4):
        raise ValueError("nr_stokes must be 1 (I) or 4 (I, Q, U, V)")
    return (int(nr_blocks) // int(blocks_per_spectrum)) * int(params.NR_CHANNELS) * int(params.NR_BEAMS) * int(nr_stokes) * 4


def nr_baselines(nr_stations: int) -> int:
    """``NB = A (A + 1) / 2``: the antenna pairs ``(a, b)``, ``b <= a``, of the correlator; pair ``(a, b)`` has index
    ``a (a + 1) / 2 + b``."""
    a = int(nr_stations)
    return a * (a + 1) // 2


def block_visibilities_bytes(params: BeamformerParameters, nt: int, blocks_per_vis: int) -> int:
    """Size of the visibilities ``int32 [C][(nt / 16) / blocks_per_vis][NB][{re, im}]`` of
    :meth:`SteeringCoefficientGenerator.correlate_block`."""
    if not 1 <= blocks_per_vis <= 4095 or (int(nt) // 16) % blocks_per_vis:
        raise ValueError("nt / 16 must be a multiple of blocks_per_vis, which is 1 .. 4095")
    return int(params.NR_CHANNELS) * (int(nt) // 16 // int(blocks_per_vis)) * nr_baselines(params.NR_STATIONS) * 8


def visibilities_bytes(params: BeamformerParameters, nr_vis: int, vis_per_integration: int) -> int:
    """Size of the integrated visibilities ``float [nr_vis / vis_per_integration][C][NB][{re, im}]`` of
    :meth:`SteeringCoefficientGenerator.integrate_visibilities`."""
    if vis_per_integration <= 0 or nr_vis % vis_per_integration:
        raise ValueError("nr_vis must be a multiple of vis_per_integration >= 1")
    return (int(nr_vis) // int(vis_per_integration)) * int(params.NR_CHANNELS) * nr_baselines(params.NR_STATIONS) * 8


def ddc_digits_bytes(nr_taps: int) -> int:
    """Size of the operand table that :meth:`SteeringCoefficientGenerator.ddc_tap_digits` makes of ``nr_taps`` taps
    (``DCS_DDC_DIGITS_BYTES``): 16 bytes per tap, whatever the number of bands."""
    if nr_taps % 64 or not 64 <= nr_taps <= 256:
        raise ValueError("nr_taps must be 64, 128, 192 or 256")
    return 16 * int(nr_taps)


def ddc_out_bytes(nr_inputs: int, out_stride: int, nr_bands: int = 1) -> int:
    """Size of the output ``float [band][input][out_stride][{re, im}]`` of :meth:`SteeringCoefficientGenerator.ddc`."""
    if nr_bands not in (1, 2):
        raise ValueError("nr_bands must be 1 or 2")
    return int(nr_bands) * int(nr_inputs) * int(out_stride) * 8


def _channeliser_shape(nr_channels: int, nr_taps: int = 1) -> None:
    if not 64 <= nr_channels <= 2048 or nr_channels & (nr_channels - 1):
        raise ValueError("nr_channels must be a power of two in [64, 2048]")
    if not 1 <= nr_taps <= 16:
        raise ValueError("nr_taps must be in [1, 16]")


def channeliser_in_pairs(nr_channels: int, nr_taps: int, nr_spectra: int) -> int:
    """The pairs of a row that :meth:`SteeringCoefficientGenerator.channelise` reads for ``nr_spectra`` spectra
    (``DCS_CHAN_IN_PAIRS``): ``(nr_spectra + nr_taps - 1) nr_channels``, the least ``in_stride``."""
    _channeliser_shape(int(nr_channels), int(nr_taps))
    if nr_spectra < 0 or nr_spectra % 16:
        raise ValueError("nr_spectra must be a multiple of 16")
    return (int(nr_spectra) + int(nr_taps) - 1) * int(nr_channels)


def channelised_bytes(nr_channels: int, out_blocks: int, out_inputs: int, q8: bool = False) -> int:
    """Size of the output ``[nr_channels][out_blocks][out_inputs][16][{re, im}]`` of
    :meth:`SteeringCoefficientGenerator.channelise` (floats) or, with ``q8``, ``.channelise_q8`` (int8: the sample tensor of
    ``nr_channels`` channels, ``out_inputs`` stations and ``16 out_blocks`` samples)."""
    _channeliser_shape(int(nr_channels))
    return int(nr_channels) * int(out_blocks) * int(out_inputs) * 32 * (1 if q8 else 4)


def spectra_sums_bytes(params: BeamformerParameters, nr_beams: int) -> int:
    """Size of the running sums ``double [C][nr_beams][2]`` of :meth:`SteeringCoefficientGenerator.spectra_sums`."""
    return int(params.NR_CHANNELS) * int(nr_beams) * 16


def filterbank_scales_bytes(params: BeamformerParameters, nr_beams: int) -> int:
    """Size of the scales ``float [C][nr_beams][2]`` of :meth:`SteeringCoefficientGenerator.filterbank_scales`."""
    return int(params.NR_CHANNELS) * int(nr_beams) * 8


def filterbank_bytes(params: BeamformerParameters, nr_beams: int, out_spectra: int) -> int:
    """Size of the filterbanks ``uint8 [nr_beams][out_spectra][C]`` of :meth:`SteeringCoefficientGenerator.filterbank_q8`."""
    return int(nr_beams) * int(out_spectra) * int(params.NR_CHANNELS)


def dm_delays_bytes(params: BeamformerParameters, nr_dm: int) -> int:
    """Size of the delay table ``int32 [nr_dm][C]`` of :meth:`SteeringCoefficientGenerator.dm_delays`."""
    return int(nr_dm) * int(params.NR_CHANNELS) * 4


def dm_time_bytes(nr_beams: int, nr_dm: int, out_spectra: int) -> int:
    """Size of the DM-time planes ``uint32 [nr_beams][nr_dm][out_spectra]`` of
    :meth:`SteeringCoefficientGenerator.dedisperse_q8`."""
    return int(nr_beams) * int(nr_dm) * int(out_spectra) * 4


def rfi_cell_sums_bytes(params: BeamformerParameters, nr_beams: int, nr_blocks: int) -> int:
    """Size of the cell sums ``uint32 [nr_beams][nr_blocks][C][2]`` of :meth:`SteeringCoefficientGenerator.rfi_moments`."""
    return int(nr_beams) * int(nr_blocks) * int(params.NR_CHANNELS) * 8


def rfi_zero_dm_bytes(nr_beams: int, nr_spectra: int) -> int:
    """Size of the zero-DM series ``uint32 [nr_beams][nr_spectra]`` of :meth:`SteeringCoefficientGenerator.rfi_moments`;
    ``nr_spectra`` is the window, ``nr_blocks * block_len``."""
    return int(nr_beams) * int(nr_spectra) * 4


def rfi_cell_flags_bytes(params: BeamformerParameters, nr_beams: int, nr_blocks: int) -> int:
    """Size of the cell flags ``uint8 [nr_beams][nr_blocks][C]`` of :meth:`SteeringCoefficientGenerator.rfi_flags`."""
    return int(nr_beams) * int(nr_blocks) * int(params.NR_CHANNELS)


def rfi_channel_mask_bytes(params: BeamformerParameters, nr_beams: int) -> int:
    """Size of the channel masks ``uint8 [nr_beams][C]`` of :meth:`SteeringCoefficientGenerator.rfi_flags`."""
    return int(nr_beams) * int(params.NR_CHANNELS)


def rfi_spectrum_flags_bytes(nr_beams: int, nr_spectra: int) -> int:
    """Size of the spectrum flags ``uint8 [nr_beams][nr_spectra]`` of :meth:`SteeringCoefficientGenerator.rfi_flags`."""
    return int(nr_beams) * int(nr_spectra)


def rfi_counts_bytes(nr_beams: int) -> int:
    """Size of the counts ``uint32 [nr_beams][3]`` of :meth:`SteeringCoefficientGenerator.rfi_flags`."""
    return int(nr_beams) * 12


def fold_profiles_bytes(params: BeamformerParameters, nr_beams: int, out_subints: int, nbin: int) -> int:
    """Size of the profiles ``uint32 [nr_beams][out_subints][C][nbin]`` of :meth:`SteeringCoefficientGenerator.fold_q8`."""
    return int(nr_beams) * int(out_subints) * int(params.NR_CHANNELS) * int(nbin) * 4


def fold_hits_bytes(nr_models: int, out_subints: int, nbin: int) -> int:
    """Size of the hits ``uint32 [nr_models][out_subints][nbin]`` of :meth:`SteeringCoefficientGenerator.fold_q8`;
    ``nr_models`` is ``nr_beams // beams_per_model``."""
    return int(nr_models) * int(out_subints) * int(nbin) * 4


def fold_scrunched_bytes(nr_beams: int, out_subints: int, nbin: int) -> int:
    """Size of the plane ``uint64 [nr_beams][out_subints][nbin]`` of :meth:`SteeringCoefficientGenerator.fold_scrunch`."""
    return int(nr_beams) * int(out_subints) * int(nbin) * 8


@dataclasses.dataclass(frozen=True)
class RfiThresholds:
    """``dcs_bf_rfi_thresholds`` (include/dcs_rfi.h): an element is an outlier iff its distance from the lower median is
    above ``max(thr * MAD, floor)``; a channel is masked with more than ``max_bad_blocks`` flagged cells."""
    mean_thr: float = 6.0
    mean_floor: float = 0.0
    var_thr: float = 6.0
    var_floor: float = 0.0
    zero_dm_thr: float = 6.0
    zero_dm_floor: float = 0.0
    max_bad_blocks: int = 0


class _RfiThresholds(ctypes.Structure):  # dcs_bf_rfi_thresholds (include/dcs_rfi.h)
    _fields_ = [("mean_thr", ctypes.c_double), ("mean_floor", ctypes.c_double), ("var_thr", ctypes.c_double),
                ("var_floor", ctypes.c_double), ("zero_dm_thr", ctypes.c_double), ("zero_dm_floor", ctypes.c_double),
                ("max_bad_blocks", ctypes.c_uint32)]


def dm_time_sums_bytes(nr_beams: int, nr_dm: int) -> int:
    """Size of the sums ``uint64 [nr_beams][nr_dm][2]`` of :meth:`SteeringCoefficientGenerator.dm_time_sums`."""
    return int(nr_beams) * int(nr_dm) * 16


def boxcar_peaks_bytes(nr_beams: int, nr_dm: int, nr_widths: int, peak_blocks: int) -> int:
    """Size of the peak plane ``uint32 [nr_beams][nr_dm][nr_widths][peak_blocks][2]`` of
    :meth:`SteeringCoefficientGenerator.boxcar_peaks`."""
    return int(nr_beams) * int(nr_dm) * int(nr_widths) * int(peak_blocks) * 8


def peak_snr_bytes(nr_beams: int, nr_dm: int, nr_widths: int, peak_blocks: int) -> int:
    """Size of the signal-to-noise ``float [nr_beams][nr_dm][nr_widths][peak_blocks]`` of
    :meth:`SteeringCoefficientGenerator.peak_snr`."""
    return int(nr_beams) * int(nr_dm) * int(nr_widths) * int(peak_blocks) * 4


def best_width_bytes(nr_beams: int, nr_dm: int, peak_blocks: int) -> int:
    """Size of the best width indices ``uint32 [nr_beams][nr_dm][peak_blocks]`` of
    :meth:`SteeringCoefficientGenerator.peak_snr`."""
    return int(nr_beams) * int(nr_dm) * int(peak_blocks) * 4


# dcs_bf_candidate (include/dcs_candidates.h): one single-pulse candidate, 32 bytes
candidate_dtype = np.dtype([("beam", np.uint32), ("dm", np.uint32), ("width_index", np.uint32), ("block", np.uint32),
                            ("time", np.uint32), ("value", np.uint32), ("snr", np.float32), ("members", np.uint32)])
# The sifter's geometry (dc_sand_amd/csrc/bf_arg_checks.h, bf_candidates.hip): a tile is CANDIDATES_TILE_DMS DMs by
# CANDIDATES_TILE_BLOCKS blocks, a segment one row of a tile; the scan takes CANDIDATES_SCAN_SPAN segments per round
CANDIDATES_TILE_DMS, CANDIDATES_TILE_BLOCKS, CANDIDATES_MAX_RADIUS, CANDIDATES_SCAN_SPAN = 16, 64, 8, 4096


def candidates_bytes(max_candidates: int) -> int:
    """Size of the record array ``dcs_bf_candidate [max_candidates]`` (:data:`candidate_dtype`) of
    :meth:`SteeringCoefficientGenerator.find_candidates`."""
    return int(max_candidates) * candidate_dtype.itemsize


def candidates_workspace_bytes(nr_beams: int, nr_dm: int, nr_blocks: int) -> int:
    """``dcs_bf_candidates_workspace_bytes``: the bytes of ``d_work`` for a
    :meth:`SteeringCoefficientGenerator.find_candidates` call of this shape.  Host only."""
    return int(_lib.companion("candidates").dcs_bf_candidates_workspace_bytes(int(nr_beams), int(nr_dm), int(nr_blocks)))


class _DdcBand(ctypes.Structure):  # dcs_ddc_band (include/dcs_ddc.h)
    _fields_ = [("phase_step", ctypes.c_uint32), ("phase0", ctypes.c_uint32), ("gain", ctypes.c_float)]


class _Band(ctypes.Structure):  # dcs_bf_band (include/dcs_dedisperse.h)
    _fields_ = [("freq_first_mhz", ctypes.c_double), ("freq_step_mhz", ctypes.c_double), ("sample_time_s", ctypes.c_double)]


def gpu_utilisation(params: BeamformerParameters, kernel_ms: float) -> tuple[float, float]:
    """``BeamformerCoeffTest::get_time`` model (``BeamformerCoefficientTest.cu:426-448``)."""
    out = (c_float * 2)()
    cp = params.to_c()
    check(_lib.lib().dcs_bf_gpu_utilisation(byref(cp), float(kernel_ms), out), "dcs_bf_gpu_utilisation")
    return float(out[0]), float(out[1])


class SteeringCoefficientGenerator:
    def __init__(self, params: BeamformerParameters):
        self.params = params
        self._cp = params.to_c()
        h = c_void_p()
        check(_lib.lib().dcs_bf_create(byref(self._cp), byref(h)), "dcs_bf_create")
        self._h = h.value
        self._host_table = None  # keeps the last uploaded table alive during the async copy

    # -- delay table ------------------------------------------------------
    def upload_delays(self, table: np.ndarray, stream=None) -> None:
        """transfer_HtoD (``BeamformerCoefficientTest.cu:207-216``)."""
        table = np.ascontiguousarray(table)
        if table.dtype != delay_vals_dtype or table.size != self.params.n_pairs:
            raise ValueError(f"delay table must be {self.params.n_pairs} x delay_vals_dtype")
        self._host_table = table
        check(_lib.lib().dcs_bf_upload_delays(c_void_p(self._h), c_void_p(table.ctypes.data), _s(stream)), "dcs_bf_upload_delays")

    def set_delays_from_global(self, d_global_table: int, nr_beams_total: int, beam_offset: int, stream=None) -> None:
        """Take beams [beam_offset, beam_offset+NR_BEAMS) of a device-resident
        global table [NR_STATIONS][nr_beams_total] (multi-GPU beam sharding)."""
        check(
            _lib.lib().dcs_bf_set_delays_from_global(
                c_void_p(self._h), c_void_p(int(d_global_table)), int(nr_beams_total), int(beam_offset), _s(stream)
            ),
            "dcs_bf_set_delays_from_global",
        )

    # -- generation -------------------------------------------------------
    def generate(self, d_out, out_bytes: int, t0: int = 0, nt: int = 1, kernel: int = MULTIPLE_CHANNELS_AND_TIMESTAMPS,
                 bitwidth: int = B32, stream=None) -> None:
        """run_kernel (``BeamformerCoefficientTest.cu:218-264``)."""
        check(
            _lib.lib().dcs_bf_generate(c_void_p(self._h), int(kernel), int(bitwidth), int(t0), int(nt), c_void_p(int(d_out)),
                                       int(out_bytes), _s(stream)),
            "dcs_bf_generate",
        )

    def generate_slab(self, d_out, out_bytes: int, c0: int, nc: int, t0: int = 0, nt: int = 1, bitwidth: int = B32,
                      stream=None) -> None:
        check(
            _lib.lib().dcs_bf_generate_slab(c_void_p(self._h), int(bitwidth), int(t0), int(nt), int(c0), int(nc),
                                            c_void_p(int(d_out)), int(out_bytes), _s(stream)),
            "dcs_bf_generate_slab",
        )

    def generate_dt(self, d_out, out_bytes: int, dt, kernel: int = MULTIPLE_CHANNELS_AND_TIMESTAMPS, bitwidth: int = B32,
                    stream=None) -> None:
        """As :meth:`generate` with fDeltaTime of every time step given by value (``dcs_bf_generate_dt``)."""
        a = _dt_array(dt)
        check(
            _lib.lib().dcs_bf_generate_dt(c_void_p(self._h), int(kernel), int(bitwidth), a.ctypes.data_as(ctypes.POINTER(c_float)),
                                          a.size, c_void_p(int(d_out)), int(out_bytes), _s(stream)),
            "dcs_bf_generate_dt",
        )

    def generate_slab_dt(self, d_out, out_bytes: int, c0: int, nc: int, dt, bitwidth: int = B32, stream=None) -> None:
        a = _dt_array(dt)
        check(
            _lib.lib().dcs_bf_generate_slab_dt(c_void_p(self._h), int(bitwidth), a.ctypes.data_as(ctypes.POINTER(c_float)), a.size,
                                               int(c0), int(nc), c_void_p(int(d_out)), int(out_bytes), _s(stream)),
            "dcs_bf_generate_slab_dt",
        )

    def generate_at(self, d_out, out_bytes: int, current_times, reference_time, kernel: int = MULTIPLE_CHANNELS_AND_TIMESTAMPS,
                    bitwidth: int = B32, stream=None) -> None:
        """The reference kernels' own time arguments (``struct timespec sCurrentTime, sRefTime``,
        ``BeamformerKernels.cuh:38-42``): one ``(tv_sec, tv_nsec)`` per time step and one reference."""
        cur = _timespecs(list(current_times))
        ref = _lib.Timespec(int(reference_time[0]), int(reference_time[1]))
        check(
            _lib.lib().dcs_bf_generate_at(c_void_p(self._h), int(kernel), int(bitwidth), cur, byref(ref), len(cur),
                                          c_void_p(int(d_out)), int(out_bytes), _s(stream)),
            "dcs_bf_generate_at",
        )

    def generate_and_beamform_dt(self, d_antenna, antenna_bytes: int, d_beams, beams_bytes: int, dt, stream=None) -> None:
        a = _dt_array(dt)
        check(
            _lib.lib().dcs_bf_generate_and_beamform_dt(c_void_p(self._h), _fp(a), a.size, _p(d_antenna), int(antenna_bytes), _p(d_beams),
                                                       int(beams_bytes), _s(stream)),
            "dcs_bf_generate_and_beamform_dt",
        )

    def generate_and_beamform(self, d_antenna, antenna_bytes: int, d_beams, beams_bytes: int, t0: int = 0,
                              nt: int | None = None, stream=None) -> None:
        """Fused coefficient generation + beamforming (run_kernel's COMBINED branch,
        ``BeamformerCoefficientTest.cu:259-262``); the table is indexed [beam*A + antenna]."""
        nt = self.params.NR_SAMPLES_PER_CHANNEL if nt is None else nt
        check(
            _lib.lib().dcs_bf_generate_and_beamform(c_void_p(self._h), int(t0), int(nt), _p(d_antenna), int(antenna_bytes), _p(d_beams),
                                                    int(beams_bytes), _s(stream)),
            "dcs_bf_generate_and_beamform",
        )

    def beamform_accumulated(self, d_antenna, antenna_bytes: int, d_beams, beams_bytes: int, nt: int, t_coeff: int | None = None,
                             dt_coeff: float | None = None, stream=None) -> None:
        """Beamformer with coefficient reuse on the matrix cores (``dcs_bf_beamform_accumulated``): the coefficients of
        ONE time (time index ``t_coeff`` or fDeltaTime ``dt_coeff``) applied to ``nt`` samples; table indexed [beam*A + antenna]."""
        fn, when, where = _coeff_time_entry(None, "dcs_bf_beamform_accumulated", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p(d_beams), int(beams_bytes), _s(stream)), where)

    # -- per-input beam weights (include/dcs_beam_weights.h, companion library libdcs_beam_weights.so): d_weights is a
    #    device [nr_beams][nr_stations] fp32 array (:class:`dc_sand_amd.beam_weights.BeamWeights.device_ptr`), read when
    #    the work runs on the stream
    def generate_and_beamform_weighted(self, d_antenna, antenna_bytes: int, d_weights, d_beams, beams_bytes: int,
                                       t0: int = 0, nt: int | None = None, dt=None, stream=None) -> None:
        """:meth:`generate_and_beamform` (or, with ``dt``, :meth:`generate_and_beamform_dt`) with per-input beam weights."""
        wl = _lib.companion("beam_weights")
        tail = (_p(d_antenna), int(antenna_bytes), _p(d_weights), _p(d_beams), int(beams_bytes), _s(stream))
        if dt is not None:
            a = _dt_array(dt)
            check(wl.dcs_bf_generate_and_beamform_weighted_dt(c_void_p(self._h), _fp(a), a.size, *tail),
                  "dcs_bf_generate_and_beamform_weighted_dt")
            return
        nt = self.params.NR_SAMPLES_PER_CHANNEL if nt is None else nt
        check(wl.dcs_bf_generate_and_beamform_weighted(c_void_p(self._h), int(t0), int(nt), *tail), "dcs_bf_generate_and_beamform_weighted")

    def beamform_accumulated_weighted(self, d_antenna, antenna_bytes: int, d_weights, d_beams, beams_bytes: int, nt: int,
                                      t_coeff: int | None = None, dt_coeff: float | None = None, stream=None) -> None:
        """:meth:`beamform_accumulated` with per-input beam weights."""
        fn, when, where = _coeff_time_entry("beam_weights", "dcs_bf_beamform_accumulated_weighted", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p(d_weights), _p(d_beams), int(beams_bytes),
                 _s(stream)), where)

    # -- quantised int8 beam output (include/dcs_beam_quant.h, companion library libdcs_beam_quant.so): d_quant_gains is a
    #    device [nr_beams] fp32 array, d_clip_count a device [nr_beams] uint64 array or None
    #    (:class:`dc_sand_amd.beam_quant.BeamQuantGains`), both read and written when the work runs on the stream
    def beamform_accumulated_q8(self, d_antenna, antenna_bytes: int, d_quant_gains, d_beams_q8, beams_bytes: int, nt: int,
                                t_coeff: int | None = None, dt_coeff: float | None = None, d_weights=None, d_clip_count=None,
                                stream=None) -> None:
        """:meth:`beamform_accumulated` (with ``d_weights``: :meth:`beamform_accumulated_weighted`) whose epilogue
        requantises every beam to int8 with its gain: ``q = clamp(rint(v * k_b), -127, 127)``, NaN -> -128; the int8
        tensor is ``[C][nt / 16][B][16][{re, im}]`` (:func:`quantised_beams_bytes`)."""
        fn, when, where = _coeff_time_entry("beam_quant", "dcs_bf_beamform_accumulated_q8", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p_or_null(d_weights), _p(d_quant_gains),
                 _p(d_beams_q8), int(beams_bytes), _p_or_null(d_clip_count), _s(stream)), where)

    # -- detected beam power (include/dcs_beam_power.h, companion library libdcs_beam_power.so): d_block_power is a device
    #    float [C][nt / 16][B] array, d_spectra a device float [nr_blocks / blocks_per_spectrum][C][B] array
    def beamform_accumulated_power(self, d_antenna, antenna_bytes: int, d_block_power, power_bytes: int, nt: int,
                                   t_coeff: int | None = None, dt_coeff: float | None = None, d_weights=None, stream=None) -> None:
        """:meth:`beamform_accumulated` (with ``d_weights``: :meth:`beamform_accumulated_weighted`) whose epilogue
        detects: ``|v|^2`` of every sample, summed pairwise over each 16-sample block, one float per (channel, block,
        beam) (:func:`block_power_bytes`)."""
        fn, when, where = _coeff_time_entry("beam_power", "dcs_bf_beamform_accumulated_power", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p_or_null(d_weights), _p(d_block_power),
                 int(power_bytes), _s(stream)), where)

    def integrate_block_power(self, d_block_power, power_bytes: int, nr_blocks: int, blocks_per_spectrum: int, d_spectra,
                              spectra_bytes: int, accumulate: bool = False, stream=None) -> None:
        """Sums the block powers ``[C][nr_blocks][B]`` ``blocks_per_spectrum`` at a time, in order, into the spectra
        ``[nr_blocks / blocks_per_spectrum][C][B]`` (:func:`power_spectra_bytes`); with ``accumulate`` the sums start
        from what ``d_spectra`` holds, so an integration can span calls."""
        pl = _lib.companion("beam_power")
        check(pl.dcs_bf_integrate_block_power(c_void_p(self._h), _p(d_block_power), int(power_bytes), int(nr_blocks),
                                              int(blocks_per_spectrum), 1 if accumulate else 0, _p(d_spectra), int(spectra_bytes),
                                              _s(stream)),
              "dcs_bf_integrate_block_power")

    # -- the true complex product, tied-array beams (include/dcs_beam_complex.h, companion library libdcs_beam_complex.so):
    #    sum_a w_a x_a, or with ``conjugate`` sum_a conj(w_a) x_a, instead of the element-wise product; tensors as
    #    :meth:`beamform_accumulated` and :meth:`beamform_accumulated_power`
    def beamform_accumulated_complex(self, d_antenna, antenna_bytes: int, d_beams, beams_bytes: int, nt: int,
                                     t_coeff: int | None = None, dt_coeff: float | None = None, d_weights=None,
                                     conjugate: bool = False, stream=None) -> None:
        """:meth:`beamform_accumulated` (with ``d_weights``: :meth:`beamform_accumulated_weighted`) with the complex
        product: ``re = sum(w_re x_re - s w_im x_im)``, ``im = sum(w_re x_im + s w_im x_re)``, ``s = -1`` with ``conjugate``."""
        fn, when, where = _coeff_time_entry("beam_complex", "dcs_bf_beamform_accumulated_complex", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p_or_null(d_weights), 1 if conjugate else 0,
                 _p(d_beams), int(beams_bytes), _s(stream)), where)

    def beamform_accumulated_complex_power(self, d_antenna, antenna_bytes: int, d_block_power, power_bytes: int, nt: int,
                                           t_coeff: int | None = None, dt_coeff: float | None = None, d_weights=None,
                                           conjugate: bool = False, stream=None) -> None:
        """:meth:`beamform_accumulated_complex` whose epilogue detects, as :meth:`beamform_accumulated_power` does: one float
        per (channel, block, beam) (:func:`block_power_bytes`), which :meth:`integrate_block_power` and the filterbank calls take."""
        fn, when, where = _coeff_time_entry("beam_complex", "dcs_bf_beamform_accumulated_complex_power", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p_or_null(d_weights), 1 if conjugate else 0,
                 _p(d_block_power), int(power_bytes), _s(stream)), where)

    # -- 8-bit voltage beams of the complex product (include/dcs_beam_complex_quant.h, companion library
    #    libdcs_beam_complex_quant.so): gains, counters and the int8 tensor as :meth:`beamform_accumulated_q8`
    def beamform_accumulated_complex_q8(self, d_antenna, antenna_bytes: int, d_quant_gains, d_beams_q8, beams_bytes: int, nt: int,
                                        t_coeff: int | None = None, dt_coeff: float | None = None, d_weights=None,
                                        conjugate: bool = False, d_clip_count=None, stream=None) -> None:
        """:meth:`beamform_accumulated_complex` whose epilogue requantises every beam to int8 with its gain, as
        :meth:`beamform_accumulated_q8` does: the bytes are the quantised floats of the complex float call, in the antenna
        tensor's order (:func:`quantised_beams_bytes`), so they can be the ``d_antenna`` of a second beamformer."""
        fn, when, where = _coeff_time_entry("beam_complex_quant", "dcs_bf_beamform_accumulated_complex_q8", t_coeff, dt_coeff)
        check(fn(c_void_p(self._h), when, int(nt), _p(d_antenna), int(antenna_bytes), _p_or_null(d_weights), 1 if conjugate else 0,
                 _p(d_quant_gains), _p(d_beams_q8), int(beams_bytes), _p_or_null(d_clip_count), _s(stream)), where)

    # -- the incoherent beam (include/dcs_incoherent_beam.h, companion library libdcs_incoherent_beam.so): d_block_power is a
    #    device uint32 [C][nt / 16] array, d_spectra a device float [nr_blocks / blocks_per_spectrum][C] array
    def incoherent_block_power(self, d_antenna, antenna_bytes: int, d_block_power, power_bytes: int, nt: int, d_weights=None,
                               stream=None) -> None:
        """The antennas' own power, ``re^2 + im^2`` summed over every 16-sample block and over the antennas taking part, as
        exact integers, one per (channel, block) (:func:`incoherent_block_power_bytes`).  ``d_weights``: ``None``, or a
        device ``float [A]`` array of FLAGS -- antenna ``a`` takes part iff its value is not 0; other values do not scale."""
        il = _lib.companion("incoherent_beam")
        check(il.dcs_bf_incoherent_block_power(c_void_p(self._h), int(nt), _p(d_antenna), int(antenna_bytes), _p_or_null(d_weights),
                                               _p(d_block_power), int(power_bytes), _s(stream)),
              "dcs_bf_incoherent_block_power")

    def integrate_incoherent_power(self, d_block_power, power_bytes: int, nr_blocks: int, blocks_per_spectrum: int, d_spectra,
                                   spectra_bytes: int, accumulate: bool = False, stream=None) -> None:
        """Sums the block powers ``[C][nr_blocks]`` ``blocks_per_spectrum`` at a time, exactly, into the spectra
        ``[nr_blocks / blocks_per_spectrum][C]`` (:func:`incoherent_spectra_bytes`), each sum rounded to float once; with
        ``accumulate`` it is added to what ``d_spectra`` holds, so an integration can span calls."""
        il = _lib.companion("incoherent_beam")
        check(il.dcs_bf_integrate_incoherent_power(c_void_p(self._h), _p(d_block_power), int(power_bytes), int(nr_blocks),
                                                   int(blocks_per_spectrum), 1 if accumulate else 0, _p(d_spectra),
                                                   int(spectra_bytes), _s(stream)),
              "dcs_bf_integrate_incoherent_power")

    # -- full-Stokes detection of two polarisations' 8-bit beams (include/dcs_stokes.h, companion library libdcs_stokes.so):
    #    d_beams_x and d_beams_y are device int8 [C][nt / 16][B][16][2] arrays (what beamform_accumulated_complex_q8 writes),
    #    d_block_stokes a device int32 [C][nt / 16][B][nr_stokes] array, d_spectra a device float
    #    [nr_blocks / blocks_per_spectrum][C][B][nr_stokes] array
    def stokes_block(self, d_beams_x, d_beams_y, beams_bytes: int, d_block_stokes, stokes_bytes: int, nt: int, nr_stokes: int = 4,
                     stream=None) -> None:
        """The Stokes parameters of every 16-sample block of the beams of polarisations x and y, as exact integers
        (:func:`block_stokes_bytes`): ``I = Pxx + Pyy`` with ``nr_stokes = 1``; ``I``, ``Q = Pxx - Pyy``,
        ``U = 2 Re sum x conj(y)``, ``V = 2 Im sum x conj(y)``, innermost, with ``nr_stokes = 4``."""
        sl = _lib.companion("stokes")
        check(sl.dcs_bf_stokes_block(c_void_p(self._h), int(nt), _p(d_beams_x), _p(d_beams_y), int(beams_bytes), int(nr_stokes),
                                     _p(d_block_stokes), int(stokes_bytes), _s(stream)),
              "dcs_bf_stokes_block")

    def integrate_stokes(self, d_block_stokes, stokes_bytes: int, nr_blocks: int, blocks_per_spectrum: int, nr_stokes: int,
                         d_spectra, spectra_bytes: int, accumulate: bool = False, stream=None) -> None:
        """Sums the block Stokes parameters ``[C][nr_blocks][B][nr_stokes]`` ``blocks_per_spectrum`` at a time, exactly,
        into the spectra ``[nr_blocks / blocks_per_spectrum][C][B][nr_stokes]`` (:func:`stokes_spectra_bytes`), each sum
        rounded to float once; with ``accumulate`` it is added to what ``d_spectra`` holds, so an integration can span
        calls.  The spectra are those of the filterbank calls with ``nr_beams = nr_stokes * B``."""
        sl = _lib.companion("stokes")
        check(sl.dcs_bf_integrate_stokes(c_void_p(self._h), _p(d_block_stokes), int(stokes_bytes), int(nr_blocks),
                                         int(blocks_per_spectrum), int(nr_stokes), 1 if accumulate else 0, _p(d_spectra),
                                         int(spectra_bytes), _s(stream)),
              "dcs_bf_integrate_stokes")

    # -- 8-bit search filterbanks (include/dcs_filterbank.h, companion library libdcs_filterbank.so): d_spectra is a device
    #    float [nr_spectra][C][nr_beams] array -- nr_beams the context's for detected spectra, 1 for incoherent ones, 4 times
    #    the context's for IQUV Stokes spectra
    def spectra_sums(self, d_spectra, spectra_bytes: int, nr_spectra: int, nr_beams: int, d_sums, sums_bytes: int,
                     accumulate: bool = False, stream=None) -> None:
        """Running fp64 sums ``{sum x, sum x^2}`` per (channel, beam) over the spectra, in time order, into ``d_sums``
        (:func:`spectra_sums_bytes`); with ``accumulate`` they start from what ``d_sums`` holds."""
        fl = _lib.companion("filterbank")
        check(fl.dcs_bf_spectra_sums(c_void_p(self._h), _p(d_spectra), int(spectra_bytes), int(nr_spectra), int(nr_beams),
                                     1 if accumulate else 0, _p(d_sums), int(sums_bytes), _s(stream)),
              "dcs_bf_spectra_sums")

    def filterbank_scales(self, d_sums, sums_bytes: int, count: int, nr_beams: int, target_std: float, d_scales,
                          scales_bytes: int, stream=None) -> None:
        """The sums of ``count`` spectra to the scales ``{mean, target_std / standard deviation}`` per (channel, beam)
        (:func:`filterbank_scales_bytes`); a channel without variance gets gain 0."""
        fl = _lib.companion("filterbank")
        check(fl.dcs_bf_filterbank_scales(c_void_p(self._h), _p(d_sums), int(sums_bytes), int(count), int(nr_beams),
                                          float(np.float32(target_std)), _p(d_scales), int(scales_bytes), _s(stream)),
              "dcs_bf_filterbank_scales")

    def filterbank_q8(self, d_spectra, spectra_bytes: int, nr_spectra: int, nr_beams: int, d_scales, level: float, d_filterbank,
                      filterbank_bytes: int, out_spectra: int, first_spectrum: int = 0, descending: bool = False,
                      d_clip_count=None, stream=None) -> None:
        """``clamp(rint((x - mean) * gain + level), 0, 255)`` of every spectrum into rows ``first_spectrum ..`` of the
        per-beam filterbanks ``uint8 [nr_beams][out_spectra][C]`` (:func:`filterbank_bytes`); ``descending`` reverses the
        channel order; ``d_clip_count``: ``None``, or a zeroed device ``uint64 [nr_beams]`` array of clipped elements."""
        fl = _lib.companion("filterbank")
        check(fl.dcs_bf_filterbank_q8(c_void_p(self._h), _p(d_spectra), int(spectra_bytes), int(nr_spectra), int(nr_beams),
                                      _p(d_scales), float(np.float32(level)), 1 if descending else 0, _p(d_filterbank),
                                      int(filterbank_bytes), int(out_spectra), int(first_spectrum), _p_or_null(d_clip_count),
                                      _s(stream)),
              "dcs_bf_filterbank_q8")

    # -- incoherent dedispersion of those filterbanks (include/dcs_dedisperse.h, companion library libdcs_dedisperse.so):
    #    d_delays a device int32 [nr_dm][C] array, d_dm_time a device uint32 [nr_beams][nr_dm][out_spectra] array
    def dm_delays(self, freq_first_mhz: float, freq_step_mhz: float, sample_time_s: float, d_dms, nr_dm: int, d_delays,
                  delays_bytes: int, stream=None) -> None:
        """The delays, in whole spectra of ``sample_time_s``, of every filterbank column (column ``j`` at
        ``freq_first_mhz + j * freq_step_mhz``) against the band's highest column for the DMs of the device
        ``double [nr_dm]`` array ``d_dms``, into ``d_delays`` (:func:`dm_delays_bytes`); fp64, rounded once per operation."""
        band = _Band(float(freq_first_mhz), float(freq_step_mhz), float(sample_time_s))
        dl = _lib.companion("dedisperse")
        check(dl.dcs_bf_dm_delays(c_void_p(self._h), ctypes.cast(ctypes.pointer(band), c_void_p), _p(d_dms), int(nr_dm),
                                  _p(d_delays), int(delays_bytes), _s(stream)),
              "dcs_bf_dm_delays")

    def dedisperse_q8(self, d_filterbank, filterbank_bytes: int, in_spectra: int, first_spectrum: int, nr_spectra: int,
                      nr_beams: int, d_delays, nr_dm: int, max_delay: int, d_dm_time, dm_time_bytes: int, out_spectra: int,
                      first_out: int = 0, d_channel_mask=None, stream=None) -> None:
        """Per beam, DM ``m`` and ``t < nr_spectra``: word ``first_out + t`` of series ``m`` of the planes
        (:func:`dm_time_bytes`) becomes the exact sum over the columns ``c`` of filterbank byte
        ``[first_spectrum + t + d_delays[m][c]][c]``; entries outside ``[0, max_delay]`` and the columns whose byte of
        ``d_channel_mask`` (``None``, or a device ``uint8 [C]`` array) is zero drop out."""
        dl = _lib.companion("dedisperse")
        check(dl.dcs_bf_dedisperse_q8(c_void_p(self._h), _p(d_filterbank), int(filterbank_bytes), int(in_spectra),
                                      int(first_spectrum), int(nr_spectra), int(nr_beams), _p(d_delays), int(nr_dm),
                                      int(max_delay), _p_or_null(d_channel_mask), _p(d_dm_time), int(dm_time_bytes),
                                      int(out_spectra), int(first_out), _s(stream)),
              "dcs_bf_dedisperse_q8")

    # -- the RFI flagger between the filterbanks and the dedispersion (include/dcs_rfi.h, companion library libdcs_rfi.so): the
    #    window of every call is nr_blocks blocks of block_len spectra from first_spectrum on
    def rfi_moments(self, d_filterbank, filterbank_bytes: int, in_spectra: int, first_spectrum: int, nr_blocks: int,
                    block_len: int, nr_beams: int, d_cell_sums, cell_sums_bytes: int, d_zero_dm=None, zero_dm_bytes: int = 0,
                    stream=None) -> None:
        """Per (beam, block, channel) the exact ``{sum x, sum x^2}`` of the block's ``block_len`` bytes into ``d_cell_sums``
        (:func:`rfi_cell_sums_bytes`) and, with ``d_zero_dm`` (:func:`rfi_zero_dm_bytes`), per beam and spectrum of the
        window the sum of the spectrum's bytes over the channels."""
        rl = _lib.companion("rfi")
        check(rl.dcs_bf_rfi_moments(c_void_p(self._h), _p(d_filterbank), int(filterbank_bytes), int(in_spectra),
                                    int(first_spectrum), int(nr_blocks), int(block_len), int(nr_beams), _p(d_cell_sums),
                                    int(cell_sums_bytes), _p_or_null(d_zero_dm), int(zero_dm_bytes), _s(stream)),
              "dcs_bf_rfi_moments")

    def rfi_flags(self, d_cell_sums, cell_sums_bytes: int, nr_blocks: int, block_len: int, nr_beams: int, d_cell_flags,
                  cell_flags_bytes: int, d_channel_mask, channel_mask_bytes: int, d_counts, counts_bytes: int,
                  thresholds: RfiThresholds = RfiThresholds(), d_zero_dm=None, zero_dm_bytes: int = 0, d_spectrum_flags=None,
                  spectrum_flags_bytes: int = 0, stream=None) -> None:
        """The statistics of :meth:`rfi_moments` to flags by a lower median and median absolute deviation across the
        channels of every (beam, block): bit 0 of a cell's flag (:func:`rfi_cell_flags_bytes`) for its sum, bit 1 for
        ``n * s2 - s1^2``; a channel's mask byte (:func:`rfi_channel_mask_bytes`) is 0 with more than
        ``thresholds.max_bad_blocks`` flagged cells, else 1; with ``d_zero_dm`` and ``d_spectrum_flags``
        (:func:`rfi_spectrum_flags_bytes`) a spectrum's flag is 1 where its zero-DM sum is an outlier of the beam's window.
        ``d_counts`` (:func:`rfi_counts_bytes`) gets ``{cells flagged, channels masked, spectra flagged}`` per beam."""
        t = thresholds
        thr = _RfiThresholds(float(t.mean_thr), float(t.mean_floor), float(t.var_thr), float(t.var_floor), float(t.zero_dm_thr),
                             float(t.zero_dm_floor), int(t.max_bad_blocks))
        rl = _lib.companion("rfi")
        check(rl.dcs_bf_rfi_flags(c_void_p(self._h), _p(d_cell_sums), int(cell_sums_bytes), _p_or_null(d_zero_dm),
                                  int(zero_dm_bytes), int(nr_blocks), int(block_len), int(nr_beams),
                                  ctypes.cast(ctypes.pointer(thr), c_void_p), _p(d_cell_flags), int(cell_flags_bytes),
                                  _p(d_channel_mask), int(channel_mask_bytes), _p_or_null(d_spectrum_flags),
                                  int(spectrum_flags_bytes), _p(d_counts), int(counts_bytes), _s(stream)),
              "dcs_bf_rfi_flags")

    def rfi_clean_q8(self, d_filterbank, filterbank_bytes: int, in_spectra: int, first_spectrum: int, nr_blocks: int,
                     block_len: int, nr_beams: int, fill: int, d_out, out_bytes: int, out_spectra: int, first_out: int = 0,
                     d_cell_flags=None, d_channel_mask=None, d_spectrum_flags=None, d_replaced=None, stream=None) -> None:
        """The window into rows ``first_out ..`` of ``d_out`` (``uint8 [nr_beams][out_spectra][C]``; may be the filterbank
        itself at the same rows) with ``fill`` for every byte whose channel's mask byte is 0, whose cell's flag is not 0 or
        whose spectrum's flag is not 0 (each ``None``: none); ``d_replaced``: ``None``, or a zeroed device
        ``uint64 [nr_beams]`` array that grows by the bytes replaced."""
        if not 0 <= int(fill) <= 255:
            raise ValueError("fill is a byte")
        rl = _lib.companion("rfi")
        check(rl.dcs_bf_rfi_clean_q8(c_void_p(self._h), _p(d_filterbank), int(filterbank_bytes), int(in_spectra),
                                     int(first_spectrum), int(nr_blocks), int(block_len), int(nr_beams), _p_or_null(d_cell_flags),
                                     _p_or_null(d_channel_mask), _p_or_null(d_spectrum_flags), int(fill), _p(d_out),
                                     int(out_bytes), int(out_spectra), int(first_out), _p_or_null(d_replaced), _s(stream)),
              "dcs_bf_rfi_clean_q8")

    # -- the pulsar folder on the same filterbanks (include/dcs_fold.h, companion library libdcs_fold.so): d_models a device
    #    dcs_bf_fold_model [nr_beams // beams_per_model][nr_subints] array (dc_sand_amd.fold.fold_models makes a row)
    def fold_q8(self, d_filterbank, filterbank_bytes: int, in_spectra: int, first_spectrum: int, subint_len: int, nr_subints: int,
                nr_beams: int, d_models, models_bytes: int, nbin: int, d_profiles, profiles_bytes: int, out_subints: int,
                first_subint: int = 0, beams_per_model: int = 1, d_delays=None, delays_bytes: int = 0, max_delay: int = 0,
                d_channel_mask=None, d_hits=None, hits_bytes: int = 0, accumulate: bool = False, stream=None) -> None:
        """Per beam ``b`` and sub-integration ``s < nr_subints``: word ``[b][first_subint + s][c][j]`` of the profiles
        (:func:`fold_profiles_bytes`) becomes (``accumulate``: grows by) the exact sum of the filterbank bytes
        ``[first_spectrum + s * subint_len + k + d_delays[p][c]][c]`` over the ``k < subint_len`` whose phase under model
        ``[p][s]``, ``p = b // beams_per_model``, falls into bin ``j`` of ``nbin``; ``d_hits`` (``None``, or
        :func:`fold_hits_bytes`) counts those ``k``.  ``d_delays``: ``None``, or a device ``int32 [P][C]`` array as
        :meth:`dm_delays` makes it; entries outside ``[0, max_delay]`` and the columns whose byte of ``d_channel_mask``
        (``None``, or ``uint8 [C]``) is zero fold to zero."""
        fl = _lib.companion("fold")
        check(fl.dcs_bf_fold_q8(c_void_p(self._h), _p(d_filterbank), int(filterbank_bytes), int(in_spectra), int(first_spectrum),
                                int(subint_len), int(nr_subints), int(nr_beams), int(beams_per_model), _p(d_models),
                                int(models_bytes), _p_or_null(d_delays), int(delays_bytes), int(max_delay),
                                _p_or_null(d_channel_mask), int(nbin), _p(d_profiles), int(profiles_bytes), _p_or_null(d_hits),
                                int(hits_bytes), int(out_subints), int(first_subint), int(bool(accumulate)), _s(stream)),
              "dcs_bf_fold_q8")

    def fold_scrunch(self, d_profiles, profiles_bytes: int, nr_beams: int, out_subints: int, first_subint: int, nr_subints: int,
                     nbin: int, d_scrunched, scrunched_bytes: int, accumulate: bool = False, stream=None) -> None:
        """Sub-integrations ``first_subint .. first_subint + nr_subints - 1`` of the profiles summed over the channels into
        the same sub-integrations of ``d_scrunched`` (:func:`fold_scrunched_bytes`), exactly, in 64 bits; ``accumulate`` adds."""
        fl = _lib.companion("fold")
        check(fl.dcs_bf_fold_scrunch(c_void_p(self._h), _p(d_profiles), int(profiles_bytes), int(nr_beams), int(out_subints),
                                     int(first_subint), int(nr_subints), int(nbin), _p(d_scrunched), int(scrunched_bytes),
                                     int(bool(accumulate)), _s(stream)),
              "dcs_bf_fold_scrunch")

    # -- the single-pulse search on those planes (include/dcs_single_pulse.h, companion library libdcs_single_pulse.so):
    #    d_widths a device uint32 [nr_widths] array of boxcar widths, d_peaks a device uint32
    #    [nr_beams][nr_dm][nr_widths][peak_blocks][2] array of {value, time}
    def dm_time_sums(self, d_dm_time, dm_time_bytes: int, plane_spectra: int, first_spectrum: int, nr_spectra: int, nr_beams: int,
                     nr_dm: int, d_sums, sums_bytes: int, accumulate: bool = False, stream=None) -> None:
        """Per (beam, DM) series the exact ``{sum x, sum x^2 mod 2^64}`` over the words ``first_spectrum ..
        first_spectrum + nr_spectra - 1`` into ``d_sums`` (:func:`dm_time_sums_bytes`); with ``accumulate`` they are added
        to what ``d_sums`` holds."""
        sl = _lib.companion("single_pulse")
        check(sl.dcs_bf_dm_time_sums(c_void_p(self._h), _p(d_dm_time), int(dm_time_bytes), int(plane_spectra), int(first_spectrum),
                                     int(nr_spectra), int(nr_beams), int(nr_dm), 1 if accumulate else 0, _p(d_sums),
                                     int(sums_bytes), _s(stream)),
              "dcs_bf_dm_time_sums")

    def boxcar_peaks(self, d_dm_time, dm_time_bytes: int, plane_spectra: int, first_spectrum: int, nr_spectra: int, nr_beams: int,
                     nr_dm: int, d_widths, nr_widths: int, max_width: int, block_len: int, d_peaks, peaks_bytes: int,
                     peak_blocks: int, first_block: int = 0, stream=None) -> None:
        """Per series, width ``w = d_widths[i]`` and block of ``block_len`` times ``t < nr_spectra``: the largest sum of
        ``w`` consecutive words from ``first_spectrum + t`` (mod 2^32) and the smallest ``t`` that attains it, into block
        ``first_block + k`` of ``d_peaks`` (:func:`boxcar_peaks_bytes`); a width outside ``[1, max_width]`` gives
        ``{0, 0xFFFFFFFF}``.  Words up to ``first_spectrum + nr_spectra + max_width - 2`` of a series are read."""
        sl = _lib.companion("single_pulse")
        check(sl.dcs_bf_boxcar_peaks(c_void_p(self._h), _p(d_dm_time), int(dm_time_bytes), int(plane_spectra), int(first_spectrum),
                                     int(nr_spectra), int(nr_beams), int(nr_dm), _p(d_widths), int(nr_widths), int(max_width),
                                     int(block_len), _p(d_peaks), int(peaks_bytes), int(peak_blocks), int(first_block),
                                     _s(stream)),
              "dcs_bf_boxcar_peaks")

    def peak_snr(self, d_peaks, peaks_bytes: int, peak_blocks: int, first_block: int, nr_blocks: int, nr_beams: int, nr_dm: int,
                 d_widths, nr_widths: int, max_width: int, d_sums, sums_bytes: int, count: int, d_snr, snr_bytes: int,
                 d_best=None, best_bytes: int = 0, stream=None) -> None:
        """The peaks of blocks ``first_block .. first_block + nr_blocks - 1`` as signal-to-noise
        ``(value - w * mean) / sqrt(w * variance)`` with the mean and variance of the ``count`` words behind ``d_sums``, in
        fp64 rounded once per operation, into ``d_snr`` (:func:`peak_snr_bytes`): 0 for a series without variance,
        ``-inf`` for a width outside ``[1, max_width]``.  ``d_best``: ``None``, or a device ``uint32`` array
        (:func:`best_width_bytes`) for the lowest width index with the largest signal-to-noise of every block."""
        sl = _lib.companion("single_pulse")
        check(sl.dcs_bf_peak_snr(c_void_p(self._h), _p(d_peaks), int(peaks_bytes), int(peak_blocks), int(first_block),
                                 int(nr_blocks), int(nr_beams), int(nr_dm), _p(d_widths), int(nr_widths), int(max_width),
                                 _p(d_sums), int(sums_bytes), int(count), _p(d_snr), int(snr_bytes), _p_or_null(d_best),
                                 int(best_bytes), _s(stream)),
              "dcs_bf_peak_snr")

    # -- the candidate sifter on that signal-to-noise (include/dcs_candidates.h, companion library libdcs_candidates.so):
    #    d_cands a device array of candidate_dtype records, d_count a device uint32 [2] array {found, written}
    def find_candidates(self, d_snr, snr_bytes: int, d_peaks, peaks_bytes: int, peak_blocks: int, first_block: int, nr_blocks: int,
                        nr_beams: int, nr_dm: int, nr_widths: int, threshold: float, dm_radius: int, block_radius: int, d_cands,
                        cands_bytes: int, max_candidates: int, d_count, d_work, work_bytes: int, stream=None) -> None:
        """The cells (beam, DM, block) of blocks ``first_block .. first_block + nr_blocks - 1`` whose largest
        signal-to-noise over the widths is at or above ``threshold`` and which no cell of the same beam within
        ``dm_radius`` DMs and ``block_radius`` blocks (0 .. 8 each) beats -- the larger value, or of equal values the
        earlier (DM, block) -- as :data:`candidate_dtype` records in ascending (beam, DM, block): the first
        ``min(found, max_candidates)`` of ``d_cands`` (:func:`candidates_bytes`; ``None`` where ``max_candidates`` is 0)
        and ``d_count = {found, written}``.  ``d_work``: :func:`candidates_workspace_bytes` bytes of scratch."""
        cl = _lib.companion("candidates")
        check(cl.dcs_bf_find_candidates(c_void_p(self._h), _p(d_snr), int(snr_bytes), _p(d_peaks), int(peaks_bytes),
                                        int(peak_blocks), int(first_block), int(nr_blocks), int(nr_beams), int(nr_dm),
                                        int(nr_widths), float(np.float32(threshold)), int(dm_radius), int(block_radius),
                                        _p_or_null(d_cands), int(cands_bytes), int(max_candidates), _p(d_count), _p(d_work),
                                        int(work_bytes), _s(stream)),
              "dcs_bf_find_candidates")

    # -- the correlator (include/dcs_correlator.h, companion library libdcs_correlator.so): d_vis is a device int32
    #    [C][(nt / 16) / blocks_per_vis][NB][2] array, d_out a device float [nr_vis / vis_per_integration][C][NB][2] array
    def correlate_block(self, d_antenna, antenna_bytes: int, d_vis, vis_bytes: int, nt: int, blocks_per_vis: int,
                        stream=None) -> None:
        """The visibilities ``sum_t x_a[t] conj(x_b[t])`` of every antenna pair ``b <= a`` (:func:`nr_baselines`) over every
        ``blocks_per_vis`` (1 .. 4095) blocks of 16 samples, as exact integers ``{re, im}``
        (:func:`block_visibilities_bytes`).  No delay table is needed."""
        cl = _lib.companion("correlator")
        check(cl.dcs_bf_correlate_block(c_void_p(self._h), int(nt), _p(d_antenna), int(antenna_bytes), int(blocks_per_vis),
                                        _p(d_vis), int(vis_bytes), _s(stream)),
              "dcs_bf_correlate_block")

    def integrate_visibilities(self, d_vis, vis_bytes: int, nr_vis: int, vis_per_integration: int, d_out, out_bytes: int,
                               accumulate: bool = False, stream=None) -> None:
        """Sums the visibilities ``[C][nr_vis][NB][2]`` ``vis_per_integration`` at a time, exactly, into
        ``[nr_vis / vis_per_integration][C][NB][2]`` (:func:`visibilities_bytes`), each sum rounded to float once; with
        ``accumulate`` it is added to what ``d_out`` holds, so an integration can span calls."""
        cl = _lib.companion("correlator")
        check(cl.dcs_bf_integrate_visibilities(c_void_p(self._h), _p(d_vis), int(vis_bytes), int(nr_vis),
                                               int(vis_per_integration), 1 if accumulate else 0, _p(d_out), int(out_bytes),
                                               _s(stream)),
              "dcs_bf_integrate_visibilities")

    # -- the narrowband digital down-converter (include/dcs_ddc.h, companion library libdcs_ddc.so): d_samples is a device int8
    #    [nr_inputs][in_stride] array, d_out a device float [band][input][out_stride][2] array
    def ddc_tap_digits(self, d_taps, nr_taps: int, nr_bands: int, d_digits, digits_bytes: int, stream=None) -> None:
        """The integer taps ``int32 [band][nr_taps][{re, im}]`` (correlation order; :func:`dc_sand_amd.ddc.band_taps`) as the
        operand table of :meth:`ddc` (:func:`ddc_digits_bytes`): three balanced base-256 digits per tap, exact for
        ``|tap| <= 8 355 711``."""
        cl = _lib.companion("ddc")
        check(cl.dcs_bf_ddc_tap_digits(c_void_p(self._h), _p(d_taps), int(nr_taps), int(nr_bands), _p(d_digits), int(digits_bytes),
                                       _s(stream)),
              "dcs_bf_ddc_tap_digits")

    def ddc(self, d_samples, samples_bytes: int, in_stride: int, nr_inputs: int, nr_out: int, d_digits, digits_bytes: int,
            nr_taps: int, bands, d_out, out_bytes: int, out_stride: int, first_output: int = 0, stream=None) -> None:
        """``nr_out`` outputs per input row: output ``m`` is the exact integer sum of the taps with samples ``16 m .. 16 m +
        nr_taps - 1``, rotated by the band's oscillator at output ``first_output + m`` and scaled by its gain.  ``bands`` is a
        sequence of one or two ``(phase_step, phase0, gain)`` (:func:`dc_sand_amd.ddc.phase_step`), read now."""
        cl = _lib.companion("ddc")
        arr = (_DdcBand * len(bands))(*[_DdcBand(int(ps) & 0xFFFFFFFF, int(p0) & 0xFFFFFFFF, float(g)) for ps, p0, g in bands])
        check(cl.dcs_bf_ddc(c_void_p(self._h), int(nr_inputs), int(nr_out), _p(d_samples), int(samples_bytes), int(in_stride),
                            _p(d_digits), int(digits_bytes), int(nr_taps), len(bands), ctypes.cast(arr, c_void_p),
                            int(first_output), _p(d_out), int(out_bytes), int(out_stride), _s(stream)),
              "dcs_bf_ddc")

    # -- the polyphase channeliser behind it (include/dcs_channeliser.h, companion library libdcs_channeliser.so): d_in is a
    #    device float [nr_inputs][in_stride][2] array (one band of ddc's output), d_out a device [nr_channels][out_blocks]
    #    [out_inputs][16][2] array of floats, d_out_q8 the same of int8: the sample tensor
    def channelise(self, d_in, in_bytes: int, in_stride: int, nr_inputs: int, nr_spectra: int, nr_channels: int, nr_taps: int,
                   d_taps, d_twiddles, d_out, out_bytes: int, out_blocks: int, out_inputs: int, first_block: int = 0,
                   first_input: int = 0, order: int = 0, stream=None) -> None:
        """``nr_spectra`` (a multiple of 16) spectra per input row: spectrum ``n`` is the FIR of the ``nr_taps`` rows of
        ``nr_channels`` pairs from pair ``n nr_channels`` on with ``d_taps`` (:func:`dc_sand_amd.channeliser.pfb_taps`) through
        the butterfly network of ``d_twiddles`` (:func:`dc_sand_amd.channeliser.twiddles`), written as floats to blocks
        ``first_block ..`` and inputs ``first_input ..`` of ``d_out`` (:func:`channelised_bytes`).  ``order`` 1 gives channels
        that ascend in frequency (:func:`dc_sand_amd.channeliser.channel_of`)."""
        cl = _lib.companion("channeliser")
        check(cl.dcs_bf_channelise(c_void_p(self._h), int(nr_channels), int(nr_taps), int(nr_inputs), int(nr_spectra), _p_or_null(d_in),
                                   int(in_bytes), int(in_stride), _p_or_null(d_taps), _p_or_null(d_twiddles), int(order),
                                   _p_or_null(d_out), int(out_bytes), int(out_blocks), int(first_block), int(out_inputs),
                                   int(first_input), _s(stream)),
              "dcs_bf_channelise")

    def channelise_q8(self, d_in, in_bytes: int, in_stride: int, nr_inputs: int, nr_spectra: int, nr_channels: int, nr_taps: int,
                      d_taps, d_twiddles, d_gains, d_out_q8, out_bytes: int, out_blocks: int, out_inputs: int,
                      first_block: int = 0, first_input: int = 0, order: int = 0, d_clip_count=None, stream=None) -> None:
        """:meth:`channelise` quantised to int8 with the gains ``float [nr_inputs][nr_channels]`` (by input of the call and output
        channel), by the quantiser of :meth:`beamform_accumulated_q8`: exactly the float call's values times the gain, rounded
        to nearest even and clamped to +-127, NaN as -128.  ``d_clip_count``: ``None``, or a device ``uint64 [nr_inputs]`` array
        that grows by each input's clipped components."""
        cl = _lib.companion("channeliser")
        check(cl.dcs_bf_channelise_q8(c_void_p(self._h), int(nr_channels), int(nr_taps), int(nr_inputs), int(nr_spectra),
                                      _p_or_null(d_in), int(in_bytes), int(in_stride), _p_or_null(d_taps), _p_or_null(d_twiddles),
                                      int(order), _p_or_null(d_gains), _p_or_null(d_out_q8), int(out_bytes), int(out_blocks),
                                      int(first_block), int(out_inputs), int(first_input), _p_or_null(d_clip_count), _s(stream)),
              "dcs_bf_channelise_q8")

    TUNING_FIELDS = ("form", "nontemporal", "chan_per_block", "tiles_per_block", "waves_per_block", "rows_per_wave",
                     "xcd_remap", "rows_same_tile", "math_mode", "wg_per_cu")
    _TUNING_DEFAULTS = (0, -1, 0, 0, 0, 0, -1, -1, 0, 0)

    def set_tuning(self, form: int = 0, nontemporal: int = -1, chan_per_block: int = 0, tiles_per_block: int = 0,
                   waves_per_block: int = 0, rows_per_wave: int = 0, xcd_remap: int = -1, rows_same_tile: int = -1,
                   math_mode: int = 0, wg_per_cu: int = 0) -> None:
        """``struct dcs_bf_tuning`` (ABI 3: ten ``int32_t``); ``set_tuning()`` restores the defaults.  The measurement
        knobs of ABI 2 (``probe_nomath`` / ``probe_pace``) are ``probes.dcs_probes.set_knobs`` of the probes build now."""
        vals = (form, nontemporal, chan_per_block, tiles_per_block, waves_per_block, rows_per_wave,
                xcd_remap, rows_same_tile, math_mode, wg_per_cu)
        if vals == self._TUNING_DEFAULTS:  # all defaults: NULL, which also forgets dcs_bf_autotune's result
            check(_lib.lib().dcs_bf_set_tuning(c_void_p(self._h), c_void_p(None)), "dcs_bf_set_tuning")
            return
        t = (ctypes.c_int32 * len(self.TUNING_FIELDS))(*vals)
        check(_lib.lib().dcs_bf_set_tuning(c_void_p(self._h), ctypes.cast(t, c_void_p)), "dcs_bf_set_tuning")

    def autotune(self, d_out, out_bytes: int, bitwidth: int = B32, stream=None) -> dict:
        """``dcs_bf_autotune``: time the tiled form's geometries on this device for this
        shape, keep the fastest for this context, return the chosen knobs."""
        t = (ctypes.c_int32 * len(self.TUNING_FIELDS))()
        check(
            _lib.lib().dcs_bf_autotune(c_void_p(self._h), int(bitwidth), c_void_p(int(d_out)), int(out_bytes), _s(stream),
                                       ctypes.cast(t, c_void_p)),
            "dcs_bf_autotune",
        )
        return dict(zip(self.TUNING_FIELDS, (int(v) for v in t)))

    def output_bytes(self, bitwidth: int = B32, nt: int = 1) -> int:
        return output_bytes(self.params, bitwidth, nt)

    # -- streaming (config 5) ---------------------------------------------
    def stream_begin(self, d_out, out_bytes: int, c0: int, nc: int, stream, bitwidth: int = B32) -> "CoefficientStream":
        h = c_void_p()
        check(
            _lib.lib().dcs_bf_stream_begin(c_void_p(self._h), int(bitwidth), int(c0), int(nc), c_void_p(int(d_out)), int(out_bytes),
                                           _s(stream), byref(h)),
            "dcs_bf_stream_begin",
        )
        return CoefficientStream(self, h.value)

    def close(self) -> None:
        if self._h:
            _lib.lib().dcs_bf_destroy(c_void_p(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CoefficientStream:
    """hipGraph replay of one time step per tick (BASELINE config 5)."""

    def __init__(self, gen: SteeringCoefficientGenerator, handle: int):
        self._gen = gen
        self._h = handle
        self._pinned_staged = None

    def tick(self, t: int, new_table: np.ndarray | None = None) -> None:
        ptr = c_void_p(None)
        if new_table is not None:
            new_table = np.ascontiguousarray(new_table)
            if new_table.dtype != delay_vals_dtype or new_table.size != self._gen.params.n_pairs:
                raise ValueError("bad delay table")
            ptr = c_void_p(new_table.ctypes.data)
        check(_lib.lib().dcs_bf_stream_tick(c_void_p(self._h), int(t), ptr), "dcs_bf_stream_tick")

    def _table_ptr(self, new_table):
        if new_table is None:
            return c_void_p(None), None
        new_table = np.ascontiguousarray(new_table)
        if new_table.dtype != delay_vals_dtype or new_table.size != self._gen.params.n_pairs:
            raise ValueError("bad delay table")
        return c_void_p(new_table.ctypes.data), new_table

    def tick_dt(self, dt: float, new_table: np.ndarray | None = None) -> None:
        """A tick at model time ``dt`` seconds after the reference time (``dcs_bf_stream_tick_dt``)."""
        ptr, keep = self._table_ptr(new_table)
        check(_lib.lib().dcs_bf_stream_tick_dt(c_void_p(self._h), float(np.float32(dt)), ptr), "dcs_bf_stream_tick_dt")

    def tick_at(self, current_time, reference_time, new_table: np.ndarray | None = None) -> None:
        ptr, keep = self._table_ptr(new_table)
        cur = _lib.Timespec(int(current_time[0]), int(current_time[1]))
        ref = _lib.Timespec(int(reference_time[0]), int(reference_time[1]))
        check(_lib.lib().dcs_bf_stream_tick_at(c_void_p(self._h), byref(cur), byref(ref), ptr), "dcs_bf_stream_tick_at")

    # -- the same ticks with the new table already on the device (a global [NR_STATIONS][nr_beams_total] table, e.g.
    #    just broadcast by RCCL; this context owns beams [beam_offset, beam_offset + NR_BEAMS)): gathered by a node of
    #    the replayed graph, no host staging (``dcs_bf_stream_tick_*_from_global``)
    def _global_args(self, d_global_table, nr_beams_total, beam_offset):
        nb = self._gen.params.NR_BEAMS if nr_beams_total is None else nr_beams_total
        return c_void_p(int(d_global_table)), int(nb), int(beam_offset)

    def tick_from_global(self, t: int, d_global_table, nr_beams_total: int | None = None, beam_offset: int = 0) -> None:
        check(_lib.lib().dcs_bf_stream_tick_from_global(c_void_p(self._h), int(t), *self._global_args(d_global_table, nr_beams_total, beam_offset)),
              "dcs_bf_stream_tick_from_global")

    def tick_dt_from_global(self, dt: float, d_global_table, nr_beams_total: int | None = None, beam_offset: int = 0) -> None:
        check(_lib.lib().dcs_bf_stream_tick_dt_from_global(c_void_p(self._h), float(np.float32(dt)),
                                                           *self._global_args(d_global_table, nr_beams_total, beam_offset)),
              "dcs_bf_stream_tick_dt_from_global")

    def tick_at_from_global(self, current_time, reference_time, d_global_table, nr_beams_total: int | None = None,
                            beam_offset: int = 0) -> None:
        cur = _lib.Timespec(int(current_time[0]), int(current_time[1]))
        ref = _lib.Timespec(int(reference_time[0]), int(reference_time[1]))
        check(_lib.lib().dcs_bf_stream_tick_at_from_global(c_void_p(self._h), byref(cur), byref(ref),
                                                           *self._global_args(d_global_table, nr_beams_total, beam_offset)),
              "dcs_bf_stream_tick_at_from_global")

    # -- staged tables: the NEXT tick's table lands while the current tick runs (``dcs_bf_stream_stage_table*``); the
    #    next tick without a table of its own makes it current
    def stage_table(self, table: np.ndarray, pinned: bool = False) -> None:
        """Stage ``table`` for the next tick that brings no table.  ``pinned=False``: copied through the stream's pinned
        ring, ``table`` is free again on return.  ``pinned=True``: ``table`` is a :func:`device.pagelocked_empty` array,
        copied from where it is; keep it unchanged until the consuming tick has run on the stream."""
        if pinned:
            if not isinstance(table, np.ndarray) or not table.flags["C_CONTIGUOUS"]:
                raise ValueError("pinned=True needs a C-contiguous pagelocked_empty array")
        else:
            table = np.ascontiguousarray(table)
        if table.dtype != delay_vals_dtype or table.size != self._gen.params.n_pairs:
            raise ValueError("bad delay table")
        check(_lib.companion("stream_staging").dcs_bf_stream_stage_table(c_void_p(self._h), _p(table.ctypes.data),
                                                                         _lib.DCS_BF_STAGE_CALLER_PINNED if pinned else 0),
              "dcs_bf_stream_stage_table")
        if pinned:
            self._pinned_staged = table  # the copy reads it asynchronously: keep the allocation alive

    def stage_table_from_global(self, d_global_table, nr_beams_total: int | None = None, beam_offset: int = 0,
                                ready_event=None) -> None:
        """Stage this context's beam slice of a device-resident global table; the gather waits (on the device) for
        ``ready_event`` -- a :class:`device.Event` or a raw ``hipEvent_t`` the producer recorded -- when given."""
        ev = ready_event.handle if hasattr(ready_event, "handle") else ready_event
        check(_lib.companion("stream_staging").dcs_bf_stream_stage_table_from_global(
                  c_void_p(self._h), *self._global_args(d_global_table, nr_beams_total, beam_offset), _p_or_null(ev)),
              "dcs_bf_stream_stage_table_from_global")

    def end(self) -> None:
        if self._h:
            _lib.lib().dcs_bf_stream_end(c_void_p(self._h))
            self._h = None
        self._pinned_staged = None

    def __del__(self):
        try:
            self.end()
        except Exception:
            pass
