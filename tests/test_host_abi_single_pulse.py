"""The companion library of the single-pulse search (include/dcs_single_pulse.h, libdcs_single_pulse.so): it exports exactly
what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python
binding has the header's argument types, the argument checks that need no device in their order, the header from C, and
the size helpers.  No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

SUMS = "dcs_bf_dm_time_sums"
PEAKS = "dcs_bf_boxcar_peaks"
SNR = "dcs_bf_peak_snr"
SINGLE_PULSE = {
    SUMS: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
    PEAKS: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32,
            c_void_p, c_size_t, c_uint64, c_uint64, c_void_p],
    SNR: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p,
          c_size_t, c_uint64, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("single_pulse", SINGLE_PULSE)
    check_header_parameter_kinds("single_pulse", SINGLE_PULSE)


def test_product_library_keeps_its_52_functions(dcs_lib):
    for part in ("dm_time_sums", "boxcar", "peak_snr"):
        check_product_inventory(SINGLE_PULSE, part)
    assert dcs_lib.dcs_abi_version() == 3


def _sums(slib, ctx, plane, out, plane_spectra=100, first=10, T=90, B=1, nr_dm=3, accumulate=0):
    return getattr(slib, SUMS)(ctx, plane, 0, plane_spectra, first, T, B, nr_dm, accumulate, out, 0, None)


def _peaks(slib, ctx, plane, widths, out, plane_spectra=100, first=10, T=70, B=1, nr_dm=3, nr_widths=4, max_width=21, block_len=64,
           peak_blocks=5, first_block=3):
    return getattr(slib, PEAKS)(ctx, plane, 0, plane_spectra, first, T, B, nr_dm, widths, nr_widths, max_width, block_len, out, 0,
                                peak_blocks, first_block, None)


def _snr(slib, ctx, peaks, widths, sums, out, best=None, peak_blocks=5, first_block=3, nr_blocks=2, B=1, nr_dm=3, nr_widths=4,
         max_width=21, count=90):
    return getattr(slib, SNR)(ctx, peaks, 0, peak_blocks, first_block, nr_blocks, B, nr_dm, widths, nr_widths, max_width, sums, 0,
                              count, out, 0, best, 0, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    slib = _lib.companion("single_pulse")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r, s, u = (c_void_p(base + 16 * i) for i in range(5))
    odd1, odd2, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 2), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        # -- dm_time_sums: NULLs, alignment, then the values
        assert _sums(slib, None, p, q) == INVALID
        assert _sums(slib, fp, None, q) == INVALID
        assert _sums(slib, fp, p, None) == INVALID
        assert _sums(slib, fp, None, None, T=0, nr_dm=0) == INVALID  # also where there is nothing to do
        for bad in (odd1, odd2):  # the planes are dwords
            assert _sums(slib, fp, bad, q) == INVALID
        for bad in (odd1, odd2, odd4):  # the sums are 64-bit words
            assert _sums(slib, fp, p, bad) == INVALID
        assert _sums(slib, fp, p, q, B=0) == INVALID
        # first_spectrum + nr_spectra > plane_spectra, also where a 64-bit sum would wrap
        for kw in (dict(plane_spectra=99), dict(first=11), dict(T=91), dict(plane_spectra=0), dict(first=2**64 - 1),
                   dict(first=2**64 - 90), dict(plane_spectra=2**64 - 1, first=2**64 - 90)):
            assert _sums(slib, fp, p, q, **kw) == INVALID, kw
        # arguments that pass every check made without a device: the fake object is refused without being used
        assert _sums(slib, fp, p, q) == UNSUPPORTED
        assert _sums(slib, fp, odd4, odd8, accumulate=7) == UNSUPPORTED
        assert _sums(slib, fp, p, q, T=0) == UNSUPPORTED
        assert _sums(slib, fp, p, q, nr_dm=0) == UNSUPPORTED
        assert _sums(slib, fp, p, q, plane_spectra=2**64 - 1, first=2**64 - 91) == UNSUPPORTED
        assert _sums(slib, fp, p, q, plane_spectra=2**40, first=5, T=2**32 - 1) == UNSUPPORTED
        # -- boxcar_peaks: NULLs, alignment, then the ranges and the windows
        assert _peaks(slib, None, p, q, r) == INVALID
        assert _peaks(slib, fp, None, q, r) == INVALID
        assert _peaks(slib, fp, p, None, r) == INVALID
        assert _peaks(slib, fp, p, q, None) == INVALID
        assert _peaks(slib, fp, p, None, r, nr_widths=0) == INVALID  # also where there is nothing to do
        for bad in (odd1, odd2):
            assert _peaks(slib, fp, bad, q, r) == INVALID
            assert _peaks(slib, fp, p, bad, r) == INVALID
        for bad in (odd1, odd2, odd4):  # a peak is a pair of dwords
            assert _peaks(slib, fp, p, q, bad) == INVALID
        assert _peaks(slib, fp, p, q, r, B=0) == INVALID
        for max_width in (0, 4097, 2**31, 2**32 - 1):
            assert _peaks(slib, fp, p, q, r, plane_spectra=2**40, max_width=max_width) == INVALID, max_width
        for block_len in (0, 1, 32, 63, 65, 96, 100, 4095, 4097, 4160, 8192, 2**32 - 64):
            assert _peaks(slib, fp, p, q, r, plane_spectra=2**40, peak_blocks=2**40, block_len=block_len) == INVALID, block_len
        # first_spectrum + nr_spectra + max_width - 1 > plane_spectra
        for kw in (dict(plane_spectra=99), dict(first=11), dict(T=71, peak_blocks=9), dict(max_width=22), dict(plane_spectra=0),
                   dict(first=2**64 - 1), dict(first=2**64 - 90), dict(plane_spectra=2**64 - 1, first=2**64 - 90),
                   dict(T=0, first=100, max_width=2), dict(T=0, first=101, max_width=1)):
            assert _peaks(slib, fp, p, q, r, **kw) == INVALID, kw
        # first_block + nr_blocks > peak_blocks: 70 spectra are two blocks of 64
        for kw in (dict(peak_blocks=4), dict(first_block=4), dict(peak_blocks=0), dict(first_block=2**64 - 1),
                   dict(first_block=2**64 - 2), dict(peak_blocks=2**64 - 1, first_block=2**64 - 2), dict(T=0, first_block=6)):
            assert _peaks(slib, fp, p, q, r, **kw) == INVALID, kw
        # arguments that pass: exactly fitting windows, nothing to do, the largest width and block
        assert _peaks(slib, fp, p, q, r) == UNSUPPORTED
        assert _peaks(slib, fp, odd4, odd4, odd8) == UNSUPPORTED
        assert _peaks(slib, fp, p, q, r, T=64, max_width=27, first_block=4) == UNSUPPORTED
        assert _peaks(slib, fp, p, q, r, T=0, first=100, max_width=1, first_block=5) == UNSUPPORTED
        assert _peaks(slib, fp, p, q, r, nr_widths=0) == UNSUPPORTED
        assert _peaks(slib, fp, p, q, r, nr_dm=0) == UNSUPPORTED
        assert _peaks(slib, fp, p, q, r, plane_spectra=2**33, first=1, T=2**32 - 1, max_width=4096, block_len=4096,
                      peak_blocks=2**20 + 3, first_block=3) == UNSUPPORTED
        assert _peaks(slib, fp, p, q, r, plane_spectra=2**64 - 1, first=2**64 - 91, peak_blocks=2**64 - 1,
                      first_block=2**64 - 3) == UNSUPPORTED
        # -- peak_snr: NULLs, alignment, then the values
        assert _snr(slib, None, p, q, r, s) == INVALID
        assert _snr(slib, fp, None, q, r, s) == INVALID
        assert _snr(slib, fp, p, None, r, s) == INVALID
        assert _snr(slib, fp, p, q, None, s) == INVALID
        assert _snr(slib, fp, p, q, r, None) == INVALID
        assert _snr(slib, fp, p, None, r, s, nr_widths=0) == INVALID
        for bad in (odd1, odd2, odd4):
            assert _snr(slib, fp, bad, q, r, s) == INVALID
            assert _snr(slib, fp, p, q, bad, s) == INVALID
        for bad in (odd1, odd2):
            assert _snr(slib, fp, p, bad, r, s) == INVALID
            assert _snr(slib, fp, p, q, r, bad) == INVALID
            assert _snr(slib, fp, p, q, r, s, best=bad) == INVALID
        assert _snr(slib, fp, p, q, r, s, B=0) == INVALID
        for max_width in (0, 4097, 2**32 - 1):
            assert _snr(slib, fp, p, q, r, s, max_width=max_width) == INVALID, max_width
        for kw in (dict(peak_blocks=4), dict(first_block=4), dict(nr_blocks=3), dict(peak_blocks=0), dict(first_block=2**64 - 1),
                   dict(peak_blocks=2**64 - 1, first_block=2**64 - 1), dict(nr_blocks=0, first_block=6)):
            assert _snr(slib, fp, p, q, r, s, **kw) == INVALID, kw
        assert _snr(slib, fp, p, q, r, s, count=0) == INVALID
        # arguments that pass
        assert _snr(slib, fp, p, q, r, s) == UNSUPPORTED
        assert _snr(slib, fp, p, q, r, s, best=u) == UNSUPPORTED
        assert _snr(slib, fp, odd8, odd4, odd8, odd4, best=odd4) == UNSUPPORTED
        assert _snr(slib, fp, p, q, r, s, nr_blocks=0, first_block=5) == UNSUPPORTED
        assert _snr(slib, fp, p, q, r, s, nr_widths=0) == UNSUPPORTED
        assert _snr(slib, fp, p, q, r, s, nr_dm=0, count=2**64 - 1, max_width=4096) == UNSUPPORTED
        assert _snr(slib, fp, p, q, r, s, peak_blocks=2**64 - 1, first_block=2**64 - 3) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 9, 10):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "single_pulse",
        '#include <stdio.h>\n#include "dcs_single_pulse.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, const uint32_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t,\n"
        "           uint64_t *, size_t, void *) = dcs_bf_dm_time_sums;\n"
        "  int (*g)(dcs_bf_context *, const uint32_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, const uint32_t *,\n"
        "           uint32_t, uint32_t, uint32_t, uint32_t *, size_t, uint64_t, uint64_t, void *) = dcs_bf_boxcar_peaks;\n"
        "  int (*h)(dcs_bf_context *, const uint32_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, const uint32_t *,\n"
        "           uint32_t, uint32_t, const uint64_t *, size_t, uint64_t, float *, size_t, uint32_t *, size_t, void *) = dcs_bf_peak_snr;\n"
        '  printf("%d %d %d %d\\n", f != 0, g != 0, h != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "1", "3"]


def test_size_helpers():
    from dc_sand_amd.generator import (SteeringCoefficientGenerator, best_width_bytes, boxcar_peaks_bytes, dm_time_sums_bytes,
                                       peak_snr_bytes)

    assert dm_time_sums_bytes(3, 7) == 3 * 7 * 16 and dm_time_sums_bytes(3, 0) == 0
    assert boxcar_peaks_bytes(3, 7, 5, 11) == 3 * 7 * 5 * 11 * 8
    assert peak_snr_bytes(3, 7, 5, 11) == 3 * 7 * 5 * 11 * 4
    assert best_width_bytes(3, 7, 11) == 3 * 7 * 11 * 4
    assert boxcar_peaks_bytes(1, 4, 4, (1 << 26) + 5) == 16 * ((1 << 26) + 5) * 8 > 1 << 33  # past 2^33: a Python int
    for name in ("dm_time_sums", "boxcar_peaks", "peak_snr"):
        assert callable(getattr(SteeringCoefficientGenerator, name))
