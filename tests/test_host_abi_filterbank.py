"""The companion library of the 8-bit search filterbanks (include/dcs_filterbank.h, libdcs_filterbank.so): it exports
exactly what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the
Python binding has the header's argument types, the argument checks that need no device, the header from C, and the size
helpers.  No GPU needed."""
import ctypes
from ctypes import c_float, c_size_t, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

SUMS = "dcs_bf_spectra_sums"
SCALES = "dcs_bf_filterbank_scales"
Q8 = "dcs_bf_filterbank_q8"
FILTERBANK = {
    SUMS: [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
    SCALES: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint32, c_float, c_void_p, c_size_t, c_void_p],
    Q8: [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_uint64, c_uint64,
         c_void_p, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("filterbank", FILTERBANK)
    check_header_parameter_kinds("filterbank", FILTERBANK)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(FILTERBANK, "filterbank")
    check_product_inventory(FILTERBANK, "spectra_sums")
    assert dcs_lib.dcs_abi_version() == 3


def _sums(flib, ctx, spectra, sums, nr_spectra=4, nr_beams=2, accumulate=0):
    return getattr(flib, SUMS)(ctx, spectra, 0, nr_spectra, nr_beams, accumulate, sums, 0, None)


def _scales(flib, ctx, sums, scales, count=4, nr_beams=2):
    return getattr(flib, SCALES)(ctx, sums, 0, count, nr_beams, 24.0, scales, 0, None)


def _q8(flib, ctx, spectra, scales, out, nr_spectra=4, nr_beams=2, flags=0, out_spectra=4, first=0, clips=None):
    return getattr(flib, Q8)(ctx, spectra, 0, nr_spectra, nr_beams, scales, 128.0, flags, out, 0, out_spectra, first, clips, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    flib = _lib.companion("filterbank")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.cast(buf, c_void_p).value
    p = c_void_p((base + 15) & ~15)  # 16-byte aligned
    off = lambda n: c_void_p(p.value + n)  # noqa: E731
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        # the sums: NULL context, input, output; spectra not 4-byte, sums not 8-byte aligned; no beams
        assert _sums(flib, None, p, p) == INVALID
        assert _sums(flib, fp, None, p) == INVALID
        assert _sums(flib, fp, p, None) == INVALID
        assert _sums(flib, fp, off(2), p) == INVALID
        assert _sums(flib, fp, off(1), p) == INVALID
        assert _sums(flib, fp, p, off(4)) == INVALID
        assert _sums(flib, fp, p, p, nr_beams=0) == INVALID
        # arguments that pass every check made without a device: the fake object is refused without being used
        for acc in (0, 1):
            assert _sums(flib, fp, off(4), off(8), accumulate=acc) == UNSUPPORTED  # the stated alignments are enough
            assert _sums(flib, fp, p, p, nr_spectra=0, accumulate=acc) == UNSUPPORTED
        # the scales: NULL context, input, output; either not 8-byte aligned; no beams; count 0 or >= 2^53
        assert _scales(flib, None, p, p) == INVALID
        assert _scales(flib, fp, None, p) == INVALID
        assert _scales(flib, fp, p, None) == INVALID
        assert _scales(flib, fp, off(4), p) == INVALID
        assert _scales(flib, fp, p, off(4)) == INVALID
        assert _scales(flib, fp, p, p, nr_beams=0) == INVALID
        for count in (0, 1 << 53, (1 << 53) + 1, (1 << 64) - 1):
            assert _scales(flib, fp, p, p, count=count) == INVALID, count
        for count in (1, (1 << 53) - 1):
            assert _scales(flib, fp, off(8), off(8), count=count) == UNSUPPORTED, count
        # the quantiser: NULL context, input, scales, output; alignments 4, 8, 16 and 8; no beams; unknown flags; rows that
        # do not fit
        assert _q8(flib, None, p, p, p) == INVALID
        assert _q8(flib, fp, None, p, p) == INVALID
        assert _q8(flib, fp, p, None, p) == INVALID
        assert _q8(flib, fp, p, p, None) == INVALID
        assert _q8(flib, fp, off(2), p, p) == INVALID
        assert _q8(flib, fp, p, off(4), p) == INVALID
        assert _q8(flib, fp, p, p, off(8)) == INVALID
        assert _q8(flib, fp, p, p, off(1)) == INVALID
        assert _q8(flib, fp, p, p, p, clips=off(4)) == INVALID
        assert _q8(flib, fp, p, p, p, nr_beams=0) == INVALID
        for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFF):
            assert _q8(flib, fp, p, p, p, flags=flags) == INVALID, flags
        for nr, out, first in ((4, 3, 0), (4, 4, 1), (1, 0, 0), (0, 4, 5), (4, 7, 4), (1, (1 << 64) - 1, (1 << 64) - 1),
                               (2, 5, (1 << 64) - 1)):
            assert _q8(flib, fp, p, p, p, nr_spectra=nr, out_spectra=out, first=first) == INVALID, (nr, out, first)
        for flags in (0, 1):
            assert _q8(flib, fp, off(4), off(8), off(16), flags=flags, clips=off(8)) == UNSUPPORTED
            assert _q8(flib, fp, p, p, p, flags=flags) == UNSUPPORTED  # no counters
        assert _q8(flib, fp, p, p, p, nr_spectra=4, out_spectra=9, first=5) == UNSUPPORTED
        assert _q8(flib, fp, p, p, p, nr_spectra=0, out_spectra=4, first=4) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, the detector's and the incoherent beam's
    # (never this build's own version: the zeroed table would be called)
    for version in (1, 3, 5):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "filterbank",
        '#include <stdio.h>\n#include "dcs_filterbank.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, const float *, size_t, uint32_t, uint32_t, uint32_t, double *, size_t, void *) =\n"
        "      dcs_bf_spectra_sums;\n"
        "  int (*g)(dcs_bf_context *, const double *, size_t, uint64_t, uint32_t, float, float *, size_t, void *) =\n"
        "      dcs_bf_filterbank_scales;\n"
        "  int (*h)(dcs_bf_context *, const float *, size_t, uint32_t, uint32_t, const float *, float, uint32_t, uint8_t *,\n"
        "           size_t, uint64_t, uint64_t, unsigned long long *, void *) = dcs_bf_filterbank_q8;\n"
        '  printf("%d %d %d %u %d\\n", f != 0, g != 0, h != 0, DCS_FB_DESCENDING, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "1", "1", "3"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import filterbank_bytes, filterbank_scales_bytes, spectra_sums_bytes

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert spectra_sums_bytes(bp, 3) == 5 * 3 * 2 * 8 and spectra_sums_bytes(bp, 1) == 5 * 2 * 8
    assert filterbank_scales_bytes(bp, 3) == 5 * 3 * 2 * 4 and filterbank_scales_bytes(bp, 1) == 5 * 2 * 4
    assert filterbank_bytes(bp, 3, 7) == 3 * 7 * 5 and filterbank_bytes(bp, 1, 2) == 2 * 5
