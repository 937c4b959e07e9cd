"""The companion library of the dedispersion (include/dcs_dedisperse.h, libdcs_dedisperse.so): it exports exactly what its
header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding has
the header's argument types, the argument checks that need no device in their order, the header from C, and the size
helpers.  No GPU needed."""
import ctypes
from ctypes import c_double, c_size_t, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

DELAYS = "dcs_bf_dm_delays"
DEDISPERSE = "dcs_bf_dedisperse_q8"
DEDISP = {
    DELAYS: [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_size_t, c_void_p],
    DEDISPERSE: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_void_p, c_uint32, c_uint32, c_void_p,
                 c_void_p, c_size_t, c_uint64, c_uint64, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("dedisperse", DEDISP)
    check_header_parameter_kinds("dedisperse", DEDISP)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(DEDISP, "dedisperse")
    check_product_inventory(DEDISP, "dm_delays")
    assert dcs_lib.dcs_abi_version() == 3


class Band(ctypes.Structure):
    _fields_ = [("first", c_double), ("step", c_double), ("ts", c_double)]


def _delays(dlib, ctx, band, dms, nr_dm, out):
    return getattr(dlib, DELAYS)(ctx, None if band is None else ctypes.cast(ctypes.pointer(band), c_void_p), dms, nr_dm, out, 0, None)


def _dedisperse(dlib, ctx, fb, delays, out, in_spectra=100, first=10, T=20, B=1, nr_dm=3, max_delay=70, mask=None,
                out_spectra=30, first_out=10):
    return getattr(dlib, DEDISPERSE)(ctx, fb, 0, in_spectra, first, T, B, delays, nr_dm, max_delay, mask, out, 0, out_spectra,
                                     first_out, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    dlib = _lib.companion("dedisperse")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r = c_void_p(base), c_void_p(base + 16), c_void_p(base + 32)
    odd1, odd2, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 2), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED
    good = Band(1500.0, -10.0, 64e-6)
    inf, nan = float("inf"), float("nan")

    def refusals():
        # -- dm_delays: NULLs, alignment, then the band
        assert _delays(dlib, None, good, p, 4, q) == INVALID
        assert _delays(dlib, fp, None, p, 4, q) == INVALID
        assert _delays(dlib, fp, good, None, 4, q) == INVALID
        assert _delays(dlib, fp, good, p, 4, None) == INVALID
        assert _delays(dlib, fp, good, None, 0, None) == INVALID  # also where there is nothing to do
        for bad in (odd1, odd2, odd4):  # the DMs are doubles
            assert _delays(dlib, fp, good, bad, 4, q) == INVALID
        for bad in (odd1, odd2):  # the delays are dwords
            assert _delays(dlib, fp, good, p, 4, bad) == INVALID
        for first, step, ts in ((nan, -10.0, 64e-6), (inf, -10.0, 64e-6), (1500.0, nan, 64e-6), (1500.0, -inf, 64e-6),
                                (1500.0, -10.0, nan), (1500.0, -10.0, inf), (1500.0, -10.0, 0.0), (1500.0, -10.0, -64e-6),
                                (0.0, 10.0, 64e-6), (-1.0, 10.0, 64e-6)):
            assert _delays(dlib, fp, Band(first, step, ts), p, 4, q) == INVALID, (first, step, ts)
        # arguments that pass every check made without a device: the fake object is refused without being used
        assert _delays(dlib, fp, good, p, 4, q) == UNSUPPORTED
        assert _delays(dlib, fp, good, odd8, 4, odd4) == UNSUPPORTED
        assert _delays(dlib, fp, good, p, 0, q) == UNSUPPORTED
        assert _delays(dlib, fp, Band(1500.0, 0.0, 1e-3), p, 4, q) == UNSUPPORTED
        assert _delays(dlib, fp, Band(1500.0, 10.0, 1e-3), p, 4, q) == UNSUPPORTED
        # -- dedisperse_q8: NULLs, alignment, then the values
        assert _dedisperse(dlib, None, p, q, r) == INVALID
        assert _dedisperse(dlib, fp, None, q, r) == INVALID
        assert _dedisperse(dlib, fp, p, None, r) == INVALID
        assert _dedisperse(dlib, fp, p, q, None) == INVALID
        for bad in (odd1, odd2, odd4, odd8):  # the filterbanks are 16-byte aligned
            assert _dedisperse(dlib, fp, bad, q, r) == INVALID
        for bad in (odd1, odd2):
            assert _dedisperse(dlib, fp, p, bad, r) == INVALID
            assert _dedisperse(dlib, fp, p, q, bad) == INVALID
        assert _dedisperse(dlib, fp, p, q, r, B=0) == INVALID
        for max_delay in (2**31 - 1, 2**31, 2**32 - 1):
            assert _dedisperse(dlib, fp, p, q, r, in_spectra=2**40, max_delay=max_delay) == INVALID, max_delay
        # first_spectrum + nr_spectra + max_delay > in_spectra, also where a 64-bit sum would wrap
        for kw in (dict(in_spectra=99), dict(first=11), dict(T=21, out_spectra=40), dict(max_delay=71), dict(in_spectra=0),
                   dict(first=2**64 - 1), dict(first=2**64 - 90), dict(in_spectra=2**64 - 1, first=2**64 - 90)):
            assert _dedisperse(dlib, fp, p, q, r, **kw) == INVALID, kw
        # first_out + nr_spectra > out_spectra
        for kw in (dict(out_spectra=29), dict(first_out=11), dict(out_spectra=0), dict(first_out=2**64 - 1),
                   dict(first_out=2**64 - 20), dict(out_spectra=2**64 - 1, first_out=2**64 - 20)):
            assert _dedisperse(dlib, fp, p, q, r, **kw) == INVALID, kw
        # arguments that pass: exactly fitting windows, a mask of any alignment, nothing to do, the largest max_delay
        assert _dedisperse(dlib, fp, p, q, r) == UNSUPPORTED
        assert _dedisperse(dlib, fp, p, odd4, odd8, mask=odd1) == UNSUPPORTED
        assert _dedisperse(dlib, fp, p, q, r, T=0) == UNSUPPORTED
        assert _dedisperse(dlib, fp, p, q, r, nr_dm=0) == UNSUPPORTED
        assert _dedisperse(dlib, fp, p, q, r, in_spectra=2**31 + 100, first=2, T=100, max_delay=2**31 - 2, out_spectra=110) == UNSUPPORTED
        assert _dedisperse(dlib, fp, p, q, r, in_spectra=2**64 - 1, first=2**64 - 91, out_spectra=2**64 - 1, first_out=2**64 - 21) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 8, 9):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "dedisperse",
        '#include <stdio.h>\n#include "dcs_dedisperse.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, const dcs_bf_band *, const double *, uint32_t, int32_t *, size_t, void *) = dcs_bf_dm_delays;\n"
        "  int (*g)(dcs_bf_context *, const uint8_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, const int32_t *, uint32_t,\n"
        "           uint32_t, const uint8_t *, uint32_t *, size_t, uint64_t, uint64_t, void *) = dcs_bf_dedisperse_q8;\n"
        "  dcs_bf_band band = {1500.0, -10.0, 64e-6};\n"
        '  printf("%d %d %d %d %d\\n", f != 0, g != 0, DCS_BF_ABI_VERSION, (int)sizeof(band), band.freq_step_mhz < 0);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3", "24", "1"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import SteeringCoefficientGenerator, dm_delays_bytes, dm_time_bytes

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert dm_delays_bytes(bp, 7) == 7 * 5 * 4 and dm_delays_bytes(bp, 0) == 0
    assert dm_time_bytes(3, 7, 11) == 3 * 7 * 11 * 4
    assert dm_time_bytes(2, 4, (1 << 28) + 5) == 2 * 4 * ((1 << 28) + 5) * 4  # past 2^32: a Python int
    assert callable(SteeringCoefficientGenerator.dm_delays) and callable(SteeringCoefficientGenerator.dedisperse_q8)
