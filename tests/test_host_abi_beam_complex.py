"""The companion library of the complex-product beamformer (include/dcs_beam_complex.h, libdcs_beam_complex.so): it exports
exactly what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the
Python binding has the header's argument types, the argument checks that need no device, and the header from C.  No GPU
needed."""
import ctypes
from ctypes import c_float, c_size_t, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

COMPLEX = {
    "dcs_bf_beamform_accumulated_complex":
        [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_complex_dt":
        [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_complex_power":
        [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_complex_power_dt":
        [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p, c_size_t, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("beam_complex", COMPLEX)
    check_header_parameter_kinds("beam_complex", COMPLEX)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(COMPLEX, "complex")
    assert dcs_lib.dcs_abi_version() == 3


def _call(clib, name, ctx, nt, out, weights=None, flags=0):
    first = 0.0 if name.endswith("_dt") else 0
    return getattr(clib, name)(ctx, first, nt, None, 0, weights, flags, out, 0, None)


def test_complex_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    clib = _lib.companion("beam_complex")
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, c_void_p)
    odd1, odd2, odd4, odd8 = (c_void_p(p.value + n) for n in (1, 2, 4, 8))
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        for name in COMPLEX:
            power = "_power" in name
            assert _call(clib, name, None, 16, p) == INVALID, name
            assert _call(clib, name, fp, 16, None) == INVALID, name
            assert _call(clib, name, fp, 16, odd1) == INVALID, name
            assert _call(clib, name, fp, 16, odd2) == INVALID, name
            # the float beams are pairs (8-byte aligned), a block power is one float (4-byte aligned)
            assert _call(clib, name, fp, 16, odd4) == (UNSUPPORTED if power else INVALID), name
            assert _call(clib, name, fp, 16, p, weights=odd2) == INVALID, name
            assert _call(clib, name, fp, 16, p, weights=odd1) == INVALID, name
            for nt in (1, 8, 17, 40):
                assert _call(clib, name, fp, nt, p) == INVALID, (name, nt)
            for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
                assert _call(clib, name, fp, 16, p, flags=flags) == INVALID, (name, flags)
            # arguments that pass every check made without a device: the fake object is refused without being used
            for flags in (0, 1):
                assert _call(clib, name, fp, 16, p, flags=flags) == UNSUPPORTED, name
                assert _call(clib, name, fp, 16, odd8, weights=odd4, flags=flags) == UNSUPPORTED, name
                assert _call(clib, name, fp, 0, p, flags=flags) == UNSUPPORTED, name

    refusals()
    # a context whose table is of another version is refused too: the first, earlier ones, and the one before this companion
    for version in (1, 3, 5, 6):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "beam_complex",
        '#include <stdio.h>\n#include "dcs_beam_complex.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_complex;\n"
        "  int (*g)(dcs_bf_context *, float, uint32_t, const int8_t *, size_t, const float *, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_complex_dt;\n"
        "  int (*h)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_complex_power;\n"
        "  int (*k)(dcs_bf_context *, float, uint32_t, const int8_t *, size_t, const float *, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_complex_power_dt;\n"
        '  printf("%d %d %d %d %u %d\\n", f != 0, g != 0, h != 0, k != 0, DCS_BF_COMPLEX_CONJ, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "1", "1", "1", "3"]
