"""The companion library of the quantised complex-product beamformer (include/dcs_beam_complex_quant.h,
libdcs_beam_complex_quant.so): it exports exactly the two names its header declares, the product library and the
complex-product companion none of them (the product's ABI 3 inventory of 52 functions is unchanged), the Python binding has
the header's argument types, the argument checks that need no device, and the header from C.  No GPU needed."""
import ctypes
from ctypes import c_float, c_size_t, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, exported, fake_handle, lib_path)

CQ = {
    "dcs_bf_beamform_accumulated_complex_q8":
        [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p],
    "dcs_bf_beamform_accumulated_complex_q8_dt":
        [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_uint32, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("beam_complex_quant", CQ)
    check_header_parameter_kinds("beam_complex_quant", CQ)
    assert len(exported(lib_path("beam_complex_quant"))) == 2


def test_product_library_and_the_complex_companion_keep_their_functions(dcs_lib):
    check_product_inventory(CQ, "complex")
    assert dcs_lib.dcs_abi_version() == 3
    assert not set(CQ) & exported(lib_path("beam_complex"))
    assert not set(CQ) & exported(lib_path("beam_quant"))


def test_generator_has_the_method_with_the_stated_parameters():
    import inspect

    from dc_sand_amd.generator import SteeringCoefficientGenerator

    params = list(inspect.signature(SteeringCoefficientGenerator.beamform_accumulated_complex_q8).parameters)
    assert params == ["self", "d_antenna", "antenna_bytes", "d_quant_gains", "d_beams_q8", "beams_bytes", "nt", "t_coeff",
                      "dt_coeff", "d_weights", "conjugate", "d_clip_count", "stream"]


def _call(clib, name, ctx, nt, gains, out, weights=None, flags=0, clips=None):
    first = 0.0 if name.endswith("_dt") else 0
    return getattr(clib, name)(ctx, first, nt, None, 0, weights, flags, gains, out, 0, clips, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    clib = _lib.companion("beam_complex_quant")
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, c_void_p)
    odd1, odd2, odd4, odd8 = (c_void_p(p.value + n) for n in (1, 2, 4, 8))
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        for name in CQ:
            assert _call(clib, name, None, 16, p, p) == INVALID, name       # no context
            assert _call(clib, name, fp, 16, None, p) == INVALID, name      # no gains
            assert _call(clib, name, fp, 16, p, None) == INVALID, name      # no output
            for odd in (odd1, odd2):                                        # gains and weights: 4-byte aligned
                assert _call(clib, name, fp, 16, odd, p) == INVALID, name
                assert _call(clib, name, fp, 16, p, p, weights=odd) == INVALID, name
            for odd in (odd1, odd2, odd4):                                  # counters and output: 8-byte aligned
                assert _call(clib, name, fp, 16, p, p, clips=odd) == INVALID, name
                assert _call(clib, name, fp, 16, p, odd) == INVALID, name
            for nt in (1, 8, 17, 40):
                assert _call(clib, name, fp, nt, p, p) == INVALID, (name, nt)
            for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFE):
                assert _call(clib, name, fp, 16, p, p, flags=flags) == INVALID, (name, flags)
            # arguments that pass every check made without a device: the fake object is refused without being used
            for flags in (0, 1):
                assert _call(clib, name, fp, 16, p, p, flags=flags) == UNSUPPORTED, name
                assert _call(clib, name, fp, 16, odd4, odd8, weights=odd4, flags=flags, clips=odd8) == UNSUPPORTED, name
                assert _call(clib, name, fp, 0, p, p, flags=flags) == UNSUPPORTED, name

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this companion
    for version in (1, 6, 7):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "beam_complex_quant",
        '#include <stdio.h>\n#include "dcs_beam_complex_quant.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, uint32_t, const float *, int8_t *,\n"
        "           size_t, unsigned long long *, void *) = dcs_bf_beamform_accumulated_complex_q8;\n"
        "  int (*g)(dcs_bf_context *, float, uint32_t, const int8_t *, size_t, const float *, uint32_t, const float *, int8_t *,\n"
        "           size_t, unsigned long long *, void *) = dcs_bf_beamform_accumulated_complex_q8_dt;\n"
        '  printf("%d %d %u %d\\n", f != 0, g != 0, DCS_BF_COMPLEX_CONJ, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "1", "3"]
