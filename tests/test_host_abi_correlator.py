"""The companion library of the correlator (include/dcs_correlator.h, libdcs_correlator.so): it exports exactly what its
header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding has the
header's argument types, the argument checks that need no device in their order, the header from C, and the size helpers.
No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_void_p

import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

BLOCK = "dcs_bf_correlate_block"
INTEGRATE = "dcs_bf_integrate_visibilities"
CORRELATOR = {
    BLOCK: [c_void_p, c_uint32, c_void_p, c_size_t, c_uint32, c_void_p, c_size_t, c_void_p],
    INTEGRATE: [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("correlator", CORRELATOR)
    check_header_parameter_kinds("correlator", CORRELATOR)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(CORRELATOR, "correlat")
    check_product_inventory(CORRELATOR, "visibilit")
    assert dcs_lib.dcs_abi_version() == 3


def _block(clib, ctx, nt, ant, n, vis):
    return getattr(clib, BLOCK)(ctx, nt, ant, 0, n, vis, 0, None)


def _integrate(clib, ctx, vis, nr_vis, m, out, accumulate=0):
    return getattr(clib, INTEGRATE)(ctx, vis, 0, nr_vis, m, accumulate, out, 0, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    clib = _lib.companion("correlator")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q = c_void_p(base), c_void_p(base + 16)
    odd1, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        assert _block(clib, None, 16, p, 1, q) == INVALID
        assert _block(clib, fp, 16, p, 1, None) == INVALID
        for bad in (odd1, odd4):  # d_vis holds (re, im) pairs: 8 bytes
            assert _block(clib, fp, 16, p, 1, bad) == INVALID
        for nt in (1, 8, 17, 40):
            assert _block(clib, fp, nt, p, 1, q) == INVALID, nt
        for n in (0, 4096, 5000, 0xFFFFFFFF):  # 1 .. 4095 blocks per visibility
            assert _block(clib, fp, 16 * 8192, p, n, q) == INVALID, n
        for nt, n in ((16, 2), (48, 2), (80, 3), (16 * 4095, 4094)):  # whole visibilities only
            assert _block(clib, fp, nt, p, n, q) == INVALID, (nt, n)
        # arguments that pass every check made without a device: the fake object is refused without being used.  The antenna
        # tensor is the context's side's to check, so neither a null nor a misaligned one is refused here
        assert _block(clib, fp, 16, p, 1, q) == UNSUPPORTED
        assert _block(clib, fp, 16, p, 1, odd8) == UNSUPPORTED
        assert _block(clib, fp, 16 * 4095, p, 4095, q) == UNSUPPORTED
        assert _block(clib, fp, 96, p, 3, q) == UNSUPPORTED
        assert _block(clib, fp, 0, p, 5, q) == UNSUPPORTED
        assert _block(clib, fp, 16, None, 1, q) == UNSUPPORTED
        assert _block(clib, fp, 16, odd8, 1, q) == UNSUPPORTED
        assert _integrate(clib, None, p, 4, 2, q) == INVALID
        assert _integrate(clib, fp, None, 4, 2, q) == INVALID
        assert _integrate(clib, fp, p, 4, 2, None) == INVALID
        for bad in (odd1, odd4):
            assert _integrate(clib, fp, bad, 4, 2, q) == INVALID
        assert _integrate(clib, fp, p, 4, 2, odd1) == INVALID
        for nr_vis, m in ((4, 0), (0, 0), (4, 3), (5, 2), (1, 2)):
            assert _integrate(clib, fp, p, nr_vis, m, q) == INVALID, (nr_vis, m)
        for acc in (0, 1):
            assert _integrate(clib, fp, p, 4, 2, q, acc) == UNSUPPORTED
            assert _integrate(clib, fp, p, 6, 6, q, acc) == UNSUPPORTED
            assert _integrate(clib, fp, p, 0, 2, q, acc) == UNSUPPORTED
            assert _integrate(clib, fp, odd8, 4, 2, odd4, acc) == UNSUPPORTED  # 8 bytes in, 4 bytes out

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 10, 11):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "correlator",
        '#include <stdio.h>\n#include "dcs_correlator.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint32_t, const int8_t *, size_t, uint32_t, int32_t *, size_t, void *) =\n"
        "      dcs_bf_correlate_block;\n"
        "  int (*g)(dcs_bf_context *, const int32_t *, size_t, uint32_t, uint32_t, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_integrate_visibilities;\n"
        '  printf("%d %d %d\\n", f != 0, g != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import SteeringCoefficientGenerator, block_visibilities_bytes, nr_baselines, visibilities_bytes

    assert [nr_baselines(a) for a in (1, 2, 3, 16, 64, 256)] == [1, 3, 6, 136, 2080, 32896]
    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert block_visibilities_bytes(bp, 96, 1) == 5 * 6 * 10 * 8
    assert block_visibilities_bytes(bp, 96, 3) == 5 * 2 * 10 * 8
    assert block_visibilities_bytes(bp, 16 * 4095, 4095) == 5 * 10 * 8
    assert visibilities_bytes(bp, 12, 4) == 3 * 5 * 10 * 8
    assert visibilities_bytes(bp, 12, 12) == 5 * 10 * 8
    for nt, n in ((96, 0), (96, 4), (16 * 4096, 4096)):
        with pytest.raises(ValueError):
            block_visibilities_bytes(bp, nt, n)
    for nr_vis, m in ((12, 0), (12, 5), (3, 4)):
        with pytest.raises(ValueError):
            visibilities_bytes(bp, nr_vis, m)
    assert callable(SteeringCoefficientGenerator.correlate_block) and callable(SteeringCoefficientGenerator.integrate_visibilities)
