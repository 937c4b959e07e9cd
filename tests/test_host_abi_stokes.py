"""The companion library of the Stokes detection (include/dcs_stokes.h, libdcs_stokes.so): it exports exactly what its header
declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding has the
header's argument types, the argument checks that need no device in their order, the header from C, and the size helpers.
No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_void_p

import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

BLOCK = "dcs_bf_stokes_block"
INTEGRATE = "dcs_bf_integrate_stokes"
STOKES = {
    BLOCK: [c_void_p, c_uint32, c_void_p, c_void_p, c_size_t, c_uint32, c_void_p, c_size_t, c_void_p],
    INTEGRATE: [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("stokes", STOKES)
    check_header_parameter_kinds("stokes", STOKES)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(STOKES, "stokes")
    assert dcs_lib.dcs_abi_version() == 3


def _block(slib, ctx, nt, x, y, ns, out):
    return getattr(slib, BLOCK)(ctx, nt, x, y, 0, ns, out, 0, None)


def _integrate(slib, ctx, block, nr_blocks, n, ns, spectra, accumulate=0):
    return getattr(slib, INTEGRATE)(ctx, block, 0, nr_blocks, n, ns, accumulate, spectra, 0, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    slib = _lib.companion("stokes")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q = c_void_p(base), c_void_p(base + 16)
    odd1, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        for ns in (1, 4):
            assert _block(slib, None, 16, p, q, ns, p) == INVALID
            assert _block(slib, fp, 16, None, q, ns, p) == INVALID
            assert _block(slib, fp, 16, p, None, ns, p) == INVALID
            assert _block(slib, fp, 16, p, q, ns, None) == INVALID
            for bad in (odd1, odd4, odd8):  # the beams are 16-byte aligned
                assert _block(slib, fp, 16, bad, q, ns, p) == INVALID
                assert _block(slib, fp, 16, p, bad, ns, p) == INVALID
            assert _block(slib, fp, 16, p, q, ns, odd1) == INVALID
            for nt in (1, 8, 17, 40):
                assert _block(slib, fp, nt, p, q, ns, p) == INVALID, nt
            # arguments that pass every check made without a device: the fake object is refused without being used
            assert _block(slib, fp, 16, p, q, ns, p) == UNSUPPORTED
            assert _block(slib, fp, 16, p, p, ns, q) == UNSUPPORTED  # the same tensor as both polarisations
            assert _block(slib, fp, 0, p, q, ns, p) == UNSUPPORTED
            assert _integrate(slib, None, p, 4, 2, ns, q) == INVALID
            assert _integrate(slib, fp, None, 4, 2, ns, q) == INVALID
            assert _integrate(slib, fp, p, 4, 2, ns, None) == INVALID
            assert _integrate(slib, fp, odd1, 4, 2, ns, q) == INVALID
            assert _integrate(slib, fp, p, 4, 2, ns, odd1) == INVALID
            for nr_blocks, n in ((4, 0), (0, 0), (4, 3), (5, 2), (1, 2)):
                assert _integrate(slib, fp, p, nr_blocks, n, ns, q) == INVALID, (nr_blocks, n)
            for acc in (0, 1):
                assert _integrate(slib, fp, p, 4, 2, ns, q, acc) == UNSUPPORTED
                assert _integrate(slib, fp, p, 6, 6, ns, q, acc) == UNSUPPORTED
                assert _integrate(slib, fp, p, 0, 2, ns, q, acc) == UNSUPPORTED
        # the outputs are aligned to 4 * nr_stokes bytes: 4 is enough for I and not for IQUV, and neither is 8
        assert _block(slib, fp, 16, p, q, 1, odd4) == UNSUPPORTED
        assert _integrate(slib, fp, odd4, 4, 2, 1, odd8) == UNSUPPORTED
        for bad in (odd4, odd8):
            assert _block(slib, fp, 16, p, q, 4, bad) == INVALID
            assert _integrate(slib, fp, bad, 4, 2, 4, q) == INVALID
            assert _integrate(slib, fp, p, 4, 2, 4, bad) == INVALID
        for ns in (0, 2, 3, 5, 8, 0xFFFFFFFF):
            assert _block(slib, fp, 16, p, q, ns, p) == INVALID, ns
            assert _integrate(slib, fp, p, 4, 2, ns, q) == INVALID, ns

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 7, 8):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "stokes",
        '#include <stdio.h>\n#include "dcs_stokes.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint32_t, const int8_t *, const int8_t *, size_t, uint32_t, int32_t *, size_t, void *) =\n"
        "      dcs_bf_stokes_block;\n"
        "  int (*g)(dcs_bf_context *, const int32_t *, size_t, uint32_t, uint32_t, uint32_t, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_integrate_stokes;\n"
        '  printf("%d %d %d %u %u\\n", f != 0, g != 0, DCS_BF_ABI_VERSION, DCS_BF_STOKES_I, DCS_BF_STOKES_IQUV);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3", "1", "4"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import SteeringCoefficientGenerator, block_stokes_bytes, stokes_spectra_bytes

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert block_stokes_bytes(bp, 48, 1) == 5 * 3 * 3 * 4
    assert block_stokes_bytes(bp, 48, 4) == 5 * 3 * 3 * 4 * 4
    assert stokes_spectra_bytes(bp, 12, 4, 4) == 3 * 5 * 3 * 4 * 4
    assert stokes_spectra_bytes(bp, 12, 12, 1) == 5 * 3 * 4
    for nr_blocks, n in ((12, 0), (12, 5), (3, 4)):
        with pytest.raises(ValueError):
            stokes_spectra_bytes(bp, nr_blocks, n, 4)
    for ns in (0, 2, 3, 5):
        with pytest.raises(ValueError):
            block_stokes_bytes(bp, 48, ns)
        with pytest.raises(ValueError):
            stokes_spectra_bytes(bp, 12, 4, ns)
    assert callable(SteeringCoefficientGenerator.stokes_block) and callable(SteeringCoefficientGenerator.integrate_stokes)
