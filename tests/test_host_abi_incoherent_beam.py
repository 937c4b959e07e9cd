"""The companion library of the incoherent beam (include/dcs_incoherent_beam.h, libdcs_incoherent_beam.so): it exports
exactly what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the
Python binding has the header's argument types, the argument checks that need no device, the header from C, and the size
helpers.  No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_void_p

import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

BLOCK_POWER = "dcs_bf_incoherent_block_power"
INTEGRATE = "dcs_bf_integrate_incoherent_power"
INCOHERENT = {
    BLOCK_POWER: [c_void_p, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
    INTEGRATE: [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("incoherent_beam", INCOHERENT)
    check_header_parameter_kinds("incoherent_beam", INCOHERENT)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(INCOHERENT, "incoherent")
    assert dcs_lib.dcs_abi_version() == 3


def _block_power(ilib, ctx, nt, out, weights=None):
    return getattr(ilib, BLOCK_POWER)(ctx, nt, None, 0, weights, out, 0, None)


def _integrate(ilib, ctx, power, nr_blocks, n, spectra, accumulate=0):
    return getattr(ilib, INTEGRATE)(ctx, power, 0, nr_blocks, n, accumulate, spectra, 0, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    ilib = _lib.companion("incoherent_beam")
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, c_void_p)
    odd1, odd2, odd4 = c_void_p(p.value + 1), c_void_p(p.value + 2), c_void_p(p.value + 4)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        assert _block_power(ilib, None, 16, p) == INVALID
        assert _block_power(ilib, fp, 16, None) == INVALID
        assert _block_power(ilib, fp, 16, odd2) == INVALID
        assert _block_power(ilib, fp, 16, odd1) == INVALID
        assert _block_power(ilib, fp, 16, p, weights=odd2) == INVALID
        assert _block_power(ilib, fp, 16, p, weights=odd1) == INVALID
        for nt in (1, 8, 17, 40):
            assert _block_power(ilib, fp, nt, p) == INVALID, nt
        # arguments that pass every check made without a device: the fake object is refused without being used
        assert _block_power(ilib, fp, 16, p) == UNSUPPORTED
        assert _block_power(ilib, fp, 16, odd4, weights=odd4) == UNSUPPORTED  # 4-byte alignment is enough
        assert _block_power(ilib, fp, 0, p) == UNSUPPORTED
        assert _integrate(ilib, None, p, 4, 2, odd4) == INVALID
        assert _integrate(ilib, fp, None, 4, 2, odd4) == INVALID
        assert _integrate(ilib, fp, p, 4, 2, None) == INVALID
        assert _integrate(ilib, fp, odd2, 4, 2, p) == INVALID
        assert _integrate(ilib, fp, p, 4, 2, odd2) == INVALID
        for nr_blocks, n in ((4, 0), (0, 0), (4, 3), (5, 2), (1, 2)):
            assert _integrate(ilib, fp, p, nr_blocks, n, odd4) == INVALID, (nr_blocks, n)
        for acc in (0, 1):
            assert _integrate(ilib, fp, p, 4, 2, odd4, acc) == UNSUPPORTED
            assert _integrate(ilib, fp, odd4, 6, 6, p, acc) == UNSUPPORTED
            assert _integrate(ilib, fp, p, 0, 2, odd4, acc) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, the detector's, and the one that is skipped
    # (never this build's own version: the zeroed table would be called)
    for version in (1, 3, 4):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "incoherent_beam",
        '#include <stdio.h>\n#include "dcs_incoherent_beam.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint32_t, const int8_t *, size_t, const float *, uint32_t *, size_t, void *) =\n"
        "      dcs_bf_incoherent_block_power;\n"
        "  int (*g)(dcs_bf_context *, const uint32_t *, size_t, uint32_t, uint32_t, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_integrate_incoherent_power;\n"
        '  printf("%d %d %d\\n", f != 0, g != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import incoherent_block_power_bytes, incoherent_spectra_bytes

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert incoherent_block_power_bytes(bp, 48) == 5 * 3 * 4
    assert incoherent_spectra_bytes(bp, 12, 4) == 3 * 5 * 4
    assert incoherent_spectra_bytes(bp, 12, 12) == 5 * 4
    for nr_blocks, n in ((12, 0), (12, 5), (3, 4)):
        with pytest.raises(ValueError):
            incoherent_spectra_bytes(bp, nr_blocks, n)
