"""The companion library of detected beam power (include/dcs_beam_power.h, libdcs_beam_power.so): it exports exactly what
its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding
has the header's argument types, the argument checks that need no device, the header from C, and the size helpers.  No
GPU needed."""
import ctypes
from ctypes import c_float, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

BEAMFORM = {
    "dcs_bf_beamform_accumulated_power": [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_power_dt": [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
}
INTEGRATE = "dcs_bf_integrate_block_power"
POWER = dict(BEAMFORM)
POWER[INTEGRATE] = [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p]


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("beam_power", POWER)
    check_header_parameter_kinds("beam_power", POWER)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(POWER, "power")
    assert dcs_lib.dcs_abi_version() == 3


def _beamform(plib, name, ctx, nt, out, weights=None):
    first = 0.0 if name.endswith("_dt") else 0
    return getattr(plib, name)(ctx, first, nt, None, 0, weights, out, 0, None)


def _integrate(plib, ctx, power, nr_blocks, n, spectra, accumulate=0):
    return getattr(plib, INTEGRATE)(ctx, power, 0, nr_blocks, n, accumulate, spectra, 0, None)


def test_power_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    plib = _lib.companion("beam_power")
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, c_void_p)
    odd1, odd2, odd4 = c_void_p(p.value + 1), c_void_p(p.value + 2), c_void_p(p.value + 4)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals(expected_when_valid):
        for name in BEAMFORM:
            assert _beamform(plib, name, None, 16, p) == INVALID, name
            assert _beamform(plib, name, fp, 16, None) == INVALID, name
            assert _beamform(plib, name, fp, 16, odd2) == INVALID, name
            assert _beamform(plib, name, fp, 16, odd1) == INVALID, name
            assert _beamform(plib, name, fp, 16, p, weights=odd2) == INVALID, name
            for nt in (1, 8, 17, 40):
                assert _beamform(plib, name, fp, nt, p) == INVALID, (name, nt)
            # arguments that pass every check made without a device: the fake object is refused without being used
            assert _beamform(plib, name, fp, 16, p) == expected_when_valid, name
            assert _beamform(plib, name, fp, 16, odd4, weights=odd4) == expected_when_valid, name  # 4-byte alignment is enough
            assert _beamform(plib, name, fp, 0, p) == expected_when_valid, name
        assert _integrate(plib, None, p, 4, 2, odd4) == INVALID
        assert _integrate(plib, fp, None, 4, 2, odd4) == INVALID
        assert _integrate(plib, fp, p, 4, 2, None) == INVALID
        assert _integrate(plib, fp, odd2, 4, 2, p) == INVALID
        assert _integrate(plib, fp, p, 4, 2, odd2) == INVALID
        for nr_blocks, n in ((4, 0), (0, 0), (4, 3), (5, 2), (1, 2)):
            assert _integrate(plib, fp, p, nr_blocks, n, odd4) == INVALID, (nr_blocks, n)
        for acc in (0, 1):
            assert _integrate(plib, fp, p, 4, 2, odd4, acc) == expected_when_valid
            assert _integrate(plib, fp, odd4, 6, 6, p, acc) == expected_when_valid
            assert _integrate(plib, fp, p, 0, 2, odd4, acc) == expected_when_valid

    refusals(UNSUPPORTED)
    # a context whose table is of another version is refused too: the version before the detector, and the first
    for version in (2, 1, 4):
        fake.set_version(version)
        refusals(UNSUPPORTED)


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "beam_power",
        '#include <stdio.h>\n#include "dcs_beam_power.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_power;\n"
        "  int (*g)(dcs_bf_context *, float, uint32_t, const int8_t *, size_t, const float *, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_power_dt;\n"
        "  int (*h)(dcs_bf_context *, const float *, size_t, uint32_t, uint32_t, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_integrate_block_power;\n"
        '  printf("%d %d %d %d\\n", f != 0, g != 0, h != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "1", "3"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.generator import block_power_bytes, power_spectra_bytes

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert block_power_bytes(bp, 48) == 5 * 3 * 3 * 4
    assert power_spectra_bytes(bp, 12, 4) == 3 * 5 * 3 * 4
    assert power_spectra_bytes(bp, 12, 12) == 5 * 3 * 4
    for nr_blocks, n in ((12, 0), (12, 5), (3, 4)):
        with pytest.raises(ValueError):
            power_spectra_bytes(bp, nr_blocks, n)
