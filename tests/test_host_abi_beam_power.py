"""The companion library of detected beam power (include/dcs_beam_power.h, libdcs_beam_power.so): it exports exactly what
its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding
has the header's argument types, the argument checks that need no device, the header from C, and the size helpers.  No
GPU needed."""
import ctypes
import re
import subprocess
from ctypes import c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

BEAMFORM = {
    "dcs_bf_beamform_accumulated_power": [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_power_dt": [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
}
INTEGRATE = "dcs_bf_integrate_block_power"
POWER = dict(BEAMFORM)
POWER[INTEGRATE] = [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p]


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return set(re.findall(r"\b(dcs_[a-z0-9_]+)\s*\(", text))


def _exported(path):
    syms = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in syms.splitlines() if " T " in l}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    from dc_sand_amd import _lib

    plib = _lib.beam_power_lib()
    assert _declared("dcs_beam_power.h") == set(POWER)
    assert _exported(_lib.POWER_LIB_PATH) == set(POWER)
    sigs = {name: (res, args) for name, res, args in _lib.BEAM_POWER_SIGNATURES}
    assert set(sigs) == set(POWER)
    for name, argtypes in POWER.items():
        res, args = sigs[name]
        assert res is c_int and list(args) == argtypes, (name, args)
        assert getattr(plib, name).argtypes == argtypes
    # the header's own parameter lists: pointer / integer / float kinds in the bound order
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dcs_beam_power.h").read_text(), flags=re.S)
    for name, argtypes in POWER.items():
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(argtypes), name
        for prm, ct in zip(params, argtypes):
            if "*" in prm:
                assert ct is c_void_p, (name, prm)
            elif "float" in prm:
                assert ct is c_float, (name, prm)
            elif "uint64_t" in prm:
                assert ct is c_uint64, (name, prm)
            elif "uint32_t" in prm:
                assert ct is c_uint32, (name, prm)
            else:
                assert "size_t" in prm and ct is c_size_t, (name, prm)


def test_product_library_keeps_its_52_functions(dcs_lib):
    from dc_sand_amd import _lib

    product = _exported(_lib.LIB_PATH)
    assert product == _declared("dcs_beamformer.h")
    assert len(product) == 52
    assert not {s for s in product if "power" in s}
    assert not set(POWER) & _declared("dcs_beamformer.h")
    assert dcs_lib.dcs_abi_version() == 3


def _beamform(plib, name, ctx, nt, out, weights=None):
    first = 0.0 if name.endswith("_dt") else 0
    return getattr(plib, name)(ctx, first, nt, None, 0, weights, out, 0, None)


def _integrate(plib, ctx, power, nr_blocks, n, spectra, accumulate=0):
    return getattr(plib, INTEGRATE)(ctx, power, 0, nr_blocks, n, accumulate, spectra, 0, None)


def test_power_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    plib = _lib.beam_power_lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, c_void_p)
    odd1, odd2, odd4 = c_void_p(p.value + 1), c_void_p(p.value + 2), c_void_p(p.value + 4)
    fake = (ctypes.c_uint64 * 64)()  # no context of this build: no table at its head
    fp = ctypes.cast(fake, c_void_p)
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
    ops = (ctypes.c_uint64 * 8)()
    fake[0] = ctypes.addressof(ops)
    for version in (2, 1, 4):
        ctypes.cast(ops, ctypes.POINTER(ctypes.c_uint32))[0] = version
        refusals(UNSUPPORTED)


def test_header_compiles_from_c(dcs_lib, tmp_path):
    from dc_sand_amd import _lib

    _lib.beam_power_lib()
    src = tmp_path / "p.c"
    src.write_text(
        '#include <stdio.h>\n#include "dcs_beam_power.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_power;\n"
        "  int (*g)(dcs_bf_context *, float, uint32_t, const int8_t *, size_t, const float *, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_power_dt;\n"
        "  int (*h)(dcs_bf_context *, const float *, size_t, uint32_t, uint32_t, uint32_t, float *, size_t, void *) =\n"
        "      dcs_bf_integrate_block_power;\n"
        '  printf("%d %d %d %d\\n", f != 0, g != 0, h != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n"
    )
    exe = tmp_path / "p"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    "-L", str(_lib.POWER_LIB_PATH.parent), "-l:libdcs_beam_power.so", "-l:libdcs_beamformer.so",
                    f"-Wl,-rpath,{_lib.POWER_LIB_PATH.parent}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
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
