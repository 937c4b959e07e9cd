"""What the host ABI tests of the companion libraries (tests/test_host_abi_*.py) share: each test file states the
argument types it expects, written out, and these checks hold the header, the built library, the table of
dc_sand_amd/companions.py and the bound functions to that statement.  No GPU needed."""
import ctypes
import re
import subprocess
from ctypes import c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]


def _header_text(header):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)


def declared(header):
    return set(re.findall(r"\b(dcs_[a-z0-9_]+)\s*\(", _header_text(header)))


def exported(path):
    syms = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in syms.splitlines() if " T " in l}


def lib_path(key):
    from dc_sand_amd import _lib
    from dc_sand_amd.companions import COMPANIONS

    return _lib.LIB_PATH.parent / COMPANIONS[key].lib


def check_exports_and_binding(key, expected):
    """The companion's header declares, its library exports and its table row lists exactly the names of ``expected``
    ({name: argtypes}); every row returns int and has those argtypes, and so has the bound function."""
    from dc_sand_amd import _lib
    from dc_sand_amd.companions import COMPANIONS

    clib = _lib.companion(key)
    assert declared(COMPANIONS[key].header) == set(expected)
    assert exported(lib_path(key)) == set(expected)
    sigs = {name: (res, args) for name, res, args in COMPANIONS[key].signatures}
    assert set(sigs) == set(expected)
    for name, argtypes in expected.items():
        res, args = sigs[name]
        assert res is c_int and list(args) == argtypes, (name, args)
        assert getattr(clib, name).argtypes == argtypes


def check_header_parameter_kinds(key, expected):
    """The header's own parameter lists: pointer / integer / float kinds in the bound order."""
    from dc_sand_amd.companions import COMPANIONS

    text = _header_text(COMPANIONS[key].header)
    for name, argtypes in expected.items():
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


def check_product_inventory(expected, substring):
    """The product library exports what include/dcs_beamformer.h declares: 52 functions, ABI 3, none of the companion's
    (``expected``) and none with ``substring`` in its name."""
    from dc_sand_amd import _lib

    product = exported(_lib.LIB_PATH)
    assert product == declared("dcs_beamformer.h")
    assert len(product) == 52
    assert not {s for s in product if substring in s}
    assert not set(expected) & declared("dcs_beamformer.h")
    assert _lib.lib().dcs_abi_version() == 3


class FakeHandle:
    """512 zeroed bytes that are no context or stream of this build: no ops table at their head, or with ``version``
    one whose version word is that.  ``ptr`` is what to pass for the handle."""

    def __init__(self, version=None):
        self._obj = (ctypes.c_uint64 * 64)()
        self._ops = (ctypes.c_uint64 * 8)()
        self.ptr = ctypes.cast(self._obj, c_void_p)
        if version is not None:
            self.set_version(version)

    def set_version(self, version):
        ctypes.cast(self._ops, ctypes.POINTER(ctypes.c_uint32))[0] = version
        self._obj[0] = ctypes.addressof(self._ops)


def fake_handle(version=None):
    return FakeHandle(version)


def compile_against(key, c_source, tmp_path):
    """``c_source`` compiled by gcc as C11 with -Wall -Werror against include/, linked with the companion ``key`` and
    the product library, and run: its output, split at white space."""
    path = lib_path(key)
    src = tmp_path / f"{key}.c"
    src.write_text(c_source)
    exe = tmp_path / key
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    "-L", str(path.parent), f"-l:{path.name}", "-l:libdcs_beamformer.so", f"-Wl,-rpath,{path.parent}"], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
