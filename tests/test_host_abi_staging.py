"""The companion library of staged delay tables (include/dcs_stream_staging.h, libdcs_stream_staging.so): it exports
exactly what its header declares, the product library none of it (its ABI 3 inventory is unchanged), the Python
binding has the header's argument types, the argument checks that need no device, and the flag as a C compiler sees
it.  No GPU needed."""
import ctypes
import re
import subprocess
from ctypes import c_int, c_uint32, c_void_p
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

STAGING = {
    "dcs_bf_stream_stage_table": [c_void_p, c_void_p, c_int],
    "dcs_bf_stream_stage_table_from_global": [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p],
}


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return set(re.findall(r"\b(dcs_[a-z0-9_]+)\s*\(", text))


def _exported(path):
    syms = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in syms.splitlines() if " T " in l}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    from dc_sand_amd import _lib

    slib = _lib.staging_lib()
    assert _declared("dcs_stream_staging.h") == set(STAGING)
    assert _exported(_lib.STAGING_LIB_PATH) == set(STAGING)
    assert not set(STAGING) & _exported(_lib.LIB_PATH)  # the product library's exports stay its ABI 3 inventory
    assert not set(STAGING) & _declared("dcs_beamformer.h")
    sigs = {name: (res, args) for name, res, args in _lib.STAGING_SIGNATURES}
    assert set(sigs) == set(STAGING)
    for name, argtypes in STAGING.items():
        res, args = sigs[name]
        assert res is c_int and list(args) == argtypes, (name, args)
        assert getattr(slib, name).argtypes == argtypes


def test_staging_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    slib = _lib.staging_lib()
    table = (ctypes.c_float * 4)()
    tp = ctypes.cast(table, c_void_p)
    assert slib.dcs_bf_stream_stage_table(None, tp, 0) == _lib.DCS_ERR_INVALID_ARGUMENT
    assert slib.dcs_bf_stream_stage_table(None, None, 0) == _lib.DCS_ERR_INVALID_ARGUMENT
    for flags in (_lib.DCS_BF_STAGE_CALLER_PINNED, 2, -1, 3):
        assert slib.dcs_bf_stream_stage_table(None, tp, flags) == _lib.DCS_ERR_INVALID_ARGUMENT
    assert slib.dcs_bf_stream_stage_table_from_global(None, None, 16, 0, None) == _lib.DCS_ERR_INVALID_ARGUMENT
    assert slib.dcs_bf_stream_stage_table_from_global(None, tp, 16, 0, None) == _lib.DCS_ERR_INVALID_ARGUMENT
    # an unknown flag is refused before the stream is looked at; an object that is no stream of this build (no
    # staging table at its head) is refused without being used
    fake = (ctypes.c_uint64 * 64)()
    fp = ctypes.cast(fake, c_void_p)
    assert slib.dcs_bf_stream_stage_table(fp, tp, 2) == _lib.DCS_ERR_INVALID_ARGUMENT
    assert slib.dcs_bf_stream_stage_table(fp, tp, 0) == _lib.DCS_ERR_UNSUPPORTED
    assert slib.dcs_bf_stream_stage_table_from_global(fp, tp, 16, 0, None) == _lib.DCS_ERR_UNSUPPORTED


def test_stage_caller_pinned_flag_compiles_from_c(dcs_lib, tmp_path):
    from dc_sand_amd import _lib

    _lib.staging_lib()
    src = tmp_path / "flag.c"
    src.write_text(
        '#include <stdio.h>\n#include "dcs_stream_staging.h"\n'
        "int main(void) {\n"
        "  int (*stage)(dcs_bf_stream *, const struct dcs_delay_vals *, int) = dcs_bf_stream_stage_table;\n"
        "  int (*stage_g)(dcs_bf_stream *, const void *, uint32_t, uint32_t, void *) = dcs_bf_stream_stage_table_from_global;\n"
        '  printf("%d %d %d\\n", DCS_BF_STAGE_CALLER_PINNED, stage != 0 && stage_g != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n"
    )
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    str(_lib.STAGING_LIB_PATH), f"-Wl,-rpath,{_lib.STAGING_LIB_PATH.parent}"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(_lib.DCS_BF_STAGE_CALLER_PINNED), "1", "3"] and _lib.DCS_BF_STAGE_CALLER_PINNED == 1
