"""The companion library of staged delay tables (include/dcs_stream_staging.h, libdcs_stream_staging.so): it exports
exactly what its header declares, the product library none of it (its ABI 3 inventory is unchanged), the Python
binding has the header's argument types, the argument checks that need no device, and the flag as a C compiler sees
it.  No GPU needed."""
import ctypes
from ctypes import c_int, c_uint32, c_void_p

from helpers.companion_abi import check_exports_and_binding, compile_against, declared, exported, fake_handle

STAGING = {
    "dcs_bf_stream_stage_table": [c_void_p, c_void_p, c_int],
    "dcs_bf_stream_stage_table_from_global": [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    from dc_sand_amd import _lib

    check_exports_and_binding("stream_staging", STAGING)
    assert not set(STAGING) & exported(_lib.LIB_PATH)  # the product library's exports stay its ABI 3 inventory
    assert not set(STAGING) & declared("dcs_beamformer.h")


def test_staging_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    slib = _lib.companion("stream_staging")
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
    fp = fake_handle().ptr
    assert slib.dcs_bf_stream_stage_table(fp, tp, 2) == _lib.DCS_ERR_INVALID_ARGUMENT
    assert slib.dcs_bf_stream_stage_table(fp, tp, 0) == _lib.DCS_ERR_UNSUPPORTED
    assert slib.dcs_bf_stream_stage_table_from_global(fp, tp, 16, 0, None) == _lib.DCS_ERR_UNSUPPORTED


def test_stage_caller_pinned_flag_compiles_from_c(dcs_lib, tmp_path):
    from dc_sand_amd import _lib

    out = compile_against(
        "stream_staging",
        '#include <stdio.h>\n#include "dcs_stream_staging.h"\n'
        "int main(void) {\n"
        "  int (*stage)(dcs_bf_stream *, const struct dcs_delay_vals *, int) = dcs_bf_stream_stage_table;\n"
        "  int (*stage_g)(dcs_bf_stream *, const void *, uint32_t, uint32_t, void *) = dcs_bf_stream_stage_table_from_global;\n"
        '  printf("%d %d %d\\n", DCS_BF_STAGE_CALLER_PINNED, stage != 0 && stage_g != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == [str(_lib.DCS_BF_STAGE_CALLER_PINNED), "1", "3"] and _lib.DCS_BF_STAGE_CALLER_PINNED == 1
