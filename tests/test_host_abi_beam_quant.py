"""The companion library of quantised int8 beam output (include/dcs_beam_quant.h, libdcs_beam_quant.so): it exports exactly
what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python
binding has the header's argument types, the argument checks that need no device, the header from C, and the range check
of BeamQuantGains.  No GPU needed."""
import ctypes
from ctypes import c_float, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

QUANT = {
    "dcs_bf_beamform_accumulated_q8":
        [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p],
    "dcs_bf_beamform_accumulated_q8_dt":
        [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("beam_quant", QUANT)
    check_header_parameter_kinds("beam_quant", QUANT)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(QUANT, "q8")
    assert dcs_lib.dcs_abi_version() == 3


def _call(qlib, name, ctx, nt, gains, weights=None, clips=None):
    first = 0.0 if name.endswith("_dt") else 0
    return getattr(qlib, name)(ctx, first, nt, None, 0, weights, gains, None, 0, clips, None)


def test_quantised_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    qlib = _lib.companion("beam_quant")
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, c_void_p)
    odd2, odd4 = c_void_p(p.value + 2), c_void_p(p.value + 4)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    for name in QUANT:
        assert _call(qlib, name, None, 16, p) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(qlib, name, fp, 16, None) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(qlib, name, fp, 16, odd2) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(qlib, name, fp, 16, p, weights=odd2) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(qlib, name, fp, 16, p, clips=odd4) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(qlib, name, fp, 16, p, clips=odd2) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        for nt in (1, 8, 17, 40):
            assert _call(qlib, name, fp, nt, p) == _lib.DCS_ERR_INVALID_ARGUMENT, (name, nt)
        # arguments that pass every check made without a device: the fake object is refused without being used
        assert _call(qlib, name, fp, 16, p) == _lib.DCS_ERR_UNSUPPORTED, name
        assert _call(qlib, name, fp, 16, odd4, weights=odd4, clips=p) == _lib.DCS_ERR_UNSUPPORTED, name
        assert _call(qlib, name, fp, 0, p) == _lib.DCS_ERR_UNSUPPORTED, name
    # a context whose table is of another version is refused too
    fake.set_version(1)  # the version before the quantiser
    for name in QUANT:
        assert _call(qlib, name, fp, 16, p) == _lib.DCS_ERR_UNSUPPORTED, name


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "beam_quant",
        '#include <stdio.h>\n#include "dcs_beam_quant.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, const float *, int8_t *, size_t,\n"
        "           unsigned long long *, void *) = dcs_bf_beamform_accumulated_q8;\n"
        "  int (*g)(dcs_bf_context *, float, uint32_t, const int8_t *, size_t, const float *, const float *, int8_t *, size_t,\n"
        "           unsigned long long *, void *) = dcs_bf_beamform_accumulated_q8_dt;\n"
        '  printf("%d %d %d\\n", f != 0, g != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3"]


def test_beam_quant_gains_refuses_a_beam_out_of_range():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.beam_quant import BeamQuantGains
    from dc_sand_amd.generator import quantised_beams_bytes

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    qg = BeamQuantGains(bp)
    assert qg.host.shape == (3,) and qg.host.dtype == np.float32 and np.all(qg.host == 1.0)
    for bad in (3, -1, 100):
        with pytest.raises(ValueError):
            qg.set(bad, 2.0)
    qg.set(2, 0.125)
    assert qg.host.tolist() == [1.0, 1.0, 0.125]
    for fn in (qg.device_ptr, qg.clip_count_ptr, qg.clip_counts):
        with pytest.raises(RuntimeError):
            fn()
    assert quantised_beams_bytes(bp, 48) == 5 * 48 * 3 * 2
