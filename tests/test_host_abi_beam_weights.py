"""The companion library of per-input beam weights (include/dcs_beam_weights.h, libdcs_beam_weights.so): it exports
exactly what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the
Python binding has the header's argument types, the argument checks that need no device, the servlet's count check in
BeamWeights.set, and slice_weights against slice_table.  No GPU needed."""
import ctypes
from ctypes import POINTER, c_float, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from helpers.companion_abi import check_exports_and_binding, check_product_inventory, compile_against, fake_handle

WEIGHTS = {
    "dcs_bf_generate_and_beamform_weighted":
        [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
    "dcs_bf_generate_and_beamform_weighted_dt":
        [c_void_p, POINTER(c_float), c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_weighted":
        [c_void_p, c_uint64, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
    "dcs_bf_beamform_accumulated_weighted_dt":
        [c_void_p, c_float, c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("beam_weights", WEIGHTS)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(WEIGHTS, "weighted")


def _call(wlib, name, ctx, nt, w, t=0):
    if name.endswith("weighted_dt"):
        if "generate" in name:
            dts = (c_float * max(nt, 1))()
            return getattr(wlib, name)(ctx, dts, nt, None, 0, w, None, 0, None)
        return getattr(wlib, name)(ctx, 0.0, nt, None, 0, w, None, 0, None)
    return getattr(wlib, name)(ctx, t, nt, None, 0, w, None, 0, None)


def test_weighted_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    wlib = _lib.companion("beam_weights")
    buf = (ctypes.c_float * 64)()
    w = ctypes.cast(buf, c_void_p)
    w_odd = c_void_p(w.value + 2)
    fp = fake_handle().ptr  # no context of this build: no weights table at its head
    for name in WEIGHTS:
        assert _call(wlib, name, None, 16, w) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(wlib, name, fp, 16, None) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        assert _call(wlib, name, fp, 16, w_odd) == _lib.DCS_ERR_INVALID_ARGUMENT, name
        for nt in (1, 8, 17, 40):
            assert _call(wlib, name, fp, nt, w) == _lib.DCS_ERR_INVALID_ARGUMENT, (name, nt)
        # arguments that pass every check made without a device: the fake object is refused without being used
        assert _call(wlib, name, fp, 16, w) == _lib.DCS_ERR_UNSUPPORTED, name
        assert _call(wlib, name, fp, 0, w) == _lib.DCS_ERR_UNSUPPORTED, name
    # t0 in whole 16-sample blocks
    assert wlib.dcs_bf_generate_and_beamform_weighted(fp, 8, 16, None, 0, w, None, 0, None) == _lib.DCS_ERR_INVALID_ARGUMENT
    assert wlib.dcs_bf_generate_and_beamform_weighted(fp, 32, 16, None, 0, w, None, 0, None) == _lib.DCS_ERR_UNSUPPORTED
    # no fDeltaTime values for a non-empty call
    assert wlib.dcs_bf_generate_and_beamform_weighted_dt(fp, None, 16, None, 0, w, None, 0, None) == _lib.DCS_ERR_INVALID_ARGUMENT


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "beam_weights",
        '#include <stdio.h>\n#include "dcs_beam_weights.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint64_t, uint32_t, const int8_t *, size_t, const float *, float *, size_t, void *) =\n"
        "      dcs_bf_beamform_accumulated_weighted;\n"
        '  printf("%d %d\\n", f != 0, DCS_BF_ABI_VERSION);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "3"]


def test_beam_weights_set_has_the_servlets_count_check():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.beam_weights import BeamWeights

    bw = BeamWeights(BeamformerParameters(NR_STATIONS=4, NR_BEAMS=3))
    assert bw.host.shape == (3, 4) and bw.host.dtype == np.float32 and np.all(bw.host == 1.0)
    with pytest.raises(ValueError, match=r"^3 weights received, expected 4$"):
        bw.set(0, 1.0, 2.0, 3.0)
    with pytest.raises(ValueError, match=r"^5 weights received, expected 4$"):
        bw.set(1, 1, 2, 3, 4, 5)
    with pytest.raises(ValueError):
        bw.set(3, 1, 2, 3, 4)
    bw.set(2, 0.5, 0, -1, 2)
    assert bw.host[2].tolist() == [0.5, 0.0, -1.0, 2.0] and np.all(bw.host[:2] == 1.0)
    with pytest.raises(RuntimeError):
        bw.device_ptr()


@pytest.mark.parametrize("B,world", [(7, 2), (16, 3), (5, 5), (64, 4)])
def test_slice_weights_follows_slice_table(B, world):
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd.parameters import delay_vals_dtype
    from dc_sand_amd.sharding import beam_range, slice_table, slice_weights

    A = 3
    gp = BeamformerParameters(NR_STATIONS=A, NR_BEAMS=B)
    table = np.zeros(A * B, dtype=delay_vals_dtype)
    table["fDelay_s"] = np.arange(A * B)  # table [a][b] = a * B + b (the layout slice_table slices)
    w = np.arange(B * A, dtype=np.float32).reshape(B, A)  # weights [b][a]
    for rank in range(world):
        sh = beam_range(B, world, rank)
        t = slice_table(table, gp, sh).reshape(A, sh.n_beams)
        beams = (t["fDelay_s"][0] - 0).astype(int)  # row a = 0: the shard's global beam numbers
        ws = slice_weights(w, gp, sh)
        assert ws.shape == (sh.n_beams, A) and ws.flags["C_CONTIGUOUS"] and ws.dtype == np.float32
        assert np.array_equal(ws, w[beams])
        assert np.array_equal(beams, np.arange(sh.beam_lo, sh.beam_hi))
