"""The companion library of the candidate sifter (include/dcs_candidates.h, libdcs_candidates.so): it exports exactly what
its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding
has the header's argument types, the record is the header's 32 bytes, the argument checks that need no device in their
order, the header from C, and the workspace figure.  No GPU needed."""
import ctypes
from ctypes import c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np

from helpers.companion_abi import (check_header_parameter_kinds, check_product_inventory, compile_against, declared, exported,
                                   fake_handle, lib_path)

WORK = "dcs_bf_candidates_workspace_bytes"
FIND = "dcs_bf_find_candidates"
CANDIDATES = {
    WORK: [c_uint32, c_uint32, c_uint32],
    FIND: [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, c_float,
           c_uint32, c_uint32, c_void_p, c_size_t, c_uint32, c_void_p, c_void_p, c_size_t, c_void_p],
}
RESTYPES = {WORK: c_size_t, FIND: c_int}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    """check_exports_and_binding of helpers/companion_abi.py, with the one row that does not return a status."""
    from dc_sand_amd import _lib
    from dc_sand_amd.companions import COMPANIONS

    clib = _lib.companion("candidates")
    row = COMPANIONS["candidates"]
    assert (row.header, row.source, row.lib) == ("dcs_candidates.h", "bf_candidates.cpp", "libdcs_candidates.so")
    assert declared(row.header) == set(CANDIDATES)
    assert exported(lib_path("candidates")) == set(CANDIDATES)
    sigs = {name: (res, args) for name, res, args in row.signatures}
    assert set(sigs) == set(CANDIDATES)
    for name, argtypes in CANDIDATES.items():
        res, args = sigs[name]
        assert res is RESTYPES[name] and list(args) == argtypes, (name, args)
        assert getattr(clib, name).argtypes == argtypes and getattr(clib, name).restype is RESTYPES[name]
    check_header_parameter_kinds("candidates", CANDIDATES)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(CANDIDATES, "candidate")
    assert dcs_lib.dcs_abi_version() == 3


def _find(clib, ctx, snr, peaks, cands, count, work, peak_blocks=200, first_block=3, nr_blocks=131, B=2, nr_dm=37, nr_widths=3,
          threshold=6.0, dm_radius=1, block_radius=1, max_candidates=5):
    return getattr(clib, FIND)(ctx, snr, 0, peaks, 0, peak_blocks, first_block, nr_blocks, B, nr_dm, nr_widths, threshold, dm_radius,
                               block_radius, cands, 0, max_candidates, count, work, 0, None)


def test_call_refuses_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    clib = _lib.companion("candidates")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r, s, u = (c_void_p(base + 16 * i) for i in range(5))
    odd1, odd2, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 2), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def refusals():
        # NULLs
        assert _find(clib, None, p, q, r, s, u) == INVALID
        assert _find(clib, fp, None, q, r, s, u) == INVALID
        assert _find(clib, fp, p, None, r, s, u) == INVALID
        assert _find(clib, fp, p, q, r, None, u) == INVALID
        assert _find(clib, fp, p, q, r, s, None) == INVALID
        assert _find(clib, fp, p, q, None, s, u) == INVALID  # no records, but max_candidates != 0
        assert _find(clib, fp, None, None, None, None, None, nr_blocks=0, nr_dm=0, max_candidates=0) == INVALID  # nothing to do
        # alignment: the planes' words, the peaks' pairs, the records and the workspace at 8 bytes, the counts' words
        for bad in (odd1, odd2):
            assert _find(clib, fp, bad, q, r, s, u) == INVALID
            assert _find(clib, fp, p, q, r, bad, u) == INVALID
        for bad in (odd1, odd2, odd4):
            assert _find(clib, fp, p, bad, r, s, u) == INVALID
            assert _find(clib, fp, p, q, bad, s, u) == INVALID
            assert _find(clib, fp, p, q, r, s, bad) == INVALID
        # the values
        assert _find(clib, fp, p, q, r, s, u, B=0) == INVALID
        for radius in (9, 16, 2**31, 2**32 - 1):
            assert _find(clib, fp, p, q, r, s, u, dm_radius=radius) == INVALID, radius
            assert _find(clib, fp, p, q, r, s, u, block_radius=radius) == INVALID, radius
        for threshold in (float("nan"), float("inf"), float("-inf")):
            assert _find(clib, fp, p, q, r, s, u, threshold=threshold) == INVALID, threshold
        # first_block + nr_blocks > peak_blocks, also where a 64-bit sum would wrap
        for kw in (dict(peak_blocks=133), dict(first_block=70), dict(nr_blocks=198), dict(peak_blocks=0), dict(first_block=2**64 - 1),
                   dict(peak_blocks=2**64 - 1, first_block=2**64 - 131), dict(nr_blocks=0, first_block=201)):
            assert _find(clib, fp, p, q, r, s, u, **kw) == INVALID, kw
        # arguments that pass every check made without a device: the fake object is refused without being used
        assert _find(clib, fp, p, q, r, s, u) == UNSUPPORTED
        assert _find(clib, fp, odd4, odd8, odd8, odd4, odd8) == UNSUPPORTED
        assert _find(clib, fp, p, q, None, s, u, max_candidates=0) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, dm_radius=8, block_radius=8) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, dm_radius=0, block_radius=0, threshold=-3.0e38) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, nr_blocks=0, first_block=200) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, nr_dm=0) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, nr_widths=0) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, peak_blocks=134, first_block=3) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, peak_blocks=2**64 - 1, first_block=2**64 - 132) == UNSUPPORTED
        assert _find(clib, fp, p, q, r, s, u, B=2**32 - 1, nr_dm=2**32 - 1, nr_blocks=2**32 - 1, peak_blocks=2**33) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 12, 13):
        fake.set_version(version)
        refusals()


def test_record_is_32_bytes_and_header_compiles_from_c(dcs_lib, tmp_path):
    from dc_sand_amd.generator import candidate_dtype

    fields = ("beam", "dm", "width_index", "block", "time", "value", "snr", "members")
    out = compile_against(
        "candidates",
        '#include <stdio.h>\n#include <stddef.h>\n#include "dcs_candidates.h"\n'
        "int main(void) {\n"
        "  size_t (*w)(uint32_t, uint32_t, uint32_t) = dcs_bf_candidates_workspace_bytes;\n"
        "  int (*f)(dcs_bf_context *, const float *, size_t, const uint32_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t,\n"
        "           uint32_t, uint32_t, float, uint32_t, uint32_t, dcs_bf_candidate *, size_t, uint32_t, uint32_t *, void *, size_t,\n"
        "           void *) = dcs_bf_find_candidates;\n"
        "  dcs_bf_candidate c;\n"
        '  printf("%d %d %d %zu %zu\\n", w != 0, f != 0, DCS_BF_ABI_VERSION, sizeof(dcs_bf_candidate), sizeof(c.snr));\n'
        + "".join(f'  printf("%zu\\n", offsetof(dcs_bf_candidate, {name}));\n' for name in fields)
        + '  printf("%zu %zu\\n", w(4, 512, 256), w(0, 512, 256));\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out[:5] == ["1", "1", "3", "32", "4"]
    assert [int(x) for x in out[5:13]] == [4 * i for i in range(8)]
    assert candidate_dtype.names == fields and candidate_dtype.itemsize == 32
    assert [candidate_dtype.fields[n][1] for n in fields] == [4 * i for i in range(8)]
    assert candidate_dtype["snr"] == np.float32 and all(candidate_dtype[n] == np.uint32 for n in fields if n != "snr")
    assert int(out[13]) > 0 and int(out[14]) == 0


def test_workspace_bytes_is_monotone_and_non_zero(dcs_lib):
    from dc_sand_amd.generator import (CANDIDATES_TILE_BLOCKS, SteeringCoefficientGenerator, candidates_bytes,
                                       candidates_workspace_bytes)

    for shape in ((1, 1, 1), (4, 512, 256), (2, 37, 131), (1, 1, 2**32 - 1), (2**32 - 1, 1, 1), (1, 2**32 - 1, 1)):
        assert candidates_workspace_bytes(*shape) > 0 and candidates_workspace_bytes(*shape) % 8 == 0, shape
    for shape in ((0, 5, 5), (5, 0, 5), (5, 5, 0)):
        assert candidates_workspace_bytes(*shape) == 0
    sizes = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 2**20, 2**32 - 1)
    for axis in range(3):
        last = 0
        for n in sizes:
            shape = [3, 5, 70]
            shape[axis] = n
            now = candidates_workspace_bytes(*shape)
            assert now >= last, (axis, n)
            last = now
    # what the three kernels need: per row of a tile of blocks one 64-bit word of marks and one 32-bit place
    segments = 4 * 512 * (-(-256 // CANDIDATES_TILE_BLOCKS))
    assert candidates_workspace_bytes(4, 512, 256) == segments * 12
    assert candidates_workspace_bytes(2**32 - 1, 2**32 - 1, 2**32 - 1) == 2**64 - 1  # does not fit: no buffer is that large
    assert candidates_bytes(0) == 0 and candidates_bytes(3) == 96
    assert callable(SteeringCoefficientGenerator.find_candidates)
