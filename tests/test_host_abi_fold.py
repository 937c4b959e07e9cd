"""The companion library of the pulsar folder (include/dcs_fold.h, libdcs_fold.so): it exports exactly what its header
declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding has the
header's argument types, the argument checks that need no device in their order, the header from C, and the size helpers.
No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory, compile_against,
                                   fake_handle)

FOLD = "dcs_bf_fold_q8"
SCRUNCH = "dcs_bf_fold_scrunch"
ABI = {
    FOLD: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p, c_size_t,
           c_uint32, c_void_p, c_uint32, c_void_p, c_size_t, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_void_p],
    SCRUNCH: [c_void_p, c_void_p, c_size_t, c_uint32, c_uint64, c_uint64, c_uint32, c_uint32, c_void_p, c_size_t, c_uint32, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("fold", ABI)
    check_header_parameter_kinds("fold", ABI)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(ABI, "fold")
    assert dcs_lib.dcs_abi_version() == 3


def _fold(fl, ctx, fb, models, prof, in_spectra=100, first=10, L=20, S=4, B=8, bpm=4, delays=None, max_delay=10, mask=None, nbin=64,
          hits=None, out_subints=9, first_subint=5, accumulate=0):
    return getattr(fl, FOLD)(ctx, fb, 0, in_spectra, first, L, S, B, bpm, models, 0, delays, 0, max_delay, mask, nbin, prof, 0, hits, 0,
                             out_subints, first_subint, accumulate, None)


def _scrunch(fl, ctx, prof, out, B=2, out_subints=9, first_subint=5, S=4, nbin=64, accumulate=0):
    return getattr(fl, SCRUNCH)(ctx, prof, 0, B, out_subints, first_subint, S, nbin, out, 0, accumulate, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    fl = _lib.companion("fold")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r = c_void_p(base), c_void_p(base + 16), c_void_p(base + 32)
    odd1, odd2, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 2), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED
    # the input windows that do not fit: first + S * L + max_delay > in_spectra, also where a 64-bit sum would wrap
    windows = (dict(in_spectra=99), dict(first=11), dict(S=5), dict(L=21), dict(max_delay=11), dict(in_spectra=0), dict(first=2**64 - 1),
               dict(first=2**64 - 80), dict(in_spectra=2**64 - 1, first=2**64 - 80))
    placements = (dict(out_subints=8), dict(first_subint=6), dict(out_subints=0), dict(first_subint=2**64 - 1),
                  dict(out_subints=2**64 - 1, first_subint=2**64 - 3))
    shapes = (dict(B=0), dict(bpm=0), dict(bpm=3), dict(bpm=16), dict(nbin=0), dict(nbin=1025), dict(nbin=2**32 - 1), dict(L=0),
              dict(L=2**24 + 1), dict(L=2**32 - 1), dict(max_delay=2**31 - 1), dict(max_delay=2**32 - 1), dict(accumulate=2),
              dict(accumulate=2**32 - 1))

    def refusals():
        # -- fold_q8: NULLs, alignment, then the values
        assert _fold(fl, None, p, q, r) == INVALID
        assert _fold(fl, fp, None, q, r) == INVALID
        assert _fold(fl, fp, p, None, r) == INVALID
        assert _fold(fl, fp, p, q, None) == INVALID
        for bad in (odd1, odd2, odd4, odd8):  # the filterbanks are 16-byte aligned
            assert _fold(fl, fp, bad, q, r) == INVALID
        for bad in (odd1, odd2, odd4):        # a model is three 64-bit words
            assert _fold(fl, fp, p, bad, r) == INVALID
        for bad in (odd1, odd2):
            assert _fold(fl, fp, p, q, bad) == INVALID
            assert _fold(fl, fp, p, q, r, delays=bad) == INVALID
            assert _fold(fl, fp, p, q, r, hits=bad) == INVALID
        for kw in shapes:
            assert _fold(fl, fp, p, q, r, in_spectra=2**62, **kw) == INVALID, kw
        for kw in windows + placements:
            assert _fold(fl, fp, p, q, r, **kw) == INVALID, kw
        assert _fold(fl, fp, p, q, r) == UNSUPPORTED
        assert _fold(fl, fp, p, odd8, odd4, delays=odd4, hits=odd4, mask=odd1, accumulate=1) == UNSUPPORTED
        assert _fold(fl, fp, p, q, r, S=0, first=90) == UNSUPPORTED       # nothing to do is no refusal
        assert _fold(fl, fp, p, q, r, nbin=1, L=1, bpm=1) == UNSUPPORTED
        assert _fold(fl, fp, p, q, r, nbin=1024, L=2**24, S=2**32 - 1, B=2**32 - 1, bpm=2**32 - 1, in_spectra=2**57, max_delay=2**31 - 2,
                     out_subints=2**33, first_subint=1) == UNSUPPORTED
        assert _fold(fl, fp, p, q, r, in_spectra=2**64 - 1, first=2**64 - 91) == UNSUPPORTED
        # -- fold_scrunch
        assert _scrunch(fl, None, p, q) == INVALID
        assert _scrunch(fl, fp, None, q) == INVALID
        assert _scrunch(fl, fp, p, None) == INVALID
        for bad in (odd1, odd2):
            assert _scrunch(fl, fp, bad, q) == INVALID
        for bad in (odd1, odd2, odd4):
            assert _scrunch(fl, fp, p, bad) == INVALID
        for kw in (dict(B=0), dict(nbin=0), dict(nbin=1025), dict(accumulate=2)) + placements:
            assert _scrunch(fl, fp, p, q, **kw) == INVALID, kw
        assert _scrunch(fl, fp, p, q) == UNSUPPORTED
        assert _scrunch(fl, fp, odd4, odd8, S=0, first_subint=9, accumulate=1, nbin=1024) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 15, 16):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "fold",
        '#include <stdio.h>\n#include "dcs_fold.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, const uint8_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t,\n"
        "           const dcs_bf_fold_model *, size_t, const int32_t *, size_t, uint32_t, const uint8_t *, uint32_t, uint32_t *, size_t,\n"
        "           uint32_t *, size_t, uint64_t, uint64_t, uint32_t, void *) = dcs_bf_fold_q8;\n"
        "  int (*g)(dcs_bf_context *, const uint32_t *, size_t, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t, uint64_t *, size_t,\n"
        "           uint32_t, void *) = dcs_bf_fold_scrunch;\n"
        "  dcs_bf_fold_model m = {1, 2, 3};\n"
        '  printf("%d %d %d %d %d %d\\n", f != 0, g != 0, DCS_BF_ABI_VERSION, (int)sizeof(m), (int)_Alignof(dcs_bf_fold_model), (int)m.accel);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3", "24", "8", "3"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd import fold as design
    from dc_sand_amd import generator as gen

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert gen.fold_profiles_bytes(bp, 3, 7, 11) == 3 * 7 * 5 * 11 * 4 and gen.fold_profiles_bytes(bp, 3, 0, 11) == 0
    assert gen.fold_hits_bytes(2, 7, 11) == 2 * 7 * 11 * 4
    assert gen.fold_scrunched_bytes(3, 7, 11) == 3 * 7 * 11 * 8
    assert gen.fold_profiles_bytes(bp, 2, 2**20, 1024) == 2 * 2**20 * 5 * 1024 * 4 > 1 << 32  # past 2^32: a Python int
    assert gen.fold_scrunched_bytes(2**20, 2**10, 1024) == 2**43 and gen.fold_hits_bytes(2**20, 2**10, 1024) == 2**42
    assert design.model_dtype.itemsize == 24
    for name in ("fold_q8", "fold_scrunch"):
        assert callable(getattr(gen.SteeringCoefficientGenerator, name))
