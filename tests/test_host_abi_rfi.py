"""The companion library of the RFI flagger (include/dcs_rfi.h, libdcs_rfi.so): it exports exactly what its header declares,
the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding has the header's
argument types, the argument checks that need no device in their order, the header from C, and the size helpers.  No GPU
needed."""
import ctypes
import re
from ctypes import c_double, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

from helpers.companion_abi import (ROOT, check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

MOMENTS = "dcs_bf_rfi_moments"
FLAGS = "dcs_bf_rfi_flags"
CLEAN = "dcs_bf_rfi_clean_q8"
RFI = {
    MOMENTS: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p, c_size_t,
              c_void_p],
    FLAGS: [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_size_t, c_void_p,
            c_size_t, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p],
    CLEAN: [c_void_p, c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint8,
            c_void_p, c_size_t, c_uint64, c_uint64, c_void_p, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("rfi", RFI)
    check_header_parameter_kinds("rfi", {MOMENTS: RFI[MOMENTS], FLAGS: RFI[FLAGS]})
    # the cleaning call has the one byte passed by value, which the shared check has no kind for: the same check, here
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dcs_rfi.h").read_text(), flags=re.S)
    params = re.search(CLEAN + r"\s*\(([^)]*)\)", text).group(1).split(",")
    assert len(params) == len(RFI[CLEAN])
    for prm, ct in zip(params, RFI[CLEAN]):
        kind = (c_void_p if "*" in prm else c_uint64 if "uint64_t" in prm else c_uint32 if "uint32_t" in prm else
                c_uint8 if "uint8_t" in prm else c_size_t if "size_t" in prm else None)
        assert ct is kind, prm


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(RFI, "rfi")
    assert dcs_lib.dcs_abi_version() == 3


class Thr(ctypes.Structure):
    _fields_ = [("mean_thr", c_double), ("mean_floor", c_double), ("var_thr", c_double), ("var_floor", c_double),
                ("zero_dm_thr", c_double), ("zero_dm_floor", c_double), ("max_bad_blocks", c_uint32)]


def _thr(**kw):
    t = Thr(6.0, 0.0, 6.0, 0.0, 6.0, 0.0, 2)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


BIG = 2**64 - 1


def _moments(rl, ctx, fb, sums, zdm=None, zbytes=BIG, in_spectra=100, first=10, nb=4, n=20, B=2):
    return getattr(rl, MOMENTS)(ctx, fb, 0, in_spectra, first, nb, n, B, sums, 0, zdm, zbytes, None)


def _flags(rl, ctx, sums, cf, cm, counts, thr="good", zdm=None, zbytes=BIG, sf=None, sbytes=BIG, cbytes=BIG, nb=4, n=20, B=2):
    t = _thr() if thr == "good" else thr
    return getattr(rl, FLAGS)(ctx, sums, 0, zdm, zbytes, nb, n, B, None if t is None else ctypes.cast(ctypes.pointer(t), c_void_p),
                              cf, 0, cm, 0, sf, sbytes, counts, cbytes, None)


def _clean(rl, ctx, fb, out, replaced=None, in_spectra=100, first=10, nb=4, n=20, B=2, out_spectra=90, first_out=10, flags=None):
    return getattr(rl, CLEAN)(ctx, fb, 0, in_spectra, first, nb, n, B, flags, flags, flags, 128, out, 0, out_spectra, first_out,
                              replaced, None)


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    rl = _lib.companion("rfi")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r, s = c_void_p(base), c_void_p(base + 16), c_void_p(base + 32), c_void_p(base + 48)
    odd1, odd2, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 2), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED
    inf, nan = float("inf"), float("nan")
    # the windows that do not fit: first + nr_blocks * block_len > spectra, also where a 64-bit sum would wrap
    windows = (dict(in_spectra=89), dict(first=21), dict(nb=5), dict(n=23), dict(in_spectra=0), dict(first=2**64 - 1),
               dict(first=2**64 - 70), dict(in_spectra=2**64 - 1, first=2**64 - 70))
    shapes = (dict(B=0), dict(n=0), dict(n=65537), dict(n=2**32 - 1), dict(nb=65536, n=65536), dict(nb=2**32 - 1, n=2))

    def refusals():
        # -- rfi_moments: NULLs, alignment, then the values
        assert _moments(rl, None, p, q) == INVALID
        assert _moments(rl, fp, None, q) == INVALID
        assert _moments(rl, fp, p, None) == INVALID
        for bad in (odd1, odd2, odd4, odd8):  # the filterbanks are 16-byte aligned
            assert _moments(rl, fp, bad, q) == INVALID
        for bad in (odd1, odd2, odd4):  # a cell is a pair of dwords
            assert _moments(rl, fp, p, bad) == INVALID
        for bad in (odd1, odd2):
            assert _moments(rl, fp, p, q, zdm=bad) == INVALID
        for kw in shapes:
            assert _moments(rl, fp, p, q, in_spectra=2**40, **kw) == INVALID, kw
        for kw in windows:
            assert _moments(rl, fp, p, q, **kw) == INVALID, kw
        assert _moments(rl, fp, p, q, zdm=r, zbytes=2 * 80 * 4 - 1) == INVALID  # the zero-DM series needs no C
        assert _moments(rl, fp, p, q) == UNSUPPORTED
        assert _moments(rl, fp, p, odd8, zdm=odd4, zbytes=2 * 80 * 4) == UNSUPPORTED
        assert _moments(rl, fp, p, q, nb=0) == UNSUPPORTED
        assert _moments(rl, fp, p, q, in_spectra=90) == UNSUPPORTED
        assert _moments(rl, fp, p, q, in_spectra=2**33, first=1, nb=65537, n=65535) == UNSUPPORTED  # 2^32 - 1 spectra
        assert _moments(rl, fp, p, q, in_spectra=2**64 - 1, first=2**64 - 81) == UNSUPPORTED
        # -- rfi_flags
        assert _flags(rl, None, p, q, r, s) == INVALID
        assert _flags(rl, fp, None, q, r, s) == INVALID
        assert _flags(rl, fp, p, None, r, s) == INVALID
        assert _flags(rl, fp, p, q, None, s) == INVALID
        assert _flags(rl, fp, p, q, r, None) == INVALID
        assert _flags(rl, fp, p, q, r, s, thr=None) == INVALID
        for bad in (odd1, odd2, odd4):
            assert _flags(rl, fp, bad, q, r, s) == INVALID
        for bad in (odd1, odd2):
            assert _flags(rl, fp, p, q, r, bad) == INVALID
            assert _flags(rl, fp, p, q, r, s, zdm=bad, sf=q) == INVALID
        for kw in shapes:
            assert _flags(rl, fp, p, q, r, s, **kw) == INVALID, kw
        for member in ("mean_thr", "mean_floor", "var_thr", "var_floor", "zero_dm_thr", "zero_dm_floor"):
            for value in (nan, inf, -inf, -1.0, -5e-324):
                assert _flags(rl, fp, p, q, r, s, thr=_thr(**{member: value})) == INVALID, (member, value)
        assert _flags(rl, fp, p, q, r, s, zdm=p) == INVALID  # the zero-DM series without the spectrum flags
        assert _flags(rl, fp, p, q, r, s, sf=p) == INVALID   # and the reverse
        assert _flags(rl, fp, p, q, r, s, cbytes=23) == INVALID
        assert _flags(rl, fp, p, q, r, s, zdm=p, sf=q, zbytes=2 * 80 * 4 - 1) == INVALID
        assert _flags(rl, fp, p, q, r, s, zdm=p, sf=q, sbytes=2 * 80 - 1) == INVALID
        assert _flags(rl, fp, p, q, r, s) == UNSUPPORTED
        assert _flags(rl, fp, odd8, odd1, odd1, odd4, cbytes=24) == UNSUPPORTED
        assert _flags(rl, fp, p, q, r, s, zdm=odd4, sf=odd1, zbytes=2 * 80 * 4, sbytes=2 * 80) == UNSUPPORTED
        assert _flags(rl, fp, p, q, r, s, thr=_thr(mean_thr=0.0, var_thr=1e300, zero_dm_floor=1e308, max_bad_blocks=2**32 - 1)) == UNSUPPORTED
        assert _flags(rl, fp, p, q, r, s, nb=0) == UNSUPPORTED
        # -- rfi_clean_q8
        assert _clean(rl, None, p, q) == INVALID
        assert _clean(rl, fp, None, q) == INVALID
        assert _clean(rl, fp, p, None) == INVALID
        for bad in (odd1, odd2, odd4, odd8):
            assert _clean(rl, fp, bad, q) == INVALID
            assert _clean(rl, fp, p, bad) == INVALID
        for bad in (odd1, odd2, odd4):
            assert _clean(rl, fp, p, q, replaced=bad) == INVALID
        for kw in shapes:
            assert _clean(rl, fp, p, q, in_spectra=2**40, out_spectra=2**40, **kw) == INVALID, kw
        for kw in windows:
            assert _clean(rl, fp, p, q, **kw) == INVALID, kw
        for kw in (dict(out_spectra=89), dict(first_out=11), dict(out_spectra=0), dict(first_out=2**64 - 1), dict(first_out=2**64 - 70),
                   dict(out_spectra=2**64 - 1, first_out=2**64 - 70)):
            assert _clean(rl, fp, p, q, **kw) == INVALID, kw
        assert _clean(rl, fp, p, q) == UNSUPPORTED
        assert _clean(rl, fp, p, p, replaced=odd8, flags=odd1) == UNSUPPORTED  # in place; flags of any alignment
        assert _clean(rl, fp, p, q, nb=0) == UNSUPPORTED
        assert _clean(rl, fp, p, q, in_spectra=2**64 - 1, first=2**64 - 81, out_spectra=2**64 - 1, first_out=2**64 - 81) == UNSUPPORTED

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 14, 15):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "rfi",
        '#include <stdio.h>\n#include "dcs_rfi.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, const uint8_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t *, size_t,\n"
        "           uint32_t *, size_t, void *) = dcs_bf_rfi_moments;\n"
        "  int (*g)(dcs_bf_context *, const uint32_t *, size_t, const uint32_t *, size_t, uint32_t, uint32_t, uint32_t,\n"
        "           const dcs_bf_rfi_thresholds *, uint8_t *, size_t, uint8_t *, size_t, uint8_t *, size_t, uint32_t *, size_t,\n"
        "           void *) = dcs_bf_rfi_flags;\n"
        "  int (*h)(dcs_bf_context *, const uint8_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t, const uint8_t *,\n"
        "           const uint8_t *, const uint8_t *, uint8_t, uint8_t *, size_t, uint64_t, uint64_t, unsigned long long *,\n"
        "           void *) = dcs_bf_rfi_clean_q8;\n"
        "  dcs_bf_rfi_thresholds thr = {6.0, 0.0, 6.0, 0.0, 6.0, 0.0, 2};\n"
        '  printf("%d %d %d %d %d %d\\n", f != 0, g != 0, h != 0, DCS_BF_ABI_VERSION, (int)sizeof(thr), (int)thr.max_bad_blocks);\n'
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "1", "3", "56", "2"]


def test_size_helpers():
    from dc_sand_amd import BeamformerParameters
    from dc_sand_amd import generator as gen

    bp = BeamformerParameters(NR_CHANNELS=5, NR_STATIONS=4, NR_BEAMS=3)
    assert gen.rfi_cell_sums_bytes(bp, 3, 7) == 3 * 7 * 5 * 8 and gen.rfi_cell_sums_bytes(bp, 3, 0) == 0
    assert gen.rfi_zero_dm_bytes(3, 70) == 3 * 70 * 4
    assert gen.rfi_cell_flags_bytes(bp, 3, 7) == 3 * 7 * 5
    assert gen.rfi_channel_mask_bytes(bp, 3) == 15
    assert gen.rfi_spectrum_flags_bytes(3, 70) == 210
    assert gen.rfi_counts_bytes(3) == 36
    assert gen.rfi_zero_dm_bytes(2, (1 << 31) + 5) == 2 * ((1 << 31) + 5) * 4  # past 2^32: a Python int
    assert ctypes.sizeof(gen._RfiThresholds) == ctypes.sizeof(Thr) == 56
    assert gen.RfiThresholds().mean_thr == 6.0 and gen.RfiThresholds().max_bad_blocks == 0
    for name in ("rfi_moments", "rfi_flags", "rfi_clean_q8"):
        assert callable(getattr(gen.SteeringCoefficientGenerator, name))
