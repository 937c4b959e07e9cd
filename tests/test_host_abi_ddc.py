"""The companion library of the digital down-converter (include/dcs_ddc.h, libdcs_ddc.so): it exports exactly what its header
declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python binding has the
header's argument types, the argument checks that need no device in their order, the header from C, and the size helpers.
No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

DIGITS = "dcs_bf_ddc_tap_digits"
DDC = "dcs_bf_ddc"
EXPORTS = {
    DIGITS: [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_size_t, c_void_p],
    DDC: [c_void_p, c_uint32, c_uint32, c_void_p, c_size_t, c_uint64, c_void_p, c_size_t, c_uint32, c_uint32, c_void_p, c_uint64,
          c_void_p, c_size_t, c_uint64, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("ddc", EXPORTS)
    check_header_parameter_kinds("ddc", EXPORTS)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(EXPORTS, "ddc")
    assert dcs_lib.dcs_abi_version() == 3


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    clib = _lib.companion("ddc")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r = c_void_p(base), c_void_p(base + 16), c_void_p(base + 32)
    odd1, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 4), c_void_p(base + 8)
    bands = (ctypes.c_uint32 * 6)()
    bp = ctypes.cast(bands, c_void_p)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED

    def digits(ctx, taps, T, nb, dig, dbytes):
        return getattr(clib, DIGITS)(ctx, taps, T, nb, dig, dbytes, None)

    def ddc(ctx=fp, ni=2, no=3, x=p, xbytes=1 << 20, istride=512, dig=q, dbytes=4096, T=256, nb=1, b=bp, first=0, out=r,
            obytes=1 << 20, ostride=8):
        return getattr(clib, DDC)(ctx, ni, no, x, xbytes, istride, dig, dbytes, T, nb, b, first, out, obytes, ostride, None)

    def refusals():
        assert digits(None, p, 256, 1, q, 4096) == INVALID
        assert digits(fp, None, 256, 1, q, 4096) == INVALID
        assert digits(fp, p, 256, 1, None, 4096) == INVALID
        assert digits(fp, odd1, 256, 1, q, 4096) == INVALID
        for bad in (odd1, odd4, odd8):  # the table is read 16 bytes at a time
            assert digits(fp, p, 256, 1, bad, 4096) == INVALID
        for T in (0, 32, 63, 65, 100, 320, 512):
            assert digits(fp, p, T, 1, q, 1 << 20) == INVALID, T
        for nb in (0, 3):
            assert digits(fp, p, 256, nb, q, 4096) == INVALID, nb
        assert digits(fp, p, 256, 2, q, 4095) == INVALID and digits(fp, p, 64, 1, q, 1023) == INVALID
        # arguments that pass every check made without a device: the fake object is refused without being used
        for T in (64, 128, 192, 256):
            for nb in (1, 2):
                assert digits(fp, p, T, nb, q, 16 * T) == UNSUPPORTED
        assert digits(fp, odd4, 64, 1, q, 1024) == UNSUPPORTED  # int32 taps: 4 bytes

        assert ddc(ctx=None) == INVALID
        assert ddc(dig=None) == INVALID and ddc(b=None) == INVALID and ddc(out=None) == INVALID
        assert ddc(x=None) == INVALID
        for bad in (odd1, odd4, odd8):
            assert ddc(x=bad) == INVALID and ddc(dig=bad) == INVALID
        assert ddc(out=odd1) == INVALID and ddc(out=odd4) == INVALID
        for T in (0, 32, 100, 320):
            assert ddc(T=T) == INVALID, T
        for nb in (0, 3):
            assert ddc(nb=nb) == INVALID, nb
        assert ddc(dbytes=4095) == INVALID
        for istride in (8, 300, 513):  # whole 16-byte chunks
            assert ddc(istride=istride) == INVALID, istride
        assert ddc(ostride=2) == INVALID  # out_stride < nr_out
        assert ddc(istride=272) == INVALID  # a row of 3 outputs reads 32 + 256 = 288 samples
        assert ddc(xbytes=512 + 287) == INVALID  # one byte short: the last row ends after its last sample
        assert ddc(obytes=(8 + 3) * 8 - 1) == INVALID and ddc(nb=2, obytes=(3 * 8 + 3) * 8 - 1) == INVALID  # the last row ends after its last pair
        assert ddc(no=0, ostride=0, obytes=0, x=None, xbytes=0, out=None) == INVALID  # the output pointer is never optional
        assert ddc() == UNSUPPORTED
        assert ddc(xbytes=512 + 288, istride=512, obytes=(8 + 3) * 8) == UNSUPPORTED  # exactly enough
        assert ddc(istride=288, xbytes=576, ostride=3, obytes=48, out=odd8) == UNSUPPORTED
        assert ddc(nb=2, obytes=2 * 2 * 8 * 8, first=(1 << 64) - 1) == UNSUPPORTED
        assert ddc(T=64, dbytes=1024, istride=96, xbytes=192) == UNSUPPORTED
        # nothing to do: no sample is read, so neither the pointer nor the sizes of the samples are looked at
        assert ddc(no=0, x=None, xbytes=0, istride=0, ostride=0, obytes=0) == UNSUPPORTED
        assert ddc(ni=0, x=None, xbytes=0, obytes=0) == UNSUPPORTED
        # sizes whose product passes 2^64 are refused, not wrapped
        assert ddc(ni=0xFFFFFFFF, ostride=1 << 62, obytes=(1 << 64) - 1) == INVALID
        assert ddc(ni=0xFFFFFFFF, istride=1 << 62, xbytes=(1 << 64) - 1, no=3, ostride=3, obytes=(1 << 64) - 1) == INVALID

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 11, 12):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "ddc",
        '#include <stdio.h>\n#include "dcs_ddc.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, const int32_t *, uint32_t, uint32_t, void *, size_t, void *) = dcs_bf_ddc_tap_digits;\n"
        "  int (*g)(dcs_bf_context *, uint32_t, uint32_t, const int8_t *, size_t, uint64_t, const void *, size_t, uint32_t, uint32_t,\n"
        "           const dcs_ddc_band *, uint64_t, float *, size_t, uint64_t, void *) = dcs_bf_ddc;\n"
        "  dcs_ddc_band b = {1u, 2u, 0.5f};\n"
        '  printf("%d %d %d %u %u %u\\n", f != 0, g != 0, DCS_BF_ABI_VERSION, (unsigned)sizeof(b), (unsigned)DCS_DDC_DIGITS_BYTES(256),\n'
        "         DCS_DDC_DECIMATION);\n"
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3", "12", "4096", "16"]


def test_size_helpers():
    from dc_sand_amd.generator import SteeringCoefficientGenerator, ddc_digits_bytes, ddc_out_bytes

    assert [ddc_digits_bytes(t) for t in (64, 128, 192, 256)] == [1024, 2048, 3072, 4096]
    for t in (0, 32, 100, 320):
        with pytest.raises(ValueError):
            ddc_digits_bytes(t)
    assert ddc_out_bytes(3, 40) == 3 * 40 * 8 and ddc_out_bytes(3, 40, 2) == 2 * 3 * 40 * 8
    with pytest.raises(ValueError):
        ddc_out_bytes(3, 40, 3)
    assert callable(SteeringCoefficientGenerator.ddc_tap_digits) and callable(SteeringCoefficientGenerator.ddc)
