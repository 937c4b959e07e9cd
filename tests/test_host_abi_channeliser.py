"""The companion library of the polyphase channeliser (include/dcs_channeliser.h, libdcs_channeliser.so): it exports exactly
what its header declares, the product library none of it (its ABI 3 inventory of 52 functions is unchanged), the Python
binding has the header's argument types, the argument checks that need no device in their order, the header from C, and the
size helpers.  No GPU needed."""
import ctypes
from ctypes import c_size_t, c_uint32, c_uint64, c_void_p

import pytest

from helpers.companion_abi import (check_exports_and_binding, check_header_parameter_kinds, check_product_inventory,
                                   compile_against, fake_handle)

FLOAT = "dcs_bf_channelise"
Q8 = "dcs_bf_channelise_q8"
EXPORTS = {
    FLOAT: [c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_uint64, c_void_p, c_void_p, c_uint32, c_void_p,
            c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_void_p],
    Q8: [c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p, c_size_t, c_uint64, c_void_p, c_void_p, c_uint32, c_void_p,
         c_void_p, c_size_t, c_uint64, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p],
}


def test_companion_exports_what_its_header_declares_and_is_bound(dcs_lib):
    check_exports_and_binding("channeliser", EXPORTS)
    check_header_parameter_kinds("channeliser", EXPORTS)


def test_product_library_keeps_its_52_functions(dcs_lib):
    check_product_inventory(EXPORTS, "channelise")
    assert dcs_lib.dcs_abi_version() == 3


def test_calls_refuse_bad_arguments_without_a_device(dcs_lib):
    from dc_sand_amd import _lib

    clib = _lib.companion("channeliser")
    buf = (ctypes.c_uint64 * 64)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p, q, r, s, t, u = (c_void_p(base + 16 * i) for i in range(6))
    odd1, odd4, odd8 = c_void_p(base + 1), c_void_p(base + 4), c_void_p(base + 8)
    fake = fake_handle()  # no context of this build: no table at its head
    fp = fake.ptr
    INVALID, UNSUPPORTED = _lib.DCS_ERR_INVALID_ARGUMENT, _lib.DCS_ERR_UNSUPPORTED
    # N = 64, P = 4, 2 inputs, 32 spectra: a row reads (32 + 3) 64 = 2240 pairs; the output is 64 x 5 x 3 runs of 16 pairs
    ROW = 35 * 64

    def call(q8, ctx=fp, N=64, P=4, ni=2, ns=32, x=p, xbytes=None, istride=ROW + 8, h=q, w=r, order=0, g=s, out=t, obytes=None,
             oblocks=5, first=3, oin=3, fin=1, n=u):
        xbytes = ((ni - 1) * istride + (ns + P - 1) * N) * 8 if xbytes is None and ni else (xbytes or 0)
        obytes = N * oblocks * oin * 32 * (1 if q8 else 4) if obytes is None else obytes
        if q8:
            return getattr(clib, Q8)(ctx, N, P, ni, ns, x, xbytes, istride, h, w, order, g, out, obytes, oblocks, first, oin, fin, n, None)
        return getattr(clib, FLOAT)(ctx, N, P, ni, ns, x, xbytes, istride, h, w, order, out, obytes, oblocks, first, oin, fin, None)

    def refusals():
        for q8 in (False, True):
            elem = 1 if q8 else 4

            def c(**kw):
                return call(q8, **kw)

            # pointers
            assert c(ctx=None) == INVALID
            assert c(x=None) == INVALID and c(h=None) == INVALID and c(w=None) == INVALID and c(out=None) == INVALID
            assert c(ctx=None, ns=0) == INVALID and c(ctx=None, ni=0) == INVALID  # the context is never optional
            # alignments: the input and the table 8 bytes, the taps 4, an output 16
            assert c(x=odd1) == INVALID and c(x=odd4) == INVALID and c(x=odd8) == UNSUPPORTED
            assert c(w=odd1) == INVALID and c(w=odd4) == INVALID and c(w=odd8) == UNSUPPORTED
            assert c(h=odd1) == INVALID and c(h=odd4) == UNSUPPORTED
            assert c(out=odd1) == INVALID and c(out=odd4) == INVALID and c(out=odd8) == INVALID
            # the fixed limits
            for N in (0, 1, 32, 63, 65, 96, 4096, 1 << 31):
                assert c(N=N, xbytes=1 << 40, istride=1 << 30, obytes=1 << 40) == INVALID, N
            for P in (0, 17, 1 << 31):
                assert c(P=P, xbytes=1 << 40, istride=1 << 30) == INVALID, P
            for ns in (1, 8, 15, 17, 31, 33):
                assert c(ns=ns, xbytes=1 << 40, istride=1 << 30) == INVALID, ns
            assert c(order=2) == INVALID and c(order=0xFFFFFFFF) == INVALID
            # sizes and windows
            assert c(istride=ROW - 1, xbytes=1 << 40) == INVALID
            assert c(xbytes=(ROW + 8 + ROW) * 8 - 1) == INVALID  # one byte short: the last row ends after its last pair
            assert c(first=4) == INVALID  # blocks 4 and 5 of 5
            assert c(first=(1 << 64) - 1) == INVALID  # first_block + 2 wraps
            assert c(oblocks=(1 << 64) - 1, first=(1 << 64) - 2, obytes=(1 << 64) - 1) == INVALID
            assert c(fin=2) == INVALID  # inputs 2 and 3 of 3
            assert c(fin=0xFFFFFFFF) == INVALID and c(ni=0xFFFFFFFF, oin=0xFFFFFFFF, fin=1, xbytes=(1 << 64) - 1, obytes=(1 << 64) - 1) == INVALID
            assert c(obytes=64 * 5 * 3 * 32 * elem - 1) == INVALID
            # products that pass 2^64 are refused, not wrapped
            assert c(oblocks=1 << 62, obytes=(1 << 64) - 1) == INVALID
            assert c(ni=0xFFFFFFFF, oin=0xFFFFFFFF, fin=0, istride=1 << 62, xbytes=(1 << 64) - 1, obytes=(1 << 64) - 1) == INVALID
            # arguments that pass every check made without a device: the fake object is refused without being used
            assert c() == UNSUPPORTED
            assert c(istride=ROW) == UNSUPPORTED and c(first=0) == UNSUPPORTED and c(fin=0) == UNSUPPORTED
            assert c(order=1) == UNSUPPORTED
            for N in (64, 128, 256, 512, 1024, 2048):
                for P in (1, 16):
                    assert c(N=N, P=P, istride=(32 + P - 1) * N) == UNSUPPORTED, (N, P)
            assert c(oblocks=(1 << 64) - 1, first=(1 << 64) - 3, oin=0xFFFFFFFF, fin=0xFFFFFFFD, N=64, obytes=(1 << 64) - 1) == INVALID  # the tensor
            # nothing to do: no pointer and no size is looked at, the limits still are
            assert c(ns=0, x=None, h=None, w=None, out=None, g=None, xbytes=0, istride=0, obytes=0, oblocks=0, first=0) == UNSUPPORTED
            assert c(ni=0, x=None, h=None, w=None, out=None, g=None, xbytes=0, istride=0, obytes=0, oin=0, fin=0) == UNSUPPORTED
            assert c(ns=0, N=100) == INVALID and c(ni=0, P=0) == INVALID
        # the quantised call's own
        assert call(True, g=None) == INVALID
        assert call(True, g=odd1) == INVALID and call(True, g=odd4) == UNSUPPORTED
        assert call(True, n=odd1) == INVALID and call(True, n=odd4) == INVALID and call(True, n=odd8) == UNSUPPORTED
        assert call(True, n=None) == UNSUPPORTED  # no counting

    refusals()
    # a context whose table is of another version is refused too: the first, and the two before this build's (never this
    # build's own version: the zeroed table would be called)
    for version in (1, 13, 14):
        fake.set_version(version)
        refusals()


def test_header_compiles_from_c(dcs_lib, tmp_path):
    out = compile_against(
        "channeliser",
        '#include <stdio.h>\n#include "dcs_channeliser.h"\n'
        "int main(void) {\n"
        "  int (*f)(dcs_bf_context *, uint32_t, uint32_t, uint32_t, uint32_t, const float *, size_t, uint64_t, const float *,\n"
        "           const float *, uint32_t, float *, size_t, uint64_t, uint64_t, uint32_t, uint32_t, void *) = dcs_bf_channelise;\n"
        "  int (*g)(dcs_bf_context *, uint32_t, uint32_t, uint32_t, uint32_t, const float *, size_t, uint64_t, const float *,\n"
        "           const float *, uint32_t, const float *, int8_t *, size_t, uint64_t, uint64_t, uint32_t, uint32_t,\n"
        "           unsigned long long *, void *) = dcs_bf_channelise_q8;\n"
        '  printf("%d %d %d %u %u %llu\\n", f != 0, g != 0, DCS_BF_ABI_VERSION, DCS_CHAN_ORDER_FFT, DCS_CHAN_ORDER_ASCENDING,\n'
        "         (unsigned long long)DCS_CHAN_IN_PAIRS(2048, 16, 32));\n"
        "  return 0;\n}\n",
        tmp_path)
    assert out == ["1", "1", "3", "0", "1", str(47 * 2048)]


def test_size_helpers():
    from dc_sand_amd.generator import SteeringCoefficientGenerator, channelised_bytes, channeliser_in_pairs

    assert channeliser_in_pairs(64, 1, 16) == 1024 and channeliser_in_pairs(2048, 16, 32) == 47 * 2048
    assert channeliser_in_pairs(64, 4, 0) == 3 * 64
    assert channelised_bytes(64, 5, 3) == 64 * 5 * 3 * 128 and channelised_bytes(64, 5, 3, q8=True) == 64 * 5 * 3 * 32
    for bad in ((32, 1, 16), (96, 1, 16), (4096, 1, 16), (64, 0, 16), (64, 17, 16), (64, 4, 15), (64, 4, -16)):
        with pytest.raises(ValueError):
            channeliser_in_pairs(*bad)
    with pytest.raises(ValueError):
        channelised_bytes(100, 1, 1)
    assert callable(SteeringCoefficientGenerator.channelise) and callable(SteeringCoefficientGenerator.channelise_q8)
