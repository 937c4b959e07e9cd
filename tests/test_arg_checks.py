"""The device-free argument checks of the companions' calls (dc_sand_amd/csrc/bf_arg_checks.h), called directly: the three
primitives every check is made of -- holds() and fits() are what the tensors past 4 GiB rest on -- and three of the per-entry
functions with argument sets of the host ABI tests.  A stand-alone C++17 program includes the header, is compiled by the
host compiler and run; its printed results are compared.  No GPU and no built library needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include <cstdio>
#include "bf_arg_checks.h"

static void say(const char *name, bool v) { std::printf("%s %s\n", name, v ? "true" : "false"); }
static void status_of(const char *name, int e)
{
    std::printf("%s %s\n", name, e == DCS_OK ? "ok" : e == DCS_ERR_INVALID_ARGUMENT ? "invalid" : "other");
}

int main()
{
    const uint64_t max64 = ~0ull;
    // holds(have, x, y, z, w): have >= x * y * z * w
    say("holds_zero_x", holds(0, 0, 5, 7, 9));
    say("holds_zero_y", holds(0, 5, 0, 7, 9));
    say("holds_zero_z", holds(0, 5, 7, 0, 9));
    say("holds_zero_w", holds(0, 5, 7, 9, 0));
    say("holds_overflowing_pair_times_zero", holds(0, 1ull << 40, 1ull << 40, 0, 1));
    say("holds_2p32_2p32", holds(max64, 1ull << 32, 1ull << 32, 1, 1));
    say("holds_2p63_2", holds(max64, 1ull << 63, 2, 1, 1));
    say("holds_exact", holds(3u * 5u * 7u * 11u, 3, 5, 7, 11));
    say("holds_one_short", holds(3u * 5u * 7u * 11u - 1u, 3, 5, 7, 11));
    const uint64_t big = ((1ull << 20) + 1u) * (1ull << 11) * 4u; // 2^33 + 2^13
    say("holds_past_2p33_exact", holds(big, (1ull << 20) + 1u, 1ull << 11, 4, 1));
    say("holds_past_2p33_one_short", holds(big - 1u, (1ull << 20) + 1u, 1ull << 11, 4, 1));
    // fits(first, n, total): first + n <= total
    say("fits_wrapping_sum", fits(max64, 1, max64));
    say("fits_to_the_last", fits(max64 - 90u, 90, max64));
    say("fits_nothing_in_nothing", fits(0, 0, 0));
    say("fits_first_past_total", fits(1, 0, 0));
    // aligned(p, bytes)
    alignas(16) static unsigned char buf[64];
    say("aligned_null_4", aligned(nullptr, 4));
    say("aligned_null_8", aligned(nullptr, 8));
    say("aligned_null_16", aligned(nullptr, 16));
    say("aligned_0_16", aligned(buf, 16));
    say("aligned_1_8", aligned(buf + 1, 8));
    say("aligned_2_8", aligned(buf + 2, 8));
    say("aligned_4_8", aligned(buf + 4, 8));
    say("aligned_4_4", aligned(buf + 4, 4));
    say("aligned_8_8", aligned(buf + 8, 8));
    say("aligned_8_16", aligned(buf + 8, 16));
    // three entries, with the values of tests/test_host_abi_single_pulse.py, _dedisperse.py and _stokes.py
    dcs_bf_context *c = reinterpret_cast<dcs_bf_context *>(buf); // never read: any non-null handle
    const uint32_t *p = reinterpret_cast<const uint32_t *>(buf), *q = p + 4, *r = p + 8;
    status_of("boxcar_peaks_fitting", boxcar_peaks_args(c, p, 100, 10, 70, 1, q, 21, 64, r, 5, 3));
    status_of("boxcar_peaks_window_one_past", boxcar_peaks_args(c, p, 100, 10, 70, 1, q, 22, 64, r, 5, 3));
    status_of("boxcar_peaks_blocks_one_past", boxcar_peaks_args(c, p, 100, 10, 70, 1, q, 21, 64, r, 4, 3));
    status_of("boxcar_peaks_no_context", boxcar_peaks_args(nullptr, p, 100, 10, 70, 1, q, 21, 64, r, 5, 3));
    const int32_t *delays = reinterpret_cast<const int32_t *>(q);
    status_of("dedisperse_q8_fitting", dedisperse_q8_args(c, buf, 100, 10, 20, 1, delays, 70, r, 30, 10));
    status_of("dedisperse_q8_window_one_past", dedisperse_q8_args(c, buf, 100, 10, 20, 1, delays, 71, r, 30, 10));
    status_of("dedisperse_q8_filterbank_at_8", dedisperse_q8_args(c, buf + 8, 100, 10, 20, 1, delays, 70, r, 30, 10));
    const int8_t *x = reinterpret_cast<const int8_t *>(buf), *y = x + 16;
    const int32_t *out = reinterpret_cast<const int32_t *>(buf);
    status_of("stokes_block_iquv", stokes_block_args(c, 16, x, y, 4, out));
    status_of("stokes_block_iquv_out_at_8", stokes_block_args(c, 16, x, y, 4, out + 2));
    status_of("stokes_block_i_out_at_4", stokes_block_args(c, 16, x, y, 1, out + 1));
    status_of("stokes_block_two_stokes", stokes_block_args(c, 16, x, y, 2, out));
    status_of("stokes_block_nt_17", stokes_block_args(c, 17, x, y, 4, out));
    return 0;
}
"""

EXPECTED = {
    "holds_zero_x": "true", "holds_zero_y": "true", "holds_zero_z": "true", "holds_zero_w": "true",
    "holds_overflowing_pair_times_zero": "true",  # the present rule: a zero on either side makes the product zero
    "holds_2p32_2p32": "false", "holds_2p63_2": "false",
    "holds_exact": "true", "holds_one_short": "false",
    "holds_past_2p33_exact": "true", "holds_past_2p33_one_short": "false",
    "fits_wrapping_sum": "false", "fits_to_the_last": "true", "fits_nothing_in_nothing": "true", "fits_first_past_total": "false",
    "aligned_null_4": "true", "aligned_null_8": "true", "aligned_null_16": "true", "aligned_0_16": "true",
    "aligned_1_8": "false", "aligned_2_8": "false", "aligned_4_8": "false", "aligned_4_4": "true", "aligned_8_8": "true",
    "aligned_8_16": "false",
    "boxcar_peaks_fitting": "ok", "boxcar_peaks_window_one_past": "invalid", "boxcar_peaks_blocks_one_past": "invalid",
    "boxcar_peaks_no_context": "invalid",
    "dedisperse_q8_fitting": "ok", "dedisperse_q8_window_one_past": "invalid", "dedisperse_q8_filterbank_at_8": "invalid",
    "stokes_block_iquv": "ok", "stokes_block_iquv_out_at_8": "invalid", "stokes_block_i_out_at_4": "ok",
    "stokes_block_two_stokes": "invalid", "stokes_block_nt_17": "invalid",
}


def _host_compiler():
    for cand in ("g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        found = shutil.which(cand)
        if found:
            return found
    raise RuntimeError("no host C++ compiler found (g++, or the clang++ that hipcc drives)")


def test_primitives_and_three_entries(tmp_path):
    src = tmp_path / "arg_checks.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "arg_checks"
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "dc_sand_amd" / "csrc"), str(src),
                    "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(line.split() for line in lines)
    assert len(lines) == len(got) == len(EXPECTED)
    assert got == EXPECTED
