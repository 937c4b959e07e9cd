"""The device-free argument checks of the channeliser's calls (dc_sand_amd/csrc/bf_arg_checks.h: channelise_args,
channelise_q8_args), called directly as tests/test_arg_checks.py calls the others: a stand-alone C++17 program includes the
header, is compiled by the host compiler and run; its printed results are compared.  No GPU and no built library needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include <cstdio>
#include "bf_arg_checks.h"

static void status_of(const char *name, int e)
{
    std::printf("%s %s\n", name, e == DCS_OK ? "ok" : e == DCS_ERR_INVALID_ARGUMENT ? "invalid" : "other");
}

int main()
{
    alignas(16) static unsigned char buf[128];
    dcs_bf_context *c = reinterpret_cast<dcs_bf_context *>(buf); // never read: any non-null handle
    const float *in = reinterpret_cast<const float *>(buf), *taps = in + 1, *tw = in + 2, *gains = in + 3;
    float *out = reinterpret_cast<float *>(buf + 16);
    const int8_t *out8 = reinterpret_cast<const int8_t *>(buf + 32);
    const unsigned long long *n = reinterpret_cast<const unsigned long long *>(buf + 8);
    const uint64_t max64 = ~0ull;
    // N = 64, P = 4, 2 inputs of 32 spectra: a row is 35 * 64 = 2240 pairs; the output [64][5][3][16][2]
    const uint64_t row = 2240, in_bytes = (2248 + row) * 8, out_bytes = 64ull * 5 * 3 * 128;
    status_of("fitting", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("stride_of_a_row", channelise_args(c, 64, 4, 2, 32, in, 2 * row * 8, row, taps, tw, 1, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("stride_one_short", channelise_args(c, 64, 4, 2, 32, in, max64, row - 1, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("in_bytes_one_short", channelise_args(c, 64, 4, 2, 32, in, in_bytes - 1, 2248, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("out_bytes_one_short", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes - 1, 5, 3, 3, 1));
    status_of("q8_quarter_the_bytes", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 1, out_bytes / 4, 5, 3, 3, 1));
    status_of("blocks_one_past", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes, 5, 4, 3, 1));
    status_of("blocks_sum_wraps", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, max64, max64, max64 - 1, 3, 1));
    status_of("inputs_one_past", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 2));
    status_of("tensor_product_wraps", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, max64, 1ull << 62, 3, 3, 1));
    status_of("rows_product_wraps", channelise_args(c, 64, 4, 0xffffffffu, 32, in, max64, 1ull << 62, taps, tw, 0, out, 4, max64, 5, 3, 0xffffffffu, 0));
    status_of("n_63", channelise_args(c, 63, 4, 2, 32, in, max64, 1 << 20, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("n_96", channelise_args(c, 96, 4, 2, 32, in, max64, 1 << 20, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("n_4096", channelise_args(c, 4096, 4, 2, 32, in, max64, 1 << 20, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("n_2048_p_16", channelise_args(c, 2048, 16, 2, 32, in, max64, 47 * 2048, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("p_0", channelise_args(c, 64, 0, 2, 32, in, max64, 1 << 20, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("p_17", channelise_args(c, 64, 17, 2, 32, in, max64, 1 << 20, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("spectra_24", channelise_args(c, 64, 4, 2, 24, in, max64, 1 << 20, taps, tw, 0, out, 4, max64, 5, 3, 3, 1));
    status_of("order_2", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 2, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("no_context", channelise_args(nullptr, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("no_input", channelise_args(c, 64, 4, 2, 32, nullptr, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("input_at_4", channelise_args(c, 64, 4, 2, 32, in + 1, in_bytes, 2248, taps, tw, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("table_at_4", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, taps, 0, out, 4, out_bytes, 5, 3, 3, 1));
    status_of("output_at_8", channelise_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, out + 2, 4, out_bytes, 5, 3, 3, 1));
    status_of("empty_no_pointers", channelise_args(c, 64, 4, 2, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, 4, 0, 0, 0, 0, 0));
    status_of("empty_no_inputs", channelise_args(c, 64, 4, 0, 32, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, 4, 0, 0, 0, 0, 0));
    status_of("empty_bad_n", channelise_args(c, 65, 4, 0, 32, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, 4, 0, 0, 0, 0, 0));
    status_of("q8_fitting", channelise_q8_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, gains, out8, out_bytes / 4, 5, 3, 3, 1, n));
    status_of("q8_no_counters", channelise_q8_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, gains, out8, out_bytes / 4, 5, 3, 3, 1, nullptr));
    status_of("q8_no_gains", channelise_q8_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, nullptr, out8, out_bytes / 4, 5, 3, 3, 1, n));
    status_of("q8_counters_at_4", channelise_q8_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, gains, out8, out_bytes / 4, 5, 3, 3, 1,
                                                    reinterpret_cast<const unsigned long long *>(buf + 4)));
    status_of("q8_one_short", channelise_q8_args(c, 64, 4, 2, 32, in, in_bytes, 2248, taps, tw, 0, gains, out8, out_bytes / 4 - 1, 5, 3, 3, 1, n));
    status_of("q8_empty_no_gains", channelise_q8_args(c, 64, 4, 2, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, 0, nullptr));
    return 0;
}
"""

EXPECTED = {
    "fitting": "ok", "stride_of_a_row": "ok", "stride_one_short": "invalid", "in_bytes_one_short": "invalid",
    "out_bytes_one_short": "invalid", "q8_quarter_the_bytes": "ok", "blocks_one_past": "invalid", "blocks_sum_wraps": "invalid",
    "inputs_one_past": "invalid", "tensor_product_wraps": "invalid", "rows_product_wraps": "invalid",
    "n_63": "invalid", "n_96": "invalid", "n_4096": "invalid", "n_2048_p_16": "ok", "p_0": "invalid", "p_17": "invalid",
    "spectra_24": "invalid", "order_2": "invalid", "no_context": "invalid", "no_input": "invalid", "input_at_4": "invalid",
    "table_at_4": "invalid", "output_at_8": "invalid", "empty_no_pointers": "ok", "empty_no_inputs": "ok", "empty_bad_n": "invalid",
    "q8_fitting": "ok", "q8_no_counters": "ok", "q8_no_gains": "invalid", "q8_counters_at_4": "invalid", "q8_one_short": "invalid",
    "q8_empty_no_gains": "ok",
}


def _host_compiler():
    for cand in ("g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        found = shutil.which(cand)
        if found:
            return found
    raise RuntimeError("no host C++ compiler found (g++, or the clang++ that hipcc drives)")


def test_channelise_args_from_a_stand_alone_program(tmp_path):
    src = tmp_path / "arg_checks_channeliser.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "arg_checks_channeliser"
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "dc_sand_amd" / "csrc"), str(src),
                    "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(line.split() for line in lines)
    assert len(lines) == len(got) == len(EXPECTED)
    assert got == EXPECTED
