"""The device-free argument checks of the RFI flagger's calls (dc_sand_amd/csrc/bf_arg_checks.h: rfi_moments_args,
rfi_flags_args, rfi_clean_q8_args), called directly as tests/test_arg_checks.py calls the others: a stand-alone C++17 program
includes the header, is compiled by the host compiler and run; its printed results are compared.  Every refusal of
include/dcs_rfi.h that needs no context, with the fitting case and the one-short cases beside it.  No GPU and no built
library needed."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

PROGRAM = r"""
#include <cstdio>
#include <limits>
#include "bf_arg_checks.h"

static void status_of(const char *name, int e)
{
    std::printf("%s %s\n", name, e == DCS_OK ? "ok" : e == DCS_ERR_INVALID_ARGUMENT ? "invalid" : "other");
}

int main()
{
    alignas(16) static unsigned char buf[128];
    dcs_bf_context *c = reinterpret_cast<dcs_bf_context *>(buf); // never read: any non-null handle
    const uint8_t *fb = buf, *bytes = buf + 1;
    uint8_t *out = buf + 16;
    const uint32_t *sums = reinterpret_cast<const uint32_t *>(buf + 8), *words = reinterpret_cast<const uint32_t *>(buf + 4);
    const unsigned long long *n8 = reinterpret_cast<const unsigned long long *>(buf + 8);
    const uint64_t max64 = ~0ull;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const dcs_bf_rfi_thresholds good = {6.0, 0.0, 6.0, 0.0, 6.0, 0.0, 2};
    // a window of 4 blocks of 20 spectra from row 10 of 90, 2 beams: the zero-DM series is 2 * 80 words
    const size_t zb = 2 * 80 * 4, sb = 2 * 80, cb = 2 * 3 * 4;

    // ---- rfi_moments_args(c, fb, in_spectra, first, nr_blocks, block_len, nr_beams, cell_sums, zero_dm, zero_dm_bytes)
    status_of("m_fitting", rfi_moments_args(c, fb, 90, 10, 4, 20, 2, sums, words, zb));
    status_of("m_no_zero_dm", rfi_moments_args(c, fb, 90, 10, 4, 20, 2, sums, nullptr, 0));
    status_of("m_nothing_to_do", rfi_moments_args(c, fb, 90, 90, 0, 20, 2, sums, words, 0));
    status_of("m_no_context", rfi_moments_args(nullptr, fb, 90, 10, 4, 20, 2, sums, words, zb));
    status_of("m_no_filterbank", rfi_moments_args(c, nullptr, 90, 10, 4, 20, 2, sums, words, zb));
    status_of("m_no_sums", rfi_moments_args(c, fb, 90, 10, 4, 20, 2, nullptr, words, zb));
    status_of("m_filterbank_at_8", rfi_moments_args(c, fb + 8, 90, 10, 4, 20, 2, sums, words, zb));
    status_of("m_sums_at_4", rfi_moments_args(c, fb, 90, 10, 4, 20, 2, words, words, zb));
    status_of("m_zero_dm_at_2", rfi_moments_args(c, fb, 90, 10, 4, 20, 2, sums, reinterpret_cast<const uint32_t *>(buf + 2), zb));
    status_of("m_no_beams", rfi_moments_args(c, fb, 90, 10, 4, 20, 0, sums, words, zb));
    status_of("m_block_len_0", rfi_moments_args(c, fb, 90, 10, 4, 0, 2, sums, words, zb));
    status_of("m_block_len_65536", rfi_moments_args(c, fb, 1 << 20, 10, 4, 65536, 2, sums, words, max64));
    status_of("m_block_len_65537", rfi_moments_args(c, fb, 1 << 20, 10, 4, 65537, 2, sums, words, max64));
    status_of("m_window_2_32_less_1", rfi_moments_args(c, fb, 1ull << 32, 1, 65537, 65535, 1, sums, words, max64));
    status_of("m_window_2_32", rfi_moments_args(c, fb, 1ull << 33, 1, 65536, 65536, 1, sums, words, max64));
    status_of("m_rows_one_short", rfi_moments_args(c, fb, 89, 10, 4, 20, 2, sums, words, zb));
    status_of("m_first_one_past", rfi_moments_args(c, fb, 90, 11, 4, 20, 2, sums, words, zb));
    status_of("m_first_wraps", rfi_moments_args(c, fb, max64, max64 - 70, 4, 20, 2, sums, words, zb));
    status_of("m_last_rows", rfi_moments_args(c, fb, max64, max64 - 80, 4, 20, 2, sums, words, zb));
    status_of("m_zero_dm_one_short", rfi_moments_args(c, fb, 90, 10, 4, 20, 2, sums, words, zb - 1));
    status_of("m_zero_dm_product_wraps", rfi_moments_args(c, fb, 1ull << 32, 0, 65537, 65535, 0xffffffffu, sums, words, max64));

    // ---- rfi_flags_args(c, cell_sums, zero_dm, zero_dm_bytes, nr_blocks, block_len, nr_beams, thr, cell_flags, channel_mask,
    //                     spectrum_flags, spectrum_flags_bytes, counts, counts_bytes)
    status_of("f_fitting", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_no_zero_dm", rfi_flags_args(c, sums, nullptr, 0, 4, 20, 2, &good, bytes, bytes, nullptr, 0, words, cb));
    status_of("f_no_blocks", rfi_flags_args(c, sums, words, 0, 0, 20, 2, &good, bytes, bytes, bytes, 0, words, cb));
    status_of("f_no_context", rfi_flags_args(nullptr, sums, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_no_sums", rfi_flags_args(c, nullptr, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_no_thresholds", rfi_flags_args(c, sums, words, zb, 4, 20, 2, nullptr, bytes, bytes, bytes, sb, words, cb));
    status_of("f_no_cell_flags", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, nullptr, bytes, bytes, sb, words, cb));
    status_of("f_no_mask", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, nullptr, bytes, sb, words, cb));
    status_of("f_no_counts", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, nullptr, cb));
    status_of("f_sums_at_4", rfi_flags_args(c, words, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_zero_dm_at_1", rfi_flags_args(c, sums, reinterpret_cast<const uint32_t *>(bytes), zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_counts_at_1", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, reinterpret_cast<const uint32_t *>(bytes), cb));
    status_of("f_no_beams", rfi_flags_args(c, sums, words, zb, 4, 20, 0, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_block_len_0", rfi_flags_args(c, sums, words, zb, 4, 0, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_block_len_65537", rfi_flags_args(c, sums, words, max64, 4, 65537, 2, &good, bytes, bytes, bytes, max64, words, cb));
    status_of("f_window_2_32", rfi_flags_args(c, sums, words, max64, 65536, 65536, 1, &good, bytes, bytes, bytes, max64, words, cb));
    status_of("f_window_2_32_less_1", rfi_flags_args(c, sums, words, max64, 65537, 65535, 1, &good, bytes, bytes, bytes, max64, words, cb));
    status_of("f_zero_dm_alone", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, bytes, nullptr, 0, words, cb));
    status_of("f_spectrum_flags_alone", rfi_flags_args(c, sums, nullptr, 0, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_zero_dm_one_short", rfi_flags_args(c, sums, words, zb - 1, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb));
    status_of("f_spectrum_flags_one_short", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb - 1, words, cb));
    status_of("f_counts_one_short", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &good, bytes, bytes, bytes, sb, words, cb - 1));
    status_of("f_product_wraps", rfi_flags_args(c, sums, words, max64, 65537, 65535, 0xffffffffu, &good, bytes, bytes, bytes, max64, words, max64));
    {
        const double bad[] = {nan, inf, -inf, -1.0, -4.9406564584124654e-324};
        const char *names[] = {"nan", "inf", "minus_inf", "minus_1", "minus_denormal"};
        for (int v = 0; v < 5; v++)
            for (int m = 0; m < 6; m++) {
                dcs_bf_rfi_thresholds t = good;
                double *member[] = {&t.mean_thr, &t.mean_floor, &t.var_thr, &t.var_floor, &t.zero_dm_thr, &t.zero_dm_floor};
                *member[m] = bad[v];
                char name[64];
                std::snprintf(name, sizeof name, "f_member_%d_%s", m, names[v]);
                status_of(name, rfi_flags_args(c, sums, words, zb, 4, 20, 2, &t, bytes, bytes, bytes, sb, words, cb));
            }
        const dcs_bf_rfi_thresholds edge = {0.0, 1e308, 1e300, 0.0, 4.9406564584124654e-324, 0.0, 0xffffffffu};
        status_of("f_members_at_their_edges", rfi_flags_args(c, sums, words, zb, 4, 20, 2, &edge, bytes, bytes, bytes, sb, words, cb));
    }

    // ---- rfi_clean_q8_args(c, fb, in_spectra, first, nr_blocks, block_len, nr_beams, out, out_spectra, first_out, replaced)
    status_of("c_fitting", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, out, 85, 5, n8));
    status_of("c_in_place", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, buf, 90, 10, nullptr));
    status_of("c_nothing_to_do", rfi_clean_q8_args(c, fb, 90, 90, 0, 20, 2, out, 85, 85, nullptr));
    status_of("c_no_context", rfi_clean_q8_args(nullptr, fb, 90, 10, 4, 20, 2, out, 85, 5, n8));
    status_of("c_no_filterbank", rfi_clean_q8_args(c, nullptr, 90, 10, 4, 20, 2, out, 85, 5, n8));
    status_of("c_no_output", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, nullptr, 85, 5, n8));
    status_of("c_filterbank_at_8", rfi_clean_q8_args(c, fb + 8, 90, 10, 4, 20, 2, out, 85, 5, n8));
    status_of("c_output_at_8", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, out + 8, 85, 5, n8));
    status_of("c_replaced_at_4", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, out, 85, 5, reinterpret_cast<const unsigned long long *>(buf + 4)));
    status_of("c_no_beams", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 0, out, 85, 5, n8));
    status_of("c_block_len_0", rfi_clean_q8_args(c, fb, 90, 10, 4, 0, 2, out, 85, 5, n8));
    status_of("c_block_len_65537", rfi_clean_q8_args(c, fb, 1 << 20, 10, 4, 65537, 2, out, 1 << 20, 5, n8));
    status_of("c_window_2_32", rfi_clean_q8_args(c, fb, 1ull << 33, 1, 65536, 65536, 1, out, 1ull << 33, 5, n8));
    status_of("c_window_2_32_less_1", rfi_clean_q8_args(c, fb, 1ull << 32, 1, 65537, 65535, 1, out, 1ull << 32, 1, n8));
    status_of("c_rows_in_one_short", rfi_clean_q8_args(c, fb, 89, 10, 4, 20, 2, out, 85, 5, n8));
    status_of("c_rows_out_one_short", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, out, 84, 5, n8));
    status_of("c_first_out_one_past", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, out, 85, 6, n8));
    status_of("c_first_wraps", rfi_clean_q8_args(c, fb, max64, max64 - 70, 4, 20, 2, out, 85, 5, n8));
    status_of("c_first_out_wraps", rfi_clean_q8_args(c, fb, 90, 10, 4, 20, 2, out, max64, max64 - 70, n8));
    status_of("c_last_rows", rfi_clean_q8_args(c, fb, max64, max64 - 80, 4, 20, 2, out, max64, max64 - 80, n8));
    return 0;
}
"""

OK = {"m_fitting", "m_no_zero_dm", "m_nothing_to_do", "m_block_len_65536", "m_window_2_32_less_1", "m_last_rows",
      "f_fitting", "f_no_zero_dm", "f_no_blocks", "f_window_2_32_less_1", "f_members_at_their_edges",
      "c_fitting", "c_in_place", "c_nothing_to_do", "c_window_2_32_less_1", "c_last_rows"}
INVALID = {"m_no_context", "m_no_filterbank", "m_no_sums", "m_filterbank_at_8", "m_sums_at_4", "m_zero_dm_at_2", "m_no_beams",
           "m_block_len_0", "m_block_len_65537", "m_window_2_32", "m_rows_one_short", "m_first_one_past", "m_first_wraps",
           "m_zero_dm_one_short", "m_zero_dm_product_wraps",
           "f_no_context", "f_no_sums", "f_no_thresholds", "f_no_cell_flags", "f_no_mask", "f_no_counts", "f_sums_at_4",
           "f_zero_dm_at_1", "f_counts_at_1", "f_no_beams", "f_block_len_0", "f_block_len_65537", "f_window_2_32",
           "f_zero_dm_alone", "f_spectrum_flags_alone", "f_zero_dm_one_short", "f_spectrum_flags_one_short", "f_counts_one_short",
           "f_product_wraps",
           *[f"f_member_{m}_{v}" for m in range(6) for v in ("nan", "inf", "minus_inf", "minus_1", "minus_denormal")],
           "c_no_context", "c_no_filterbank", "c_no_output", "c_filterbank_at_8", "c_output_at_8", "c_replaced_at_4", "c_no_beams",
           "c_block_len_0", "c_block_len_65537", "c_window_2_32", "c_rows_in_one_short", "c_rows_out_one_short",
           "c_first_out_one_past", "c_first_wraps", "c_first_out_wraps"}
EXPECTED = {**{name: "ok" for name in OK}, **{name: "invalid" for name in INVALID}}


def _host_compiler():
    for cand in ("g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        found = shutil.which(cand)
        if found:
            return found
    raise RuntimeError("no host C++ compiler found (g++, or the clang++ that hipcc drives)")


def test_rfi_args_from_a_stand_alone_program(tmp_path):
    src = tmp_path / "arg_checks_rfi.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "arg_checks_rfi"
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "dc_sand_amd" / "csrc"), str(src),
                    "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(line.split() for line in lines)
    assert not OK & INVALID
    assert len(lines) == len(got) == len(EXPECTED)
    wrong = {k: (got.get(k), v) for k, v in EXPECTED.items() if got.get(k) != v}
    assert not wrong, wrong
