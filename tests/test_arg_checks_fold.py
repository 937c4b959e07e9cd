"""The device-free argument checks of the pulsar folder's calls (dc_sand_amd/csrc/bf_arg_checks.h: fold_q8_args,
fold_scrunch_args), called directly as tests/test_arg_checks_rfi.py calls the flagger's: a stand-alone C++17 program includes
the header, is compiled by the host compiler and run; its printed results are compared.  Every refusal of include/dcs_fold.h
that needs no context, with the fitting case and the one-short cases beside it.  No GPU and no built library needed."""
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
    const uint8_t *fb = buf;
    const dcs_bf_fold_model *m = reinterpret_cast<const dcs_bf_fold_model *>(buf + 8), *m4 = reinterpret_cast<const dcs_bf_fold_model *>(buf + 4);
    const int32_t *d = reinterpret_cast<const int32_t *>(buf + 4), *d2 = reinterpret_cast<const int32_t *>(buf + 2);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(buf + 4), *w2 = reinterpret_cast<const uint32_t *>(buf + 2);
    const uint64_t *s = reinterpret_cast<const uint64_t *>(buf + 8), *s4 = reinterpret_cast<const uint64_t *>(buf + 4);
    const uint64_t max64 = ~0ull;

    // ---- fold_q8_args(c, fb, in_spectra, first, subint_len, nr_subints, nr_beams, beams_per_model, models, delays, max_delay, nbin,
    //                   profiles, hits, out_subints, first_subint, accumulate): 4 sub-integrations of 20 from row 10 of 100, delays to 10
    status_of("f_fitting", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_no_delays_no_hits", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, nullptr, 10, 64, w, nullptr, 9, 5, 1));
    status_of("f_nothing_to_do", fold_q8_args(c, fb, 100, 90, 20, 0, 8, 4, m, d, 10, 64, w, w, 9, 9, 0));
    status_of("f_no_context", fold_q8_args(nullptr, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_no_filterbank", fold_q8_args(c, nullptr, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_no_models", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, nullptr, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_no_profiles", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, nullptr, w, 9, 5, 0));
    status_of("f_filterbank_at_8", fold_q8_args(c, fb + 8, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_models_at_4", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m4, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_delays_at_2", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d2, 10, 64, w, w, 9, 5, 0));
    status_of("f_profiles_at_2", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w2, w, 9, 5, 0));
    status_of("f_hits_at_2", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w2, 9, 5, 0));
    status_of("f_no_beams", fold_q8_args(c, fb, 100, 10, 20, 4, 0, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_no_beams_per_model", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 0, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_beams_per_model_no_divisor", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 3, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_beams_per_model_all", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 8, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_nbin_0", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 0, w, w, 9, 5, 0));
    status_of("f_nbin_1", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 1, w, w, 9, 5, 0));
    status_of("f_nbin_1024", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 1024, w, w, 9, 5, 0));
    status_of("f_nbin_1025", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 1025, w, w, 9, 5, 0));
    status_of("f_subint_len_0", fold_q8_args(c, fb, 100, 10, 0, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_subint_len_2_24", fold_q8_args(c, fb, 1ull << 40, 10, 1u << 24, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_subint_len_2_24_and_1", fold_q8_args(c, fb, 1ull << 40, 10, (1u << 24) + 1u, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_max_delay_2_31_less_2", fold_q8_args(c, fb, 1ull << 40, 10, 20, 4, 8, 4, m, d, 0x7ffffffeu, 64, w, w, 9, 5, 0));
    status_of("f_max_delay_2_31_less_1", fold_q8_args(c, fb, 1ull << 40, 10, 20, 4, 8, 4, m, d, 0x7fffffffu, 64, w, w, 9, 5, 0));
    status_of("f_rows_one_short", fold_q8_args(c, fb, 99, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_first_one_past", fold_q8_args(c, fb, 100, 11, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_delay_one_past", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 11, 64, w, w, 9, 5, 0));
    status_of("f_first_wraps", fold_q8_args(c, fb, max64, max64 - 80, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_last_rows", fold_q8_args(c, fb, max64, max64 - 90, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 0));
    status_of("f_largest_window", fold_q8_args(c, fb, 1ull << 57, 0, 1u << 24, 0xffffffffu, 8, 4, m, d, 0x7ffffffeu, 64, w, w, 1ull << 32, 1, 0));
    status_of("f_subints_one_short", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 8, 5, 0));
    status_of("f_first_subint_one_past", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 6, 0));
    status_of("f_first_subint_wraps", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, max64, max64 - 3, 0));
    status_of("f_last_subints", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, max64, max64 - 4, 0));
    status_of("f_accumulate_2", fold_q8_args(c, fb, 100, 10, 20, 4, 8, 4, m, d, 10, 64, w, w, 9, 5, 2));

    // ---- fold_scrunch_args(c, profiles, nr_beams, out_subints, first_subint, nr_subints, nbin, scrunched, accumulate)
    status_of("s_fitting", fold_scrunch_args(c, w, 2, 9, 5, 4, 64, s, 0));
    status_of("s_accumulate", fold_scrunch_args(c, w, 2, 9, 5, 4, 1024, s, 1));
    status_of("s_nothing_to_do", fold_scrunch_args(c, w, 2, 9, 9, 0, 1, s, 0));
    status_of("s_no_context", fold_scrunch_args(nullptr, w, 2, 9, 5, 4, 64, s, 0));
    status_of("s_no_profiles", fold_scrunch_args(c, nullptr, 2, 9, 5, 4, 64, s, 0));
    status_of("s_no_output", fold_scrunch_args(c, w, 2, 9, 5, 4, 64, nullptr, 0));
    status_of("s_profiles_at_2", fold_scrunch_args(c, w2, 2, 9, 5, 4, 64, s, 0));
    status_of("s_output_at_4", fold_scrunch_args(c, w, 2, 9, 5, 4, 64, s4, 0));
    status_of("s_no_beams", fold_scrunch_args(c, w, 0, 9, 5, 4, 64, s, 0));
    status_of("s_nbin_0", fold_scrunch_args(c, w, 2, 9, 5, 4, 0, s, 0));
    status_of("s_nbin_1025", fold_scrunch_args(c, w, 2, 9, 5, 4, 1025, s, 0));
    status_of("s_subints_one_short", fold_scrunch_args(c, w, 2, 8, 5, 4, 64, s, 0));
    status_of("s_first_subint_wraps", fold_scrunch_args(c, w, 2, max64, max64 - 3, 4, 64, s, 0));
    status_of("s_accumulate_2", fold_scrunch_args(c, w, 2, 9, 5, 4, 64, s, 2));
    return 0;
}
"""

OK = {"f_fitting", "f_no_delays_no_hits", "f_nothing_to_do", "f_beams_per_model_all", "f_nbin_1", "f_nbin_1024", "f_subint_len_2_24",
      "f_max_delay_2_31_less_2", "f_last_rows", "f_largest_window", "f_last_subints", "s_fitting", "s_accumulate", "s_nothing_to_do"}
INVALID = {"f_no_context", "f_no_filterbank", "f_no_models", "f_no_profiles", "f_filterbank_at_8", "f_models_at_4", "f_delays_at_2",
           "f_profiles_at_2", "f_hits_at_2", "f_no_beams", "f_no_beams_per_model", "f_beams_per_model_no_divisor", "f_nbin_0", "f_nbin_1025",
           "f_subint_len_0", "f_subint_len_2_24_and_1", "f_max_delay_2_31_less_1", "f_rows_one_short", "f_first_one_past",
           "f_delay_one_past", "f_first_wraps", "f_subints_one_short", "f_first_subint_one_past", "f_first_subint_wraps", "f_accumulate_2",
           "s_no_context", "s_no_profiles", "s_no_output", "s_profiles_at_2", "s_output_at_4", "s_no_beams", "s_nbin_0", "s_nbin_1025",
           "s_subints_one_short", "s_first_subint_wraps", "s_accumulate_2"}
EXPECTED = {**{name: "ok" for name in OK}, **{name: "invalid" for name in INVALID}}


def _host_compiler():
    for cand in ("g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        found = shutil.which(cand)
        if found:
            return found
    raise RuntimeError("no host C++ compiler found (g++, or the clang++ that hipcc drives)")


def test_fold_args_from_a_stand_alone_program(tmp_path):
    src = tmp_path / "arg_checks_fold.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "arg_checks_fold"
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "dc_sand_amd" / "csrc"), str(src),
                    "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(line.split() for line in lines)
    assert not OK & INVALID
    assert len(lines) == len(got) == len(EXPECTED)
    wrong = {k: (got.get(k), v) for k, v in EXPECTED.items() if got.get(k) != v}
    assert not wrong, wrong
