"""The shape tables of the matrix-core beamformer's GPU tests (tests/test_gpu_parity.py, test_gpu_beamformer_exact.py,
test_gpu_beam_weights.py, test_gpu_beam_quant.py, test_gpu_beam_power.py, test_gpu_beam_complex.py,
test_gpu_beam_complex_quant.py) and RUNS, the declared list of the output kinds each test function runs its table with.  The
tests take their parameters from RUNS (shapes_of, weighted_of, math_modes_of), and tests/test_launch_forms.py takes the census
of RUNS with helpers/launch_forms.py: bacc_plan names the instantiation and the geometry of every (shape, kind), on the CPU.
No GPU, no library: importable anywhere."""
from collections import namedtuple

# The shapes of test_beamform_accumulated_on_the_matrix_cores (tests/test_gpu_parity.py) and of the tests that hold
# the same launches bit for bit: staged and kChain, ragged antennas / beams, several beam groups and several workgroups per
# channel
ACC_SHAPES = [(64, 16, 64, 256), (64, 16, 5, 32), (64, 64, 7, 64), (64, 40, 3, 48), (8, 4, 5, 16), (37, 21, 9, 48),
              (130, 3, 4, 16), (4, 40, 7, 32), (9, 5, 3, 16), (129, 33, 2, 32), (256, 17, 2, 16), (1, 1, 1, 16),
              (66, 70, 2, 80), (128, 16, 3, 64), (192, 48, 2, 32), (200, 20, 2, 32), (64, 1024, 1, 32),
              (64, 32, 3, 112), (64, 24, 2, 272), (64, 16, 2, 592), (48, 16, 3, 48), (64, 64, 2, 272),
              (256, 64, 2, 272), (100, 20, 3, 112), (256, 16, 1, 1600), (65, 16, 2, 48),
              # enough workgroups for the XCD-grouped numbering to leave its identity tail (> 8 x the sharers):
              (64, 1024, 9, 32), (130, 20, 9, 32), (256, 64, 9, 16), (192, 48, 11, 48),
              # more than 64 beams at <= 64 antennas (several beam groups per channel, ragged last group)
              (64, 128, 3, 64), (48, 200, 2, 48), (64, 72, 2, 32), (33, 129, 2, 16), (64, 256, 2, 272)]
# The shapes above launch fewer workgroups than the chip holds (1280 four-wave ones of the matrix-core beamformer), and the
# launcher then halves a workgroup's share of the sample blocks until every wave has ONE: the second block of a pair, the
# later pairs and every later trip of the kernels' loops never run at them.  These launch 1280 to 1296 workgroups, so the
# launcher leaves a wave several blocks: (A, B, C, nt, the number of blocks that blocks_on_some_wave must prove).
# staged: 1 tile per workgroup and waves of 3 / 2, 1, 1, 1 blocks (whole and ragged antennas and beams); 2 tiles (shared
# coefficient making); 4 tiles with one beam group (the 8-block cap: 5 / 4 blocks) and with two, ragged; the XCD-grouped
# numbering.  kChain: 2 chunks with a partial one, 2 whole chunks, 3 chunks (a wave without one), 4 whole chunks with a
# ragged last beam group.  Then the deep ones: 4 blocks per wave (two whole pairs), 16 (eight pairs), and kChain's 4.
MIN_DEPTH = 3  # a third block is a live second pair
DEEP_SHAPES_OLDER = [(64, 16, 640, 272, MIN_DEPTH), (37, 9, 640, 272, MIN_DEPTH), (64, 24, 640, 144, MIN_DEPTH),
                     (64, 40, 640, 144, MIN_DEPTH), (48, 72, 320, 144, MIN_DEPTH), (64, 1024, 40, 80, MIN_DEPTH),
                     (100, 20, 320, 272, MIN_DEPTH), (128, 16, 640, 272, MIN_DEPTH), (130, 20, 320, 272, MIN_DEPTH),
                     (256, 33, 216, 272, MIN_DEPTH),
                     (64, 16, 1280, 256, 4), (48, 72, 640, 256, 10), (130, 20, 640, 256, 4)]
DEEPEST_SHAPES = DEEP_SHAPES_OLDER[-3:]
# The geometry classes that none of those has (tests/test_launch_forms.py holds the list to them): staged with two tiles and
# ragged antennas; kChain with four chunks, the last partial, with three whole chunks, and with a second chunk of ONE antenna;
# three workgroups per (channel, beam group), the last one's waves with 2, 2, 2 and 3 blocks (1281 workgroups).  Behind the
# older ones, whose positions decide their entry point (by index or by value, in turn).
DEEP_SHAPES = DEEP_SHAPES_OLDER + [(37, 21, 640, 144, MIN_DEPTH), (200, 20, 320, 272, MIN_DEPTH), (192, 16, 640, 272, MIN_DEPTH),
                                   (65, 16, 640, 272, MIN_DEPTH), (64, 16, 427, 528, MIN_DEPTH)]

# The quantiser's and the detector's (A, B, C, nt): kStaged and kChain, FULL and ragged antennas, ragged beam tiles, odd numbers
# of sample blocks
QUANT_SHAPES = [(4, 2, 8, 16), (64, 16, 64, 256), (64, 256, 4, 64), (130, 3, 4, 16), (129, 33, 2, 32), (200, 20, 2, 32),
                (65, 16, 2, 48), (100, 20, 3, 112), (256, 64, 8, 256)]

# The complex product's
COMPLEX_STAGED = [(8, 4, 5, 16), (64, 16, 2, 32), (37, 21, 3, 48), (64, 40, 3, 48), (64, 72, 2, 32)]
COMPLEX_CHAIN = [(65, 16, 2, 48), (130, 3, 4, 16), (200, 20, 2, 32), (256, 17, 2, 16)]
COMPLEX_SMALL = COMPLEX_STAGED + COMPLEX_CHAIN
COMPLEX_DEEP_OLDER = [(64, 16, 640, 272, 3), (48, 72, 320, 144, 3), (130, 20, 320, 272, 3)]  # kStaged 1 and 4 tiles, kChain
# ... and: staged ragged with one tile, two tiles (two waves share the making of NINE operands), kChain with two whole chunks,
# with four, and with two of which the last is partial
COMPLEX_DEEP = COMPLEX_DEEP_OLDER + [(37, 9, 640, 272, 3), (64, 24, 640, 144, 3), (128, 16, 640, 272, 3), (256, 33, 216, 272, 3),
                                     (100, 20, 320, 272, 3)]
assert all(s in DEEP_SHAPES for s in COMPLEX_DEEP)

# The fp32 fma-chain form (math_mode 8) where a wave takes a second block: its line is 4096 workgroups.  1, 2 and 4 beam tiles
# (3, 3 and 2 blocks on a wave); three chunks of antennas with a partial last one, two whole chunks (2 blocks)
FP32_DEEP_SHAPES = [(8, 4, 2048, 272), (41, 33, 1024, 144), (40, 40, 2048, 64), (130, 5, 2048, 144), (128, 5, 2048, 144)]

# ---- the lists of the small tests, as they stood in the test files
NON_FINITE_SHAPES = [(20, 18, 3, 32), (64, 16, 2, 64), (130, 20, 2, 32), (256, 5, 1, 16)]
NON_FINITE_DEEP_SHAPES = [(64, 16, 1280, 256, 4), (130, 20, 640, 256, 4)]
FULL_SCALE_CASES = [("acc", 64, 16, 2, 32), ("acc", 256, 17, 2, 32), ("acc", 200, 20, 2, 48),
                    ("fused", 48, 5, 2, 16), ("fused", 200, 3, 2, 16)]
ONE_HOT_CASES = [("acc", 37, 21, 2), ("acc", 130, 20, 1), ("acc", 256, 16, 1),
                 ("fused", 37, 5, 2), ("fused", 130, 3, 1)]
FLAGGED_SHAPES = [(64, 16, 3, 64), (37, 21, 4, 48), (130, 20, 2, 32), (256, 17, 2, 16), (4, 40, 3, 32)]
RANDOM_WEIGHT_SHAPES = [(64, 16, 4, 64), (37, 21, 3, 48), (129, 33, 2, 32), (256, 64, 2, 32), (1, 1, 1, 16),
                        (64, 128, 2, 48), (192, 48, 2, 32)]
COUNTER_SHAPES = [(64, 16, 5, 80), (64, 40, 3, 48), (130, 20, 3, 48), (256, 33, 2, 32)]
SPECIAL_SHAPES = [(64, 16, 3, 64), (48, 37, 2, 48), (130, 20, 2, 32), (256, 16, 2, 48)]
NULL_WEIGHT_SHAPES = [(64, 24, 3, 48), (200, 20, 2, 32)]
SUBNORMAL_SHAPES = [(64, 40, 3, 48), (37, 21, 4, 32), (192, 17, 2, 32), (130, 20, 3, 48)]
UNALIGNED_SHAPES = [(64, 40, 3, 48), (192, 17, 2, 32)]
INTEGRATION_SHAPES = [(64, 40, 3, 64), (130, 20, 3, 96), (64, 16, 5, 256), (256, 33, 2, 32)]
REPLAY_SHAPES = [(64, 40, 3, 64), (130, 20, 3, 64)]
SLICE_SHAPES = [(65, 37, 3, 48), (64, 50, 2, 32)]
SLOW_SHAPES = [(37, 21, 3, 48), (200, 20, 2, 32)]
COMPLEX_PAIR_SHAPES = [(64, 16, 2, 32), (130, 20, 2, 32)]


def acc_only(cases):
    """The (A, B, C, nt) of a list's "acc" entries (the others are the fused kernel's); an entry without nt is 16 * A samples."""
    return [tuple(c[1:]) if len(c) == 5 else tuple(c[1:]) + (16 * c[1],) for c in cases if c[0] == "acc"]


# ---- the declared list.  A call is (output kind, weighted, math_mode); math_mode 8 is the fp32 fma-chain form
KINDS = {"float": (False, False, False), "q8": (True, False, False), "power": (False, True, False),
         "complex": (False, False, True), "complex q8": (True, False, True), "complex power": (False, True, True)}  # (quant, power, complex)
F, FW, F8 = ("float", False, 0), ("float", True, 0), ("float", False, 8)
Q, QW, P, PW = ("q8", False, 0), ("q8", True, 0), ("power", False, 0), ("power", True, 0)
CX, CXW = ("complex", False, 0), ("complex", True, 0)
CXQ, CXQW, CXP, CXPW = ("complex q8", False, 0), ("complex q8", True, 0), ("complex power", False, 0), ("complex power", True, 0)

Run = namedtuple("Run", "test table shapes calls")


def _run(test, table, calls, shapes=None):
    return Run(test, table, [tuple(s[:4]) for s in (globals()[table] if shapes is None else shapes)], tuple(calls))


PARITY, EXACT, WEIGHTS = "test_gpu_parity.py::", "test_gpu_beamformer_exact.py::", "test_gpu_beam_weights.py::"
QUANT, POWER, COMPLEX, CQUANT = "test_gpu_beam_quant.py::", "test_gpu_beam_power.py::", "test_gpu_beam_complex.py::", "test_gpu_beam_complex_quant.py::"
RUNS = [
    _run(PARITY + "test_beamform_accumulated_on_the_matrix_cores", "ACC_SHAPES", (F, F8)),
    _run(PARITY + "test_beamform_accumulated_non_finite_coefficients", "NON_FINITE_SHAPES", (F, F8)),
    _run(PARITY + "test_beamform_accumulated_non_finite_coefficients_in_every_pair_of_blocks", "NON_FINITE_DEEP_SHAPES", (F,)),
    _run(PARITY + "test_fp32_chain_form_with_several_blocks_per_wave", "FP32_DEEP_SHAPES", (F8,)),
    _run(EXACT + "test_matrix_core_form_is_the_fixed_point_model_bit_for_bit", "ACC_SHAPES", (F, FW)),
    _run(EXACT + "test_matrix_core_form_with_several_blocks_per_wave_bit_for_bit", "DEEP_SHAPES", (F, FW)),
    _run(EXACT + "test_full_scale_samples_against_unit_coefficients", "FULL_SCALE_CASES", (F, FW), acc_only(FULL_SCALE_CASES)),
    _run(EXACT + "test_one_antenna_at_a_time", "ONE_HOT_CASES", (F, FW), acc_only(ONE_HOT_CASES)),
    _run(WEIGHTS + "test_unit_and_power_of_two_weights_on_the_matrix_cores", "ACC_SHAPES", (F, FW)),
    _run(WEIGHTS + "test_flagged_antennas_contribute_nothing", "FLAGGED_SHAPES", (F, FW)),
    _run(WEIGHTS + "test_random_weights_on_the_matrix_cores_within_the_bound", "RANDOM_WEIGHT_SHAPES", (FW,)),
    _run(QUANT + "test_quantised_output_is_the_model_of_the_float_output", "QUANT_SHAPES", (F, Q, FW, QW)),
    _run(QUANT + "test_quantised_output_with_several_blocks_per_wave", "DEEP_SHAPES", (F, Q, FW, QW)),
    _run(QUANT + "test_counters_add_up_and_stay_zero_without_clipping", "COUNTER_SHAPES", (F, Q)),
    _run(QUANT + "test_special_gains_weights_and_delay_values_touch_their_beam_only", "SPECIAL_SHAPES", (F, Q, FW, QW)),
    _run(QUANT + "test_null_weights_equal_all_ones_weights", "NULL_WEIGHT_SHAPES", (F, Q, QW)),
    _run(QUANT + "test_int8_beams_at_an_address_that_is_8_byte_aligned_only", "UNALIGNED_SHAPES", (F, Q)),
    _run(QUANT + "test_captured_call_picks_up_new_gains_on_replay", "REPLAY_SHAPES", (FW, QW)),
    _run(QUANT + "test_beam_slices_reproduce_the_full_call", "SLICE_SHAPES", (F, Q)),
    _run(POWER + "test_block_power_is_the_model_of_the_float_output", "QUANT_SHAPES", (F, P, FW, PW)),
    _run(POWER + "test_block_power_with_several_blocks_per_wave", "DEEP_SHAPES", (F, P, FW, PW)),
    _run(POWER + "test_special_weights_and_delay_values_touch_their_beam_only", "SPECIAL_SHAPES", (F, P, FW, PW)),
    _run(POWER + "test_null_weights_equal_all_ones_weights", "NULL_WEIGHT_SHAPES", (F, P, PW)),
    _run(POWER + "test_subnormal_squares_are_not_flushed", "SUBNORMAL_SHAPES", (FW, PW)),
    _run(POWER + "test_block_power_at_an_address_that_is_4_byte_aligned_only", "UNALIGNED_SHAPES", (F, P)),
    _run(POWER + "test_integration_is_the_ordered_sum", "INTEGRATION_SHAPES", (FW, PW)),
    _run(POWER + "test_captured_calls_pick_up_new_samples_on_replay", "REPLAY_SHAPES", (FW, PW)),
    _run(POWER + "test_beam_slices_reproduce_the_full_call", "SLICE_SHAPES", (F, P)),
    _run(COMPLEX + "test_complex_product_is_the_model_bit_for_bit", "COMPLEX_SMALL", (F, CX)),
    _run(COMPLEX + "test_one_sample_component_at_a_time_gives_the_planes_of_the_element_wise_call", "COMPLEX_SMALL", (F, CX)),
    _run(COMPLEX + "test_weights", "COMPLEX_SMALL", (CX, CXW)),
    _run(COMPLEX + "test_slow_class_and_nan_delays_against_the_fp64_sum", "SLOW_SHAPES", (CX, CXP)),
    _run(COMPLEX + "test_several_blocks_per_wave_bit_for_bit", "COMPLEX_DEEP", (CX, CXW, CXP, CXPW)),
    _run(COMPLEX + "test_block_power_is_the_model_of_the_complex_float_output", "COMPLEX_SMALL", (F, CX, CXW, CXP, CXPW)),
    _run(COMPLEX + "test_captured_complex_call_replayed_after_a_younger_plain_call", "COMPLEX_PAIR_SHAPES", (F, CX)),
    _run(COMPLEX + "test_a_conjugate_beam_on_its_own_source_adds_coherently", "COMPLEX_PAIR_SHAPES", (F, CX, CXP)),
    _run(CQUANT + "test_bytes_and_counters_are_the_quantised_complex_float_output", "COMPLEX_SMALL", (CX, CXQ, CXW, CXQW)),
    _run(CQUANT + "test_bytes_are_the_quantised_model_on_the_coefficient_bits", "COMPLEX_SMALL", (CXQ, CXQW)),
    _run(CQUANT + "test_not_the_element_wise_quantised_call_but_its_re_plane_without_x_im", "COMPLEX_SMALL", (F, Q, CX, CXQ)),
    _run(CQUANT + "test_several_blocks_per_wave", "COMPLEX_DEEP", (CX, CXQ, CXW, CXQW)),
    _run(CQUANT + "test_special_gains_and_a_nan_delay_touch_their_beam_only", "SPECIAL_SHAPES", (CX, CXQ)),
    _run(CQUANT + "test_null_weights_equal_all_ones_weights", "NULL_WEIGHT_SHAPES", (CX, CXQ, CXQW)),
    _run(CQUANT + "test_int8_beams_at_an_address_that_is_8_byte_aligned_only", "UNALIGNED_SHAPES", (CX, CXQ)),
    _run(CQUANT + "test_captured_call_picks_up_new_gains_on_replay", "REPLAY_SHAPES", (CXW, CXQW)),
    _run(CQUANT + "test_beam_slices_reproduce_the_full_call", "SLICE_SHAPES", (CX, CXQ)),
]
_BY_TEST = {r.test: r for r in RUNS}
assert len(_BY_TEST) == len(RUNS)


def run_of(test):
    return _BY_TEST[test]


def shapes_of(test, raw=False):
    """The table of ``test`` as its parametrize list: (A, B, C, nt), with ``raw`` the table's own entries (a deep table's fifth
    is the number of blocks to prove on some wave; a list that the fused kernel shares begins with the kernel's name)."""
    return list(globals()[_BY_TEST[test].table]) if raw else list(_BY_TEST[test].shapes)


def weighted_of(test):
    """[False, True] where the test is run both ways: the values of its ``weighted`` parameter."""
    return sorted({w for _, w, _ in _BY_TEST[test].calls})


def math_modes_of(test):
    return sorted({m for _, _, m in _BY_TEST[test].calls})


def older_runs():
    """RUNS as the tables and the tests stood before the deep lists were extended: the deep tables' older entries, no fp32 form
    at depth, the complex float call deep without weights only and the detecting complex call deep at A = 130 alone."""
    out = []
    for r in RUNS:
        if r.table == "FP32_DEEP_SHAPES":
            continue
        shapes = {"DEEP_SHAPES": DEEP_SHAPES_OLDER, "COMPLEX_DEEP": COMPLEX_DEEP_OLDER}.get(r.table)
        if r.test == COMPLEX + "test_several_blocks_per_wave_bit_for_bit":
            out.append(_run(r.test, r.table, (CX,), shapes))
            out.append(_run(r.test, r.table, (CXP,), [s for s in shapes if s[0] == 130]))
        else:
            out.append(r if shapes is None else _run(r.test, r.table, r.calls, shapes))
    return out
