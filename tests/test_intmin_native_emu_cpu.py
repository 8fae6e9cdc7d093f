"""A selection of tests/test_intmin_native_gpu.py on the CPU, against the UNMODIFIED library source (tests/emu: the translation
unit with k2_removal_round.hpp compiled with g++ on the lock-step wave64 emulator), once more with the lanes of every lock-step
interval resumed in reverse: the selection of a round's first hit must not depend on which lane or wave arrives first."""
from .test_emu_suite_cpu import run_emulated

F = "test_intmin_native_gpu.py::"
ROUNDS = [F + "test_round_equals_removal_batch_and_get_kept[False-65]",
          F + "test_round_equals_removal_batch_and_get_kept[False-257]",
          F + "test_round_equals_removal_batch_and_get_kept[True-65]",
          F + "test_a_round_wider_than_the_kept_budget_is_split[False-257]"]
SELECTION = ROUNDS + [F + "test_native_loop_equals_the_sequential_reference[1-SrcDstFIFO-0]",
                      F + "test_native_loop_equals_the_sequential_reference[1-SrcDstFIFO-7]",
                      F + "test_a_capacity_before_the_hit_is_evaluated_again",
                      F + "test_a_capacity_that_stays_is_an_error_by_name",
                      F + "test_refusals_by_name"]


def test_removal_round_and_native_loop_sources_on_the_cpu():
    run_emulated(SELECTION, timeout=600)


def test_the_selection_does_not_depend_on_the_order_of_the_lanes():
    run_emulated(ROUNDS, lane_order="reverse", timeout=600)
