"""A selection of tests/test_wcmin_native_gpu.py on the CPU, against the UNMODIFIED library source (tests/emu: the translation
unit with k2_wildcard_round.hpp compiled with g++ on the lock-step wave64 emulator, the specialised module 22 through the stand-in
for hiprtc), and the round tests once more with the lanes of every lock-step interval resumed in reverse: the reduction of a
round's first hit must not depend on which lane or wave arrives first.  This is how the whole feature - kernel, round, loop,
bindings - is exercised on a machine without a GPU."""
from .test_emu_suite_cpu import run_emulated

F = "test_wcmin_native_gpu.py::"
ROUNDS = [F + "test_round_equals_wildcard_batch_and_get_trace[False-65-None]",
          F + "test_round_equals_wildcard_batch_and_get_trace[False-64-64]",
          F + "test_round_equals_wildcard_batch_and_get_trace[True-257-1]",
          F + "test_round_equals_wildcard_batch_and_get_trace[True-1-None]",
          F + "test_round_on_tables_that_run_only_compiled[real3]",
          F + "test_a_round_wider_than_the_kept_budget_is_split[False-257]"]
SELECTION = ROUNDS + [F + "test_native_loop_equals_the_mirror_and_the_transliteration[narrow0-ClockThenSingleton-LAST-0]",
                      F + "test_native_loop_equals_the_mirror_and_the_transliteration[narrow0-ClockThenSingleton-LAST-7]",
                      F + "test_native_loop_equals_the_mirror_and_the_transliteration[narrow0-ClockClusterizer-FIRST-1]",
                      F + "test_native_loop_equals_the_mirror_and_the_transliteration[narrow0-SingletonClusterizer-LAST-0]",
                      F + "test_native_loop_equals_the_mirror_and_the_transliteration[real3-ClockThenSingleton-LAST-0]",
                      F + "test_native_loop_equals_the_mirror_and_the_transliteration[array5-ClockClusterizer-FIRST-7]",
                      F + "test_native_loop_on_the_specialised_narrow_table_and_with_skip_clock_clusters",
                      F + "test_launches_fall_by_one_per_adoption",
                      F + "test_a_capacity_before_the_hit_is_evaluated_again",
                      F + "test_a_capacity_that_stays_is_an_error_by_name",
                      F + "test_refusals_by_name",
                      F + "test_python_entry_points_return_what_their_default_paths_return"]


def test_wildcard_round_and_native_loop_sources_on_the_cpu():
    run_emulated(SELECTION, timeout=900)


def test_the_reduction_does_not_depend_on_the_order_of_the_lanes():
    run_emulated(ROUNDS, lane_order="reverse", timeout=900)
