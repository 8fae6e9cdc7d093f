"""tests/test_fuzz_pipeline_gpu.py on the CPU, against the UNMODIFIED kernel sources (tests/emu: the reduction kernels of
csrc/k_fuzz_reduce.hpp, k_fuzz_generate and K1's workgroup-per-test variant compiled with g++ on the lock-step wave64 emulator),
and the reductions once more with the lanes of every lock-step interval resumed in reverse.
Cut there (EMU in the module): the resident summary runs 20 tests x 4 executions instead of 70 x 16; the campaign comparison runs
(tests_per_launch, max_tests) = (8, 20), (3, 17), (64, 13) of the ten pairs; the compiled tables run 7 tests in launches of 3 with
4 executions; the context test runs launches of 8.  The summary's sizes are not cut."""
from .test_emu_suite_cpu import run_emulated

G = "test_fuzz_pipeline_gpu.py::"
SUMMARY = [G + "test_summary_of_crafted_planes", G + "test_summary_refusals"]
SELECTION = SUMMARY + [G + "test_summary_of_resident_results_equals_the_summary_of_copied_results",
                       G + "test_summary_of_resident_results_with_payload_areas",
                       G + "test_pipelined_campaign_equals_the_synchronous_one",
                       G + "test_in_flight_zero_is_two",
                       G + "test_pipelined_campaign_through_the_compiled_tables[raft5]",
                       G + "test_pipelined_campaign_through_the_compiled_tables[big]",
                       G + "test_pipelined_campaign_with_payload_areas",
                       G + "test_executions_beyond_p_max",
                       G + "test_the_context_after_a_campaign_that_discarded_launches",
                       G + "test_refusals"]


def test_fuzz_pipeline_kernel_sources_on_the_cpu():
    run_emulated(SELECTION, timeout=1500)


def test_the_reductions_do_not_depend_on_the_order_of_the_lanes():
    run_emulated(SUMMARY + [G + "test_pipelined_campaign_equals_the_synchronous_one[0-3-17-5-partial_last]"], lane_order="reverse", timeout=900)
