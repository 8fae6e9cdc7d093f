"""A selection of tests/test_fuzz_campaign_gpu.py on the CPU, against the UNMODIFIED kernel sources (tests/emu: k_fuzz_generate
and K1's workgroup-per-test variant compiled with g++ on the lock-step wave64 emulator, the specialised kernel through the
stand-in for hiprtc), once more with the lanes of every lock-step interval resumed in reverse: the reduction of a test's
executions into its flag word must not depend on which lane arrives first."""
from .test_emu_suite_cpu import run_emulated

G = "test_fuzz_campaign_gpu.py::"
SELECTION = [G + "test_generated_tests_equal_the_mirror[kills-False]",
             G + "test_generated_tests_equal_the_mirror[one_pair-True]",
             G + "test_generated_tests_equal_the_mirror[waits-False]",
             G + "test_generated_tests_equal_the_mirror[stride_255-True]",
             G + "test_the_rejection_branch_of_nextint_inside_the_generator",
             G + "test_generator_refusals_by_name",
             G + "test_tests_launch_equals_the_plain_path_and_the_oracle[False-0-70-1]",
             G + "test_tests_launch_equals_the_plain_path_and_the_oracle[True-1-70-64]",
             G + "test_tests_launch_equals_the_plain_path_and_the_oracle[True-0-1-64]",
             G + "test_resident_tests_are_what_the_host_array_is",
             G + "test_a_p_max_one_below_what_one_test_needs_flags_that_test_alone",
             G + "test_wide_and_big_tables[big]",
             G + "test_a_payloads_table_is_refused_by_name",
             G + "test_campaign_equals_fuzz_driven_by_the_mirror[FullyRandom]",
             G + "test_campaign_with_executions_beyond_p_max_answers_what_fuzz_answers",
             G + "test_campaign_without_a_violation_returns_none"]


def test_fuzz_campaign_kernel_sources_on_the_cpu():
    run_emulated(SELECTION, timeout=600)


def test_the_flag_reduction_does_not_depend_on_the_order_of_the_lanes():
    run_emulated([G + "test_tests_launch_equals_the_plain_path_and_the_oracle[False-0-70-64]",
                  G + "test_tests_launch_equals_the_plain_path_and_the_oracle[False-1-70-1]",
                  G + "test_a_p_max_one_below_what_one_test_needs_flags_that_test_alone",
                  G + "test_campaign_equals_fuzz_driven_by_the_mirror[SrcDstFIFO]"],
                 lane_order="reverse", timeout=600)
