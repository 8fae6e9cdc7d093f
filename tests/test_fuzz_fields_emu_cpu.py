"""The fuzz campaign for messages with more than two fields on the wave64 emulator (tests/emu): a selection of
tests/test_fuzz_fields_gpu.py with the kernel sources unmodified - k_fuzz_generate_fields against the mirror for three and six
fields, K1 with a workgroup per test and the tests' payload areas in both strategies, the case whose violation depends on a
field beyond the second, the resident events and areas, and the campaign - and the K1 cases once more with the lanes of a wave
emulated in reverse order (the per-test flag is a reduction over a wave's lanes)."""
from .test_emu_suite_cpu import run_emulated

G = "test_fuzz_fields_gpu.py::"


def test_field_generator_on_the_cpu():
    run_emulated([G + "test_generated_tests_and_areas_equal_the_mirror[3-False]", G + "test_generated_tests_and_areas_equal_the_mirror[3-True]",
                  G + "test_generated_tests_and_areas_equal_the_mirror[6-False]", G + "test_generated_tests_and_areas_equal_the_mirror[6-True]",
                  G + "test_generator_refusals_by_name",
                  G + "test_two_field_generator_on_the_narrow_table_gives_the_old_entry_points_bytes"])


K1 = [G + "test_tests_launch_with_areas_equals_the_plain_path_and_the_oracle[ledger-0-70]",
      G + "test_tests_launch_with_areas_equals_the_plain_path_and_the_oracle[raft_fields-1-70]",
      G + "test_tests_launch_with_areas_equals_the_plain_path_and_the_oracle[raft_fields-0-1]",
      G + "test_a_violation_that_depends_on_a_field_beyond_the_second",
      G + "test_resident_tests_and_areas_are_what_the_host_arrays_are[ledger]"]


def test_k1_tests_with_areas_and_the_campaign_on_the_cpu():
    run_emulated(K1 + [G + "test_campaign_result_and_the_found_tests_areas",
                       G + "test_campaign_equals_fuzz_driven_by_the_mirror_on_one_context"])


def test_k1_tests_with_areas_with_the_lanes_in_reverse_order():
    run_emulated(K1, lane_order="reverse")
