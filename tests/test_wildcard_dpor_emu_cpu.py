"""A selection of tests/test_wildcard_dpor_gpu.py on the CPU, against the UNMODIFIED kernel source (tests/emu: csrc/k3_wildcard.hpp
compiled with g++ on the lock-step wave64 emulator, the specialised kernel through the stand-in for hiprtc), once more with the
lanes of every lock-step interval resumed in reverse.  Without a GPU this is the only execution of the kernel."""
from .test_emu_suite_cpu import run_emulated

F = "test_wildcard_dpor_gpu.py::"
SELECTION = [F + "test_batch_equals_the_transliterations_interleavings[False-64]",
             F + "test_batch_equals_the_transliterations_interleavings[True-1]",
             F + "test_wildcard_dpor_test_equals_testWithDpor[1]",
             F + "test_wildcard_dpor_test_equals_testWithDpor[4]",
             F + "test_max_alts_reached_and_one_beyond",
             F + "test_dpor_budget_of_one_of_the_hitting_number_and_of_one_less[3-True-3]",
             F + "test_dpor_budget_of_one_of_the_hitting_number_and_of_one_less[2-False-2]",
             F + "test_wildcard_minimizer_over_dpor_is_the_transliterations[ClockClusterizer]",
             F + "test_refusals_by_name"]


def test_wildcard_dpor_kernel_source_against_the_transliteration_on_the_cpu():
    run_emulated(SELECTION, timeout=280)


def test_wildcard_dpor_results_do_not_depend_on_the_order_of_the_lanes():
    run_emulated([F + "test_batch_equals_the_transliterations_interleavings[False-64]",
                  F + "test_wildcard_dpor_test_equals_testWithDpor[64]"], lane_order="reverse", timeout=280)
