"""A selection of tests/test_wildcard_ddmin_gpu.py on the CPU, against the UNMODIFIED kernel source (tests/emu: the candidates
launch of csrc/k2_wildcard_cand.hpp compiled with g++ on the lock-step wave64 emulator, the specialised kernel through the
stand-in for hiprtc), once more with the lanes of every lock-step interval resumed in reverse: the reduction of a candidate's
proposals on the device must not depend on which lane arrives first."""
from .test_emu_suite_cpu import run_emulated

SELECTION = ["test_wildcard_ddmin_gpu.py::test_candidates_launch_equals_the_transliteration[False-64]",
             "test_wildcard_ddmin_gpu.py::test_candidates_launch_equals_the_transliteration[True-1]",
             "test_wildcard_ddmin_gpu.py::test_native_wildcard_ddmin_equals_the_mirror_and_the_transliteration[6-LastOnlyStrategy]",
             "test_wildcard_ddmin_gpu.py::test_a_capacity_before_the_first_hit_is_unknown_and_evaluated_again",
             "test_wildcard_ddmin_gpu.py::test_a_capacity_that_stays_is_an_error_by_name",
             "test_wildcard_ddmin_gpu.py::test_refusals_by_name"]


def test_candidates_kernel_source_against_the_transliteration_on_the_cpu():
    run_emulated(SELECTION, timeout=280)


def test_the_reduction_does_not_depend_on_the_order_of_the_lanes():
    run_emulated(["test_wildcard_ddmin_gpu.py::test_candidates_launch_equals_the_transliteration[False-64]",
                  "test_wildcard_ddmin_gpu.py::test_native_wildcard_ddmin_equals_the_mirror_and_the_transliteration[12-BackTrackStrategy]"],
                 lane_order="reverse", timeout=280)
