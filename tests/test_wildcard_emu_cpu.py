"""A selection of tests/test_wildcard_gpu.py on the CPU, against the UNMODIFIED kernel source (tests/emu: csrc/k2_wildcard.hpp
compiled with g++ on the lock-step wave64 emulator, the specialised kernel through the stand-in for hiprtc), once more with the
lanes of every lock-step interval resumed in reverse.  Without a GPU this is the only execution of the wildcard kernel."""
from .test_emu_suite_cpu import run_emulated

SELECTION = ["test_wildcard_gpu.py::test_exact_selectors_are_the_removal_replay",
             "test_wildcard_gpu.py::test_wildcard_replays_equal_the_transliteration[False-64]",
             "test_wildcard_gpu.py::test_wildcard_replays_equal_the_transliteration[True-1]",
             "test_wildcard_gpu.py::test_limits_are_refused_by_name",
             "test_wildcard_gpu.py::test_wildcard_minimizer_on_the_gpu_is_the_transliterations[ClockThenSingleton]"]


def test_wildcard_kernel_source_against_the_transliteration_on_the_cpu():
    run_emulated(SELECTION, timeout=280)


def test_wildcard_results_do_not_depend_on_the_order_of_the_lanes():
    run_emulated(["test_wildcard_gpu.py::test_wildcard_replays_equal_the_transliteration[False-64]",
                  "test_wildcard_gpu.py::test_fault_heavy_wildcard_replays_equal_the_transliteration[False]"], lane_order="reverse", timeout=280)
