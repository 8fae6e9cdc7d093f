"""A selection of tests/test_wildcard_payloads_gpu.py and tests/test_dpor_areas_gpu.py on the CPU, against the UNMODIFIED kernel
sources (tests/emu: the wildcard kernels compiled for the DEMI_MODEL_PAYLOADS / DEMI_MODEL_ARRAY tables through the stand-in
for hiprtc, on the lock-step wave64 emulator - which also aborts a launch that writes behind its dynamic LDS), once more with
the lanes of every lock-step interval resumed in reverse."""
from .test_emu_suite_cpu import run_emulated

SELECTION = ["test_wildcard_payloads_gpu.py::test_wildcard_replays_equal_the_transliteration[real5-None]",
             "test_wildcard_payloads_gpu.py::test_wildcard_replays_equal_the_transliteration[real3-64]",
             "test_wildcard_payloads_gpu.py::test_wildcard_replays_equal_the_transliteration[array5-1]",
             "test_wildcard_payloads_gpu.py::test_exact_selectors_are_the_removal_replay[True]",
             "test_wildcard_payloads_gpu.py::test_candidates_launch_and_native_ddmin_equal_the_transliteration",
             "test_wildcard_payloads_gpu.py::test_the_gamut_runs_every_stage_on_a_trace_with_ext_areas",
             "test_wildcard_payloads_gpu.py::test_refusals_by_name",
             "test_dpor_areas_gpu.py"]


def test_payload_wildcard_kernels_and_dpor_areas_on_the_cpu():
    run_emulated(SELECTION, timeout=600)


def test_payload_wildcard_results_do_not_depend_on_the_order_of_the_lanes():
    run_emulated(["test_wildcard_payloads_gpu.py::test_wildcard_replays_equal_the_transliteration[real3-64]",
                  "test_wildcard_payloads_gpu.py::test_wildcard_replays_equal_the_transliteration[array5-None]",
                  "test_wildcard_payloads_gpu.py::test_candidates_launch_and_native_ddmin_equal_the_transliteration"],
                 lane_order="reverse", timeout=600)
