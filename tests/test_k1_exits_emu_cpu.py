"""tests/test_k1_exits_gpu.py on the CPU: the unmodified kernel sources on the wave64 emulator (tests/emu), the table interpreter
and the compiled kernels, with the lanes of every lock-step interval resumed first to last and last to first.  TEST
INFRASTRUCTURE, like tests/test_emu_suite_cpu.py: on a GPU box the same file runs on the GPU and that run is the parity claim."""
from .test_emu_suite_cpu import run_emulated


def test_exit_paths_against_the_oracle_on_the_cpu():
    run_emulated(["test_k1_exits_gpu.py"], timeout=900)


def test_exit_paths_with_the_lanes_in_reverse_order():
    run_emulated(["test_k1_exits_gpu.py"], lane_order="reverse", timeout=900)
