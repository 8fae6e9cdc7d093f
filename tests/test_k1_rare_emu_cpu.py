"""tests/test_k1_rare_gpu.py on the CPU: the unmodified kernel sources on the wave64 emulator (tests/emu), the table interpreter
and the compiled kernels with the hints (K1_RARE) and without (DEMI_K1_NO_RARE), the lanes of every lock-step interval resumed
first to last and last to first.  TEST INFRASTRUCTURE, like tests/test_emu_suite_cpu.py: on a GPU box the same file runs on the
GPU and that run is the parity claim.  (g++ reads the hint as clang does - a statement about block order, not about values - so
what this holds is the source: k1_next_int's loop behind the first draw's test against jr_next_int's loop around it.)"""
from .test_emu_suite_cpu import run_emulated


def test_hinted_paths_against_the_oracle_on_the_cpu():
    run_emulated(["test_k1_rare_gpu.py"], timeout=1500)


def test_hinted_paths_with_the_lanes_in_reverse_order():
    run_emulated(["test_k1_rare_gpu.py"], lane_order="reverse", timeout=1500)
