"""tests/test_k1_fx_commute_gpu.py on the CPU: the unmodified kernel sources on the wave64 emulator (tests/emu), the table
interpreter and the compiled kernels, with the lanes of every lock-step interval resumed first to last and last to first.  TEST
INFRASTRUCTURE, like tests/test_emu_suite_cpu.py: on a GPU box the same file runs on the GPU and that run is the parity claim."""
import pytest

from .test_emu_suite_cpu import run_emulated


def test_reordered_deliveries_against_the_oracle_on_the_cpu():
    run_emulated(["test_k1_fx_commute_gpu.py"], timeout=900)


def test_reordered_deliveries_with_the_lanes_in_reverse_order():
    run_emulated(["test_k1_fx_commute_gpu.py"], lane_order="reverse", timeout=900)


def test_the_overflow_matrix_notices_a_dropped_moved_bit():
    """Broken on purpose (DEMI_K1_FX_DROP_MOVED: the apply phase takes no row for moved, so the queue overflow of the moved TSET ends
    the pass before the BCAST the program runs first): the case whose Kick is [BCAST, TSET RT] with the queue at its capacity and
    a BCAST that overflows p_max must then report the queue flag where the oracle reports the pending flag - and fail.  The
    case whose BCAST fits passes either way."""
    broken = {"DEMI_EXPERIMENT": "1", "DEMI_JIT_DEFINES": "DEMI_K1_FX_DROP_MOVED=1"}
    case = "test_k1_fx_commute_gpu.py::test_reordered_deliveries_equal_the_oracle[%s-compiled]"
    run_emulated([case % "matrix-k5-q8-p12"], extra_env=broken, timeout=600)
    with pytest.raises(AssertionError, match="verdicts differ"):
        run_emulated([case % "matrix-k5-q8-p11"], extra_env=broken, timeout=600)
    run_emulated([case % "matrix-k5-q8-p11"], timeout=600)
