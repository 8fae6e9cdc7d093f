"""tests/test_replay_pipeline_gpu.py on the CPU: demi_replay_batch_submit / _wait over the unmodified kernel sources on the wave64
emulator (tests/emu) - the narrow-table parity at the wave edges (interpreted and compiled, the three filterKnownAbsents
settings), three calls in flight, the neighbours of outstanding tickets and the tickets' refusals; three in flight once more with
the lanes of every lock-step interval resumed last to first.  TEST INFRASTRUCTURE, like tests/test_emu_suite_cpu.py: the
emulator's streams run in order of submission, so the overlap itself is the GPU run's claim."""
from .test_emu_suite_cpu import run_emulated

F = "test_replay_pipeline_gpu.py::"


def test_replay_tickets_against_the_oracle_on_the_cpu():
    run_emulated([F + "test_parity_at_the_wave_edges", F + "test_three_in_flight", F + "test_neighbours_of_outstanding_tickets",
                  F + "test_tickets_name_their_kind_and_are_single_use"], timeout=900)


def test_three_in_flight_with_the_lanes_in_reverse_order():
    run_emulated([F + "test_three_in_flight"], lane_order="reverse", timeout=900)
