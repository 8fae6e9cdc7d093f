"""The capacity rule and the first-hit round of the replay path (demi_amd/csrc/replay_host.hpp) without a GPU and without the
emulator: a stand-alone program (tests/harness/replay_host_harness.cpp) drives both templates with scripted answers - for the
round: no proposals, width 1, a hit in the first and in the last chunk, an abort after / before / without a hit, an abort that
stays, a capacity that is already the largest, each with its exact launches and retried; for the batch: nothing undecided, some
undecided, still undecided, already the largest.  It is built with -fsanitize=address,undefined and run as a child process;
nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capacity_rule_and_first_hit_round_with_scripted_answers(tmp_path):
    exe = tmp_path / "replay_host_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "harness", "replay_host_harness.cpp")], cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout + out.stderr      # the sanitizers report nothing
    assert out.stdout.strip() == "replay_host: 20 cases ok"
