"""The native wildcard-minimization loop (demi_amd/csrc/wcmin_host.hpp: the Clusterizers, WildcardMinimizer.minimize / doMinimize)
without a GPU and without the emulator: a stand-alone program (tests/harness/wcmin_host_harness.cpp), built with
-fsanitize=address,undefined and run as a child process; nothing sanitized is loaded into this interpreter.  There is no C wildcard
oracle, so the Python mirror W.WildcardMinimizer runs over the transliterated device at the same max_batch, every presence row it
asks for is written down with its answer (tests/wcmin_cases.py), and the harness answers the native loop's rounds from that file -
a row that is not in it fails the case.  Held equal to the mirror: the returned trace byte for byte, total_replays, the
internal_sizes sequence, the round sizes and the adoptions."""
import os
import subprocess

import pytest

from demi_amd import types as T

from . import wcmin_cases as Wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wcmin_harness") / "wcmin_host_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "harness", "wcmin_host_harness.cpp")], cwd=ROOT)
    return str(exe)


def run_case(harness, tmp_path, oracle, name, clustering, policy, skip_clock, max_batch):
    model, trace, fp, _ = Wc.workload(oracle, name)
    want = Wc.mirror(oracle, name, clustering, policy, skip_clock, max_batch)
    Wc.write_case(tmp_path / "case.bin", model, trace, Wc.params_of(model, clustering, policy, skip_clock, max_batch), want["segments"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([harness, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout + out.stderr      # the sanitizers report nothing
    got = Wc.read_result(tmp_path / "out.bin")
    assert got["status"] == 0
    assert got["trace"].tobytes() == want["trace"].tobytes()
    assert got["total_replays"] == want["total_replays"]
    assert got["sizes"] == want["internal_sizes"]
    assert got["batches"] == want["batches"] and got["rounds"] == len(want["batches"])
    assert got["adoptions"] == want["adoptions"]
    return got, want


@pytest.mark.parametrize("max_batch", [1, 7, 0])
@pytest.mark.parametrize("skip_clock", [0, 1])
@pytest.mark.parametrize("policy", sorted(Wc.POLICIES))
@pytest.mark.parametrize("clustering", sorted(Wc.CLUSTERINGS))
@pytest.mark.parametrize("name", ["narrow0", "narrow1", "real3"])
def test_native_loop_equals_the_python_mirror(oracle, harness, tmp_path, name, clustering, policy, skip_clock, max_batch):
    run_case(harness, tmp_path, oracle, name, clustering, policy, skip_clock, max_batch)


def test_the_cases_reach_what_they_are_there_for(oracle, harness, tmp_path):
    """What the comparison above rests on, asserted on the mirror's own runs: a minimization with more than one adoption (the
    native loop fetches the trace once per pass, for the last row that satisfied the length rule), a Singleton pass over a trace
    that is not the start trace, and a result shorter than the loaded execution."""
    two_adoptions = shrinks = second_pass_differs = False
    for name in ("narrow0", "narrow1", "real3"):
        model, trace, fp, _ = Wc.workload(oracle, name)
        want = Wc.mirror(oracle, name, "ClockThenSingleton", "LAST", 0, 0)
        two_adoptions |= want["adoptions"] >= 2
        shrinks |= len(want["trace"]) < len(trace.events)
        second_pass_differs |= len(want["segments"]) == 2 and want["segments"][1]["trace"].tobytes() != T.rec_events(trace.events).tobytes()
    assert two_adoptions and shrinks and second_pass_differs
