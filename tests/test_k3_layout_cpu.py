"""The staging-area layouts of the K3 host path (demi_amd/csrc/k3_layout.hpp) without a GPU and without the emulator: a stand-alone
program (tests/harness/k3_layout_harness.cpp) calls every layout function at the shapes of tests/harness/k3_layout_expected.inc -
n in {1, 63, 64, 1025}, max_pairs in {0, 1, 64, 4096}, one to three ranks, 0 / 1 / 300 deltas, fetches of 1 / FETCH_INLINE_IDS /
FETCH_INLINE_IDS + 1 ids, staging areas of 1 / Q_TILE / Q_TILE + 1 / 2^21 points - and asserts that each is a sound carving (ordered,
no overlap, aligned fields aligned, packed fields adjacent, total covering the last) whose offsets EQUAL the literals there: those
were printed by the offset chains demi_gpu.hip spelled out at nine places before the header existed.  It is built with
-fsanitize=address,undefined and run as a child process; nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_staging_area_is_carved_as_it_was():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "k3_layout_harness")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", exe, os.path.join(ROOT, "tests", "harness", "k3_layout_harness.cpp")], cwd=ROOT)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        env.pop("LD_PRELOAD", None)
        out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout + out.stderr      # the sanitizers report nothing
    assert out.stdout.strip() == "k3_layout: 187 cases ok"
