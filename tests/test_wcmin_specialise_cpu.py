"""Module 22 of demi_model_specialize, the wildcard round's kernel (csrc/k2_wildcard_round.hpp), without a device:
demi_specialize_check compiles it only on request (DEMI_SPECIALIZE_CHECK_ROUND), for the narrow, the wide and the real-field raft
tables, and the code object reports no private segment and no spilled vector register - the check DESIGN.md section 0.10 describes
for modules 18 and 19."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = {"narrow": "M.raft_model(5)", "wide": "M.raft_model(5, term0=1000, loglen0=300)",
          "real": "M.raft_model(5, election_budget=2, log_cap=8, real_fields=True)"}


def _check(tmp_path, knob):
    code = ("import sys, os; sys.path.insert(0, %r)\n"
            "from demi_amd import _native, model as M\n"
            "try:\n"
            "    for name, m in (%s):\n"
            "        os.environ['DEMI_JIT_DUMP'] = os.path.join(%r, name)\n"
            "        os.environ['DEMI_JIT_DUMP_SRC'] = os.path.join(%r, name + '.src')\n"
            "        print('SIZE', _native.specialize_check(m.to_struct())[0])\n"
            "except _native.DemiError as e:\n"
            "    print('ERR', e)\n" % (ROOT, ", ".join("(%r, %s)" % kv for kv in sorted(TABLES.items())), str(tmp_path), str(tmp_path)))
    env = dict(os.environ, DEMI_EXPERIMENT="1")
    for k in ("DEMI_SPECIALIZE_CHECK_K1_ONLY", "DEMI_SPECIALIZE_CHECK_TESTS", "DEMI_SPECIALIZE_CHECK_ROUND", "DEMI_JIT_FLAGS", "DEMI_JIT_DEFINES", "LD_PRELOAD"):
        env.pop(k, None)
    if knob:
        env["DEMI_SPECIALIZE_CHECK_ROUND"] = knob
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    if "hiprtc not found" in out.stdout:
        pytest.skip("no hiprtc in this environment")
    assert out.stdout.count("SIZE") == len(TABLES), out.stdout + out.stderr


def test_module_22_compiles_on_request_without_scratch_or_spills(tmp_path):
    from .test_jit_cpu import _meta_values
    _check(tmp_path, "only")
    for name in TABLES:
        image = str(tmp_path / name) + ".22"
        assert os.path.exists(image), name
        assert not os.path.exists(str(tmp_path / name) + ".18")            # ("only": just the round's module)
        assert open(str(tmp_path / name) + ".src.22").read().rstrip("\n").rsplit("\n", 1)[-1] == '#include "k2_wildcard_round.hpp"'
        image = open(image, "rb").read()
        assert b"k2_replay_wildcard_round" in image
        sizes = _meta_values(image, ".private_segment_fixed_size")
        assert sizes and all(v == 0 for v in sizes), (name, sizes)
        spills = _meta_values(image, ".vgpr_spill_count")
        assert spills and all(v == 0 for v in spills), (name, spills)


def test_without_the_knob_no_module_22(tmp_path):
    _check(tmp_path, None)
    for name in TABLES:
        assert os.path.exists(str(tmp_path / name) + ".18") and not os.path.exists(str(tmp_path / name) + ".22")
