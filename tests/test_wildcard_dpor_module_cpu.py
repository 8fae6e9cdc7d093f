"""The specialised K3 with wildcard entries (module 23, csrc/k3_wildcard.hpp) compiled device-free for gfx950, as
demi_specialize_check compiles the other modules: present on request only, no stack frame, no spilled vector register."""
import os
import subprocess
import sys

import pytest

from .test_jit_cpu import ROOT, _meta_values


def _check(table, env_extra, tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from demi_amd import _native, model as M\n"
            "m = M.raft_model(5, term0=1000, loglen0=300) if %r == 'wide' else M.raft_model(5)\n"
            "try:\n"
            "    print('CHECK', _native.specialize_check(m.to_struct()))\n"
            "except _native.DemiError as e:\n"
            "    print('ERR', e)\n" % (ROOT, table))
    env = dict(os.environ, DEMI_EXPERIMENT="1", DEMI_JIT_DUMP=str(tmp_path / "img"), **env_extra)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=280)


@pytest.mark.parametrize("table", ["narrow", "wide"])
def test_wildcard_dpor_module_compiles_for_gfx950_without_scratch(tmp_path, table):
    out = _check(table, {"DEMI_SPECIALIZE_CHECK_K3W": "only"}, tmp_path)
    if "hiprtc not found" in out.stdout:
        pytest.skip("no hiprtc in this environment")
    assert "CHECK" in out.stdout and out.stdout.count("k3_dpor_wild") == 1, out.stdout + out.stderr[-2000:]
    image = open(str(tmp_path / "img") + ".23", "rb").read()
    sizes = _meta_values(image, ".private_segment_fixed_size")
    assert sizes and all(v == 0 for v in sizes), sizes
    assert b"12k3_dpor_wildE" in image and b"7k3_dporE" not in image      # (k3_dpor itself is not part of the module)
    assert all(v == 0 for v in _meta_values(image, ".vgpr_spill_count"))
    assert not os.path.exists(str(tmp_path / "img") + ".0") and not os.path.exists(str(tmp_path / "img") + ".2")      # ("only": just it)


def test_the_default_check_keeps_its_set_of_modules(tmp_path):
    """Without the environment value demi_specialize_check compiles what it compiled before: no module 23."""
    out = _check("narrow", {"DEMI_SPECIALIZE_CHECK_K1_ONLY": "1"}, tmp_path)
    if "hiprtc not found" in out.stdout:
        pytest.skip("no hiprtc in this environment")
    assert "CHECK" in out.stdout and "k3_dpor_wild" not in out.stdout, out.stdout + out.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "img") + ".23")
