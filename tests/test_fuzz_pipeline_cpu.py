"""CPU suite of the pipelined fuzz campaign: the conditions the GPU suite's comparisons rely on, asserted on the mirror and the
oracle alone; the pipeline's bookkeeping (demi_amd/csrc/fuzz_pipeline_host.hpp) as a stand-alone program with scripted launch
outcomes under -fsanitize=address,undefined; the reduction kernels compiled for gfx950 without a GPU; the JNI shims."""
import os
import subprocess

import numpy as np
import pytest

from demi_amd import fuzzer as F, model as M, types as T

from . import fuzz_campaign_cases as FC
from . import fuzz_pipeline_cases as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMPAIGN_SEED, CAMPAIGN_EPC = 0xC0DE0000, 16        # tests/test_fuzz_campaign_gpu.py's campaign workload


@pytest.fixture(scope="module")
def campaign_verdicts():
    """the oracle's verdicts of the campaign workload's first 17 tests, at p_max 64 and 30"""
    from oracle import oracle_py as O
    O.build()
    model = M.raft_model(5)
    tests = [F.events_to_array(FC.mirror_test(FC.RAFT5, CAMPAIGN_SEED + i)) for i in range(FP.CAMPAIGN_FIRST + 1)]
    return {p: [O.random_explore(model, t, CAMPAIGN_EPC, seed_base=0, limits=T.Limits(200, 30, p, 0, 0, 0)) for t in tests] for p in (64, 30)}


def test_workload_conditions(campaign_verdicts):
    """which launch holds the first violating test for every (tests_per_launch, max_tests) of the GPU comparison"""
    viol = [bool((v["flags"] & T.V_VIOLATION).any()) for v in campaign_verdicts[64]]
    assert viol == [False] * FP.CAMPAIGN_FIRST + [True]
    assert not any((v["flags"] & FP.OVF).any() for v in campaign_verdicts[64])        # (no aborts: capacity_aborts is 0 there)
    seen = set()
    for tpl, max_tests, launch, where in FP.CAMPAIGN_CASES:
        k, launches, n_in = FP.launch_of_first(tpl, max_tests)
        assert k == launch
        if where == "none":
            assert k is None and (tpl == 1 or max_tests % tpl != 0)
        elif where == "first":
            assert k == 0
        elif where == "middle":
            assert 0 < k < launches - 1 and n_in == tpl
        else:
            assert where == "partial_last" and k == launches - 1 and 0 < n_in < tpl
        seen.add((tpl, where))
    assert {t for t, _ in seen} == {1, 3, 8, 64} and {w for _, w in seen} == {"first", "middle", "partial_last", "none"}
    assert any(w == "none" and t > 1 for t, w in seen)


def test_the_p_max_30_workload_has_an_abort_before_its_hit(campaign_verdicts):
    v = campaign_verdicts[30]
    assert any((x["flags"] & FP.OVF).any() and not (x["flags"] & T.V_VIOLATION).any() for x in v[:FP.CAMPAIGN_FIRST])


def test_the_reference_restates_the_host_loop():
    """summary_reference on planes whose answer is evident"""
    f, v = FP.plane(70, 9, hits=[40, 50], aborts=[3, 39, 41], viol_at=5, abort_at=[2, 7])
    assert FP.summary_reference(f, v)[:4] == (40, 2, 5, 1)
    f, v = FP.plane(70, 9, hits=[40], both=[12], aborts=[3, 30], viol_at=5, abort_at=[7])
    assert FP.summary_reference(f, v)[:4] == (12, 1, 5, 0) and FP.summary_reference(f, v)[4] == v[12, 5].tobytes()
    f, v = FP.plane(5, 2, aborts=[1, 4])
    assert FP.summary_reference(f, v) == (5, 2, 2, 0, bytes(16))
    f[2] |= 1
    assert FP.summary_reference(f, v) == "device"


def test_pipeline_driver_with_scripted_launch_outcomes(tmp_path):
    exe = tmp_path / "fuzz_pipeline_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "harness", "fuzz_pipeline_harness.cpp")], cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout + out.stderr      # the sanitizers report nothing
    assert out.stdout.strip() == "fuzz_pipeline_host: 208 cases ok"


def test_the_reduction_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """k_fuzz_meta_max, k_fuzz_first_hit, k_fuzz_summarise (device only, no GPU): no stack frame, no spilled register, and the few
    LDS words of the workgroup reductions"""
    from .test_jit_cpu import _meta_values
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    src = tmp_path / "fzr.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s/include/demi_gpu.h"\n#include "%s/demi_amd/csrc/k_fuzz_reduce.hpp"\n' % (ROOT, ROOT))
    obj = tmp_path / "fzr.co"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                           str(src), "-o", str(obj)], timeout=280)
    image = obj.read_bytes()
    for name in (b"k_fuzz_meta_max", b"k_fuzz_first_hit", b"k_fuzz_summarise"):
        assert name in image
    assert _meta_values(image, ".private_segment_fixed_size") == [0, 0, 0]
    assert _meta_values(image, ".vgpr_spill_count") == [0, 0, 0]
    assert _meta_values(image, ".sgpr_spill_count") == [0, 0, 0]
    assert sorted(_meta_values(image, ".group_segment_fixed_size")) == [16, 32, 56]
    assert _meta_values(image, ".wavefront_size") == [64, 64, 64]


def test_jni_shims_of_the_two_entry_points():
    import re
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "jni"), "check"])
    shim = open(os.path.join(ROOT, "jni", "demi_jni.c")).read()
    scala = open(os.path.join(ROOT, "scala", "akka", "dispatch", "verification", "gpu", "DemiGpu.scala")).read()
    for name, native in (("fuzzLaunchSummary", "demi_fuzz_launch_summary("), ("fuzzCampaignPipelined", "demi_fuzz_campaign_pipelined(")):
        assert re.search(r"FN\(%s\)\(JNIEnv" % name, shim) and re.search(r"@native def %s\(" % name, scala) and native in shim


def test_python_structs_have_the_headers_sizes():
    import ctypes as C
    assert C.sizeof(T.FuzzSummary) == 40 and C.sizeof(T.FuzzPipelineParams) == 8 and C.sizeof(T.FuzzPipelineStats) == 8
    assert T.FuzzSummary.verdict.offset == 24
    from demi_amd import _native
    L = _native.lib()
    for name in ("demi_fuzz_launch_summary", "demi_fuzz_launch_summary_row", "demi_fuzz_campaign_pipelined"):
        assert getattr(L, name).argtypes
