"""The native internal-minimization loop (demi_amd/csrc/intmin_host.hpp: OneAtATimeStrategy, LeftToRightOneAtATime,
SrcDstFIFORemoval, STSSchedMinimizer.minimize) without a GPU and without the emulator: a stand-alone program
(tests/harness/intmin_host_harness.cpp) answers its rounds with the CPU oracle's removal replay, is built with
-fsanitize=address,undefined and run as a child process; nothing is loaded into this interpreter.  Its trace, replay count,
record_internal_size sequence and round sizes are held against the Python sequential loop / the Python mirror at the same
max_batch over the same oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

from demi_amd import types as T
from demi_amd.apps import raft5_config2
from demi_amd.internal_minimization import LeftToRightOneAtATime, SrcDstFIFORemoval, STSSchedMinimizer

from .test_internal_min_cpu import OracleRemoval, _verified_mcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRATEGIES = {"LeftToRight": (LeftToRightOneAtATime, T.REMOVAL_LEFT_TO_RIGHT), "SrcDstFIFO": (SrcDstFIFORemoval, T.REMOVAL_SRC_DST_FIFO)}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    from oracle import oracle_py
    oracle_py.build()
    exe = tmp_path_factory.mktemp("intmin_harness") / "intmin_host_harness"
    build = os.path.join(ROOT, "oracle", "_build")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "harness", "intmin_host_harness.cpp"),
                           "-L" + build, "-loracle", "-Wl,-rpath," + build, "-pthread"], cwd=ROOT)
    return str(exe)


@pytest.fixture(scope="module")
def workloads(oracle):
    """skip -> (model, verified MCS execution, fingerprint), computed once."""
    model, events, lim = raft5_config2()
    return {skip: (model,) + _verified_mcs(oracle, model, events, lim, skip) for skip in (0, 1, 2)}


def write_case(path, model, trace, fp, strategy, max_batch):
    ext = np.ascontiguousarray(trace.original_externals, dtype=T.EXT_EVENT_DTYPE)
    rec = T.rec_events(trace.events)
    flags = model.to_struct().flags
    with open(path, "wb") as f:
        f.write(struct.pack("<6I", 0x31484D49, strategy, max_batch, fp.code, len(ext), len(rec)))
        f.write(struct.pack("<11I", model.n_actors, model.n_msg_types, model.n_classes, len(model.code), model.inv_kind, model.inv_fa,
                            model.inv_va, model.inv_fb, model.fp_match_mask, flags, len(model.init_state)))
        f.write(np.asarray(model.msg_class, dtype=np.uint8).tobytes())
        f.write(np.asarray(model.actor_class, dtype=np.uint8).tobytes())
        f.write(np.asarray(model.handler_start, dtype="<u2").tobytes())
        f.write(np.asarray(model.code, dtype="<u4").tobytes())
        f.write(np.asarray(model.init_state, dtype="<u8").tobytes())
        f.write(ext.tobytes())
        f.write(rec.tobytes())


def read_result(path):
    raw = open(path, "rb").read()
    status, n_trace, n_sizes, n_batches, unignorable, adoptions, total = struct.unpack_from("<6IQ", raw, 0)
    off = struct.calcsize("<6IQ")
    trace = np.frombuffer(raw, dtype=T.REC_EVENT_DTYPE, count=n_trace, offset=off)
    off += n_trace * T.REC_EVENT_DTYPE.itemsize
    sizes = np.frombuffer(raw, dtype="<u4", count=n_sizes, offset=off).tolist()
    off += 4 * n_sizes
    batches = np.frombuffer(raw, dtype="<u4", count=n_batches, offset=off).tolist()
    assert off + 4 * n_batches == len(raw)
    return dict(status=np.int32(np.uint32(status)).item(), trace=trace, sizes=sizes, batches=batches, unignorable=unignorable,
                adoptions=adoptions, total_replays=total)


@pytest.mark.parametrize("max_batch", [1, 7, 0])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
@pytest.mark.parametrize("skip", [0, 1, 2])
def test_native_loop_equals_the_python_sequential_loop(oracle, harness, workloads, tmp_path, skip, strategy, max_batch):
    model, trace, fp = workloads[skip]
    cls, code = STRATEGIES[strategy]
    mcs = trace.original_externals
    seq = STSSchedMinimizer(mcs, trace, fp, cls(trace, model), OracleRemoval(oracle, model), max_batch=1)
    s1, t1 = seq.minimize()
    mirror = STSSchedMinimizer(mcs, trace, fp, cls(trace, model), OracleRemoval(oracle, model), max_batch=max_batch or (1 << 14))
    mirror.minimize()
    write_case(tmp_path / "case.bin", model, trace, fp, code, max_batch)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([harness, str(tmp_path / "case.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr.strip(), out.stdout + out.stderr      # the sanitizers report nothing
    got = read_result(tmp_path / "out.bin")
    assert got["status"] == 0
    assert got["trace"].tobytes() == T.rec_events(t1.events).tobytes()
    assert got["total_replays"] == s1.total_replays
    assert got["sizes"] == seq.internal_sizes
    assert got["unignorable"] == cls(trace, model).unignorable
    assert got["batches"] == mirror.batches
    assert got["adoptions"] > 0 and len(got["trace"]) < len(trace.events)
