"""CPU suite of the fuzz campaign: the describable message generator (fuzzer.SendGenerator, the host mirror of
csrc/k_fuzz.hpp) and the conditions the GPU suite's seed sets must contain, asserted on the mirror alone."""
import numpy as np
import pytest

from demi_amd import fuzzer as F, types as T
from demi_amd.model import M_CLIENT

from . import fuzz_campaign_cases as FC
from .limit_tables import seed_rejecting_draw


def test_send_generator_restates_raft_traces_closure():
    """generate_fuzz_test with the descriptor of raft_trace's closure is raft_trace(exact=False), event for event"""
    for n_actors, n_events, weights in ((5, 50, None), (3, 20, None), (3, 40, FC.KILLS.weights), (2, 30, FC.ONE_PAIR.weights)):
        prefix = FC.raft_prefix(n_actors)
        for seed in range(0xDE31, 0xDE31 + 150):
            want = F.raft_trace(n_actors, n_events, seed, weights=weights, exact=False)
            got = F.generate_fuzz_test(n_events - len(prefix), weights or F.FuzzerWeights(), F.raft_send_generator(), prefix, seed)
            assert got == want, (n_actors, seed)


def test_send_generator_draw_order_and_counter():
    """alternative (only when there is more than one), target, p0, p1 - and the counter restarts with every test"""
    class Rng:
        def __init__(self):
            self.asked = []

        def next_int(self, bound):
            self.asked.append(bound)
            return bound - 1

    class Alive:
        def __init__(self, rng, n):
            self.rng, self.n = rng, n

        def __len__(self):
            return self.n

        def get_random(self):
            return 10 + self.rng.next_int(self.n)

    g = F.SendGenerator([(1, F.FIXED(0), F.CONST(1), F.CONST(2)), (M_CLIENT, F.RANDOM_ALIVE, F.RANDOM(7), F.RANDOM(200))])
    r = Rng()
    assert g(r, Alive(r, 3)) == F.send(12, M_CLIENT, 6, 199) and r.asked == [2, 3, 7, 200]
    r.asked.clear()
    assert g(r, Alive(r, 0)) == F.send(0, M_CLIENT, 6, 199) and r.asked == [2, 7, 200]      # nobody alive: actor 0, no draw
    one = F.SendGenerator([(M_CLIENT, F.FIXED(2), F.COUNTER, F.COUNTER)], field_bits=8)
    r = Rng()
    out = [one(r, Alive(r, 1)) for _ in range(257)]
    assert r.asked == [] and out[0] == F.send(2, M_CLIENT, 1, 1) and out[255] == F.send(2, M_CLIENT, 0, 0) and out[256][4] == 1
    assert one(Rng(), None) == F.send(2, M_CLIENT, 1, 1)                                     # another test's generator: from 1 again
    s = g.to_struct()
    assert s.nbytes == 136 and int(s["n_alts"][0]) == 2 and int(s["alts"][0][1]["p1_arg"]) == 200
    for bad in ([], [(1, F.FIXED(0), F.CONST(256), F.CONST(0))], [(1, F.FIXED(0), F.RANDOM(0), F.CONST(0))],
                [(1, F.FIXED(0), F.RANDOM(257), F.CONST(0))], [(1, F.FIXED(0), F.CONST(0), F.CONST(0))] * 9):
        with pytest.raises(ValueError):
            F.SendGenerator(bad)


def test_thresholds_are_the_mirrors_own_sums():
    w = F.FuzzerWeights()
    total, *cum = F.fuzz_thresholds(w)
    assert total == sum([w.kill, w.send, w.partition, w.unpartition]) + w.wait_quiescence
    assert cum == [w.kill, w.kill + w.send, w.kill + w.send + w.partition, w.kill + w.send + w.partition + w.unpartition]


def test_workload_conditions():
    """what the seed sets of the GPU suite must contain, for both forms of seeding"""
    for explicit in (False, True):
        seeds = FC.explicit_seeds() if explicit else [FC.SEED_BASE + i for i in range(FC.N_TESTS)]
        # tests that end early because all nodes were killed: no postfix, no final WaitQuiescence appended
        kills = FC.mirror_tests("kills", explicit)
        early = [t for t in kills if len(t) < FC.KILLS.stride - 1 and sum(1 for e in t if e[0] == T.EV_KILL) == 3]
        assert len(early) >= 10 and any(t[-1][0] != T.EV_WAIT_QUIESCENCE for t in early)
        assert any(len(t) >= FC.KILLS.stride - 1 for t in kills)                       # ... and tests that run to the end
        # the retry on an empty partition set (one pair: a second Partition in a row has nothing to take)
        extra = 0
        for s in seeds[:60]:
            ev, doubles, _ = FC.mirror_test(FC.ONE_PAIR, s, counting=True)
            assert len(ev) == FC.ONE_PAIR.stride                                       # (nothing ends a test early here)
            extra += doubles - FC.ONE_PAIR.num_events
        assert extra >= 60
        # the WaitQuiescence retry
        extra = 0
        for s in seeds[:60]:
            ev, doubles, _ = FC.mirror_test(FC.WAITS, s, counting=True)
            assert all(not (a[0] == b[0] == T.EV_WAIT_QUIESCENCE) for a, b in zip(ev, ev[1:]))
            extra += doubles - FC.WAITS.num_events
        assert extra >= 60
        # differing lengths and batch counts
        for name, n_lengths in (("kills", 8), ("raft5", 2)):
            tests = FC.mirror_tests(name, explicit)
            assert len({len(t) for t in tests}) >= n_lengths and len({FC.n_batches(t) for t in tests}) >= 4, name
        # the prefix and the final WaitQuiescence alone
        assert all(list(t) == FC.PREFIX_ONLY.prefix + [F.wait_quiescence()] for t in FC.mirror_tests("prefix_only", explicit))
    assert FC.STRIDE_255.stride == T.MAX_EXT_EVENTS == 255 and FC.STRIDE_256.stride == 256
    assert max(len(t) for t in FC.mirror_tests("stride_255")) == 255                   # a test that fills its row
    assert FC.N_TESTS % 64 != 0


def test_a_crafted_seed_takes_nextints_rejection_branch_inside_the_generator():
    """kill weight alone, three nodes: the first event is Kill(nextInt(3)), the generator's third step (nextDouble takes two).
    The seed whose third step returns 2^31 - 1 makes that draw a rejected one."""
    cfg = FC.Config("all_kills", 3, 4, F.FuzzerWeights(kill=1.0, send=0.0, wait_quiescence=0.0, partition=0.0, unpartition=0.0))
    seed = seed_rejecting_draw(3, low=0x1234)
    ev, doubles, rejected = FC.mirror_test(cfg, seed, counting=True)
    assert rejected >= 1
    assert ev == FC.mirror_test(cfg, seed)                                              # the counting generator changes nothing
    assert [e[0] for e in ev[len(cfg.prefix):]] == [T.EV_KILL] * 3 and doubles == 4     # the fourth Kill finds nobody alive
    _, _, plain = FC.mirror_test(cfg, seed + 1, counting=True)
    assert plain == 0


def test_events_round_trip_through_the_array_form():
    for t in FC.mirror_tests("raft5")[:20]:
        assert F.array_to_events(F.events_to_array(list(t))) == list(t)
    assert np.dtype(F.SEND_GEN_DTYPE).itemsize == 136 and np.dtype(F.SEND_ALT_DTYPE).itemsize == 16


@pytest.mark.parametrize("table", ["narrow", "wide"])
def test_workgroup_per_test_modules_compile_for_gfx950_without_scratch(tmp_path, table):
    """the specialised K1 of demi_random_explore_tests (modules 20 and 21, FullyRandom and SrcDstFIFO), compiled device-free as
    demi_specialize_check compiles the others: both present, no stack frame, no spilled vector register"""
    import os
    import subprocess
    import sys
    from .test_jit_cpu import ROOT, _meta_values
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from demi_amd import _native, model as M\n"
            "m = M.raft_model(5, term0=1000, loglen0=300) if %r == 'wide' else M.raft_model(5)\n"
            "try:\n"
            "    print('CHECK', _native.specialize_check(m.to_struct()))\n"
            "except _native.DemiError as e:\n"
            "    print('ERR', e)\n" % (ROOT, table))
    env = dict(os.environ, DEMI_EXPERIMENT="1", DEMI_SPECIALIZE_CHECK_TESTS="only", DEMI_JIT_DUMP=str(tmp_path / "img"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=280)
    if "hiprtc not found" in out.stdout:
        pytest.skip("no hiprtc in this environment")
    assert "CHECK" in out.stdout and out.stdout.count("k1_random_explore") == 2, out.stdout + out.stderr[-2000:]
    for k in (20, 21):
        image = open(str(tmp_path / "img") + ".%d" % k, "rb").read()
        sizes = _meta_values(image, ".private_segment_fixed_size")
        assert sizes and all(v == 0 for v in sizes), (k, sizes)
        assert all(v == 0 for v in _meta_values(image, ".vgpr_spill_count")), k
    assert not os.path.exists(str(tmp_path / "img") + ".0")                 # ("only": just the two)


def test_the_generator_kernel_keeps_its_sets_in_lds_not_in_scratch(tmp_path):
    """k_fuzz_generate compiled for gfx950 (device only, no GPU): no stack frame, no spilled vector register, and the three
    randomized sets as 256 byte columns of 64 lanes in LDS"""
    import os
    import subprocess
    from .test_jit_cpu import ROOT, _meta_values
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    src = tmp_path / "fz.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s/include/demi_gpu.h"\n#include "%s/demi_amd/csrc/k_fuzz.hpp"\n' % (ROOT, ROOT))
    obj = tmp_path / "fz.co"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                           str(src), "-o", str(obj)], timeout=280)
    image = obj.read_bytes()
    assert b"k_fuzz_generate" in image
    assert _meta_values(image, ".private_segment_fixed_size") == [0]
    assert _meta_values(image, ".vgpr_spill_count") == [0]
    assert _meta_values(image, ".group_segment_fixed_size") == [256 * 64]
