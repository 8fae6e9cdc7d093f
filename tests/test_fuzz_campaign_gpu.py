"""GPU suite of the fuzz campaign: k_fuzz_generate against the host mirror byte for byte, K1 with a workgroup per test against
the plain path (trace_load + random_explore per test) and the CPU oracle, and the campaign against fuzz() driven by the mirror.
The seed sets and what they must contain are tests/fuzz_campaign_cases.py's, asserted in tests/test_fuzz_campaign_cpu.py."""
import os

import numpy as np
import pytest

from demi_amd import _native, fuzzer as F, model as M, types as T
from demi_amd.runner_utils import fuzz, fuzz_campaign
from demi_amd.schedulers import FullyRandom, ReplayScheduler, SchedulerConfig, SrcDstFIFO

from . import fuzz_campaign_cases as FC
from .limit_tables import seed_rejecting_draw

pytestmark = pytest.mark.gpu
EMU = os.environ.get("DEMI_EMU") == "1"
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF


@pytest.fixture(scope="module")
def ctxs():
    """one context per cluster size, the raft table loaded"""
    made = {}

    def get(n_actors):
        if n_actors not in made:
            made[n_actors] = _native.Context(0)
            made[n_actors].model_load(M.raft_model(n_actors).to_struct())
        return made[n_actors]
    yield get
    for c in made.values():
        c.close()


def _packed(tests, stride):
    out = np.zeros((len(tests), stride), dtype=T.EXT_EVENT_DTYPE)
    for i, t in enumerate(tests):
        out[i, :len(t)] = F.events_to_array(list(t))
    return out


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("name", [c.name for c in FC.CONFIGS])
def test_generated_tests_equal_the_mirror(ctxs, name, explicit):
    cfg = {c.name: c for c in FC.CONFIGS}[name]
    want = FC.mirror_tests(name, explicit)
    ev, n_ev, n_b = ctxs(cfg.n_actors).fuzz_generate(FC.N_TESTS, cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, cfg.postfix,
                                                     seed_base=FC.SEED_BASE, seeds=FC.explicit_seeds() if explicit else None)
    assert ev.shape == (FC.N_TESTS, cfg.stride)
    assert n_ev.tolist() == [len(t) for t in want]
    assert n_b.tolist() == [FC.n_batches(t) for t in want]
    assert ev.tobytes() == _packed(want, cfg.stride).tobytes()           # the tail of every row is zero


def test_the_rejection_branch_of_nextint_inside_the_generator(ctxs):
    cfg = FC.Config("all_kills", 3, 4, F.FuzzerWeights(kill=1.0, send=0.0, wait_quiescence=0.0, partition=0.0, unpartition=0.0))
    seeds = [seed_rejecting_draw(3, low=0x1234), seed_rejecting_draw(3, low=0x1234) + 1, seed_rejecting_draw(5, low=7)]
    assert FC.mirror_test(cfg, seeds[0], counting=True)[2] >= 1                 # (the mirror asserts that the retry happens)
    ev, n_ev, _ = ctxs(3).fuzz_generate(len(seeds), cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seeds=seeds)
    for i, s in enumerate(seeds):
        want = FC.mirror_test(cfg, s)
        assert F.array_to_events(ev[i, :n_ev[i]]) == want and len(want) == 9


def test_generator_refusals_by_name(ctxs):
    ctx, c = ctxs(5), FC.STRIDE_256

    def refused(what, *a, **kw):
        with pytest.raises(_native.DemiError) as e:
            ctx.fuzz_generate(*a, **kw)
        assert what in str(e.value), str(e.value)
    refused("DEMI_MAX_EXT_EVENTS", 4, c.num_events, c.weights, c.gen(), c.prefix)                    # 256 events: one too many
    ok = FC.STRIDE_255
    assert ctx.fuzz_generate(2, ok.num_events, ok.weights, ok.gen(), ok.prefix)[0].shape == (2, 255)
    refused("without a Start", 4, 10, F.FuzzerWeights(), FC.raft_gen(), [F.send(0, M.M_BOOTSTRAP)])
    refused("without a Start", 4, 10, F.FuzzerWeights(), FC.raft_gen(), [])
    refused("all zero", 4, 10, F.FuzzerWeights(0.0, 0.0, 0.0, 0.0, 0.0), FC.raft_gen(), FC.raft_prefix(5))
    refused("Start()ed twice", 4, 10, F.FuzzerWeights(), FC.raft_gen(), FC.raft_prefix(5) + [F.start(2)])
    refused("actor out of range", 4, 10, F.FuzzerWeights(), FC.raft_gen(), [F.start(5)])
    refused("non-external", 4, 10, F.FuzzerWeights(), F.SendGenerator([(M.M_CLIENT + 1, F.RANDOM_ALIVE, F.COUNTER, F.CONST(0))]), FC.raft_prefix(5))
    refused("target out of range", 4, 10, F.FuzzerWeights(), F.SendGenerator([(M.M_CLIENT, F.FIXED(5), F.COUNTER, F.CONST(0))]), FC.raft_prefix(5))
    refused("field_bits", 4, 10, F.FuzzerWeights(), F.SendGenerator([(M.M_CLIENT, F.FIXED(0), F.COUNTER, F.CONST(0))], field_bits=16), FC.raft_prefix(5))
    # weights under which the generator's redraws would never end are refused, never launched: WaitQuiescence alone (the second
    # one is drawn again forever), Partition without UnPartition (the pairs run out), partitions with a single node (no pair)
    W = F.FuzzerWeights
    for w, prefix in ((W(0.0, 0.0, 1.0, 0.0, 0.0), FC.raft_prefix(5)), (W(0.0, 0.0, 0.1, 0.5, 0.0), FC.raft_prefix(5)),
                      (W(0.0, 0.0, 0.1, 0.0, 0.5), FC.raft_prefix(5)), (W(0.0, 0.0, 0.1, 0.5, 0.5), [F.start(0)]),
                      (W(0.0, 1e-9, 1.0, 0.0, 0.0), FC.raft_prefix(5))):
        refused("DEMI_FUZZ_MIN_PROGRESS", 4, 10, w, FC.raft_gen(), prefix)
        with pytest.raises(_native.DemiError) as e:
            ctx.fuzz_campaign(10, w, FC.raft_gen(), prefix, FC.k1_limits(), max_tests=4)
        assert "DEMI_FUZZ_MIN_PROGRESS" in str(e.value)
    # ... and the neighbouring weights that do make progress are taken: both partition weights with two nodes or more, Kill alone,
    # nothing to generate at all
    for w, n in ((W(0.0, 0.0, 0.1, 0.5, 0.5), 10), (W(0.5, 0.0, 0.5, 0.0, 0.0), 10), (W(0.0, 0.0, 1.0, 0.0, 0.0), 0)):
        cfg = FC.Config("edge", 5, n, w)
        ev, n_ev, _ = ctx.fuzz_generate(8, n, w, cfg.gen(), cfg.prefix, seed_base=FC.SEED_BASE)
        for i in range(8):
            assert F.array_to_events(ev[i, :n_ev[i]]) == FC.mirror_test(cfg, FC.SEED_BASE + i)
    with pytest.raises(_native.DemiError) as e:
        ctx.random_explore_tests(None, 4, FC.k1_limits(), n_tests=1 << 19)
    assert "resident tests" in str(e.value)
    with pytest.raises(ValueError):
        ctx.random_explore_tests(np.zeros((2, 4), dtype=T.EXT_EVENT_DTYPE), 4, FC.k1_limits())        # no n_ev


# ------------------------------------------------------------------------------------------------ K1 with a workgroup per test
_plain = {}


def _plain_path(ctx, specialize, strategy, epc, tests, lim):
    """trace_load + random_explore per test, once per variant"""
    key = (specialize, strategy, epc, lim.p_max, len(tests))
    if key not in _plain:
        out = []
        for ev in tests:
            ctx.trace_load(ev)
            out.append(ctx.random_explore(epc, lim, seed_base=FC.K1_SEED_BASE))
        _plain[key] = out
    return _plain[key]


@pytest.fixture(scope="module")
def raft5_ctx():
    made = {}

    def get(specialize):
        if specialize not in made:
            made[specialize] = _native.Context(0)
            made[specialize].model_load(M.raft_model(5).to_struct())
            if specialize:
                made[specialize].model_specialize()
        return made[specialize]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("epc", [1, 70])
@pytest.mark.parametrize("strategy", [T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO])
@pytest.mark.parametrize("specialize", [False, True])
def test_tests_launch_equals_the_plain_path_and_the_oracle(raft5_ctx, monkeypatch, specialize, strategy, epc, lanes):
    n = 37 if not EMU else 9
    tests = FC.k1_tests()[:n] if not EMU else FC.k1_tests()[::4][:n]
    if EMU:
        epc = min(epc, 66)
    lim = FC.k1_limits(strategy)
    ctx = raft5_ctx(specialize)
    if EMU:
        from oracle import oracle_py as O
        want = [O.random_explore(M.raft_model(5), ev, epc, seed_base=FC.K1_SEED_BASE, limits=lim) for ev in tests]
    else:
        want = FC.k1_oracle(strategy, epc)
    plain = _plain_path(ctx, specialize, strategy, epc, tests, lim)
    monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", str(lanes))
    v, f = ctx.random_explore_tests(list(tests), epc, lim, seed_base=FC.K1_SEED_BASE)
    monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE")
    assert v.shape == (len(tests), epc) and len({len(t) for t in tests}) >= 5
    for i in range(len(tests)):
        assert v[i].tobytes() == plain[i].tobytes() == want[i].tobytes(), i
        assert int(f[i]) == (1 if (want[i]["flags"] & T.V_VIOLATION).any() else 0) | (2 if (want[i]["flags"] & OVF).any() else 0), i
    if not EMU:
        assert 0 < int((f & 1).sum()) < len(tests)                      # violating and clean tests
    assert not (f & 2).any()


@pytest.mark.parametrize("specialize", [False, True])
def test_more_executions_per_test_than_a_workgroup_holds(raft5_ctx, monkeypatch, specialize):
    """epc = 300: with full waves (64 lanes) a test is two workgroups, the second with 44 of its 256 lanes at work; with the lanes
    per wave the launch picks itself, as many workgroups as 300 executions need at that width."""
    epc = 300 if not EMU else 70
    tests = [FC.k1_tests()[i] for i in (0, 16, 32)]
    lim = FC.k1_limits()
    ctx = raft5_ctx(specialize)
    plain = _plain_path(ctx, specialize, "epc300", epc, tests, lim)
    for lanes in (None, 64) if not EMU else (16,):
        if lanes:
            monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", str(lanes))
        v, f = ctx.random_explore_tests(tests, epc, lim, seed_base=FC.K1_SEED_BASE)
        assert v.shape == (3, epc)
        for i in range(3):
            assert v[i].tobytes() == plain[i].tobytes(), (lanes, i)
            assert int(f[i]) == (1 if (plain[i]["flags"] & T.V_VIOLATION).any() else 0) | (2 if (plain[i]["flags"] & OVF).any() else 0), (lanes, i)


def test_resident_tests_are_what_the_host_array_is(raft5_ctx):
    """tests = NULL: the generated tests in the context, explored without ever leaving the device"""
    cfg, n, epc = FC.K1_KILLS5, 21 if not EMU else 5, 20
    ctx = raft5_ctx(False)
    ev, n_ev, _ = ctx.fuzz_generate(n, cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed_base=FC.SEED_BASE)
    v, f = ctx.random_explore_tests(None, epc, FC.k1_limits(), seed_base=FC.K1_SEED_BASE, n_tests=n)
    v2, f2 = ctx.random_explore_tests(ev, epc, FC.k1_limits(), seed_base=FC.K1_SEED_BASE, n_ev=n_ev)
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()
    ctx.trace_load(ev[3, :n_ev[3]])
    assert v[3].tobytes() == ctx.random_explore(epc, FC.k1_limits(), seed_base=FC.K1_SEED_BASE).tobytes()


def test_a_p_max_one_below_what_one_test_needs_flags_that_test_alone(raft5_ctx, oracle):
    tests, epc = FC.k1_tests(), 70
    model = M.raft_model(5)

    def aborted(i, p_max):
        return bool((oracle.random_explore(model, tests[i], epc, seed_base=FC.K1_SEED_BASE, limits=FC.k1_limits(p_max=p_max))["flags"] & OVF).any())
    # (chosen with the oracle) test 32 needs 43 pending slots, every other test fewer than 43
    assert aborted(32, 42) and not aborted(32, 43) and not any(aborted(i, 42) for i in range(len(tests)) if i != 32)
    pick = list(range(26, 37)) if not EMU else [31, 32, 33]
    v, f = raft5_ctx(False).random_explore_tests([tests[i] for i in pick], epc, FC.k1_limits(p_max=42), seed_base=FC.K1_SEED_BASE)
    assert [bool(x & 2) for x in f] == [i == 32 for i in pick]
    for k, i in enumerate(pick):
        assert v[k].tobytes() == oracle.random_explore(model, tests[i], epc, seed_base=FC.K1_SEED_BASE, limits=FC.k1_limits(p_max=42)).tobytes()
    _, f = raft5_ctx(False).random_explore_tests([tests[32]], epc, FC.k1_limits(p_max=43), seed_base=FC.K1_SEED_BASE)
    assert not f[0] & 2


@pytest.mark.parametrize("table", ["wide", "big"])
def test_wide_and_big_tables(oracle, table):
    """a smaller case each for the layouts that run only as compiled tables"""
    if table == "wide":
        model, n_actors, lim = M.raft_model(5, term0=1000, loglen0=300), 5, T.Limits(200, 30, 64, 0, 0, 0)
    else:
        from demi_amd.apps import raft11_config2
        model, _, lim = raft11_config2()
        n_actors = 11
    cfg = FC.Config(table, n_actors, 24, F.FuzzerWeights(kill=0.05))
    n, epc = (6, 40) if not EMU else (3, 8)
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        ctx.model_specialize()
        ev, n_ev, n_b = ctx.fuzz_generate(n, cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed_base=FC.SEED_BASE)
        v, f = ctx.random_explore_tests(None, epc, lim, seed_base=FC.K1_SEED_BASE, n_tests=n)
        for i in range(n):
            mirror = FC.mirror_test(cfg, FC.SEED_BASE + i)
            assert F.array_to_events(ev[i, :n_ev[i]]) == mirror
            want = oracle.random_explore(model, ev[i, :n_ev[i]], epc, seed_base=FC.K1_SEED_BASE, limits=lim)
            assert v[i].tobytes() == want.tobytes(), i
            ctx.trace_load(ev[i, :n_ev[i]])
            assert v[i].tobytes() == ctx.random_explore(epc, lim, seed_base=FC.K1_SEED_BASE).tobytes()
            assert int(f[i]) == (1 if (want["flags"] & T.V_VIOLATION).any() else 0) | (2 if (want["flags"] & OVF).any() else 0)
    finally:
        ctx.close()


def test_a_payloads_table_is_refused_by_name():
    model = M.raft_model(5, log_cap=8, real_fields=True)
    assert model.to_struct().flags >> 16 & 7 > 2                          # DEMI_MODEL_PAYLOADS
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        with pytest.raises(_native.DemiError) as e:
            ctx.random_explore_tests([FC.k1_tests()[0]], 4, FC.k1_limits())
        assert "DEMI_MODEL_PAYLOADS" in str(e.value)
        with pytest.raises(_native.DemiError) as e:
            ctx.fuzz_campaign(10, F.FuzzerWeights(), FC.raft_gen(), FC.raft_prefix(5), FC.k1_limits(), max_tests=4)
        assert "DEMI_MODEL_PAYLOADS" in str(e.value)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the campaign
CAMPAIGN_SEED = 0xC0DE0000      # chosen with the mirror and the oracle: under 16 executions per test (seeds 0 .. 15) tests 0 .. 15
CAMPAIGN_EPC = 16               # of RAFT5 are clean, test 16 violates first in execution 4, test 21 in execution 7


def _same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    (t1, v1, i1, f1), (t2, v2, i2, f2) = a, b
    assert t1.events.tobytes() == t2.events.tobytes() and t1.original_externals.tobytes() == t2.original_externals.tobytes()
    assert v1 == v2 and i1.tobytes() == i2.tobytes() and f1.tobytes() == f2.tobytes()


@pytest.mark.parametrize("strategy_ctor", [FullyRandom, SrcDstFIFO])
def test_campaign_equals_fuzz_driven_by_the_mirror(oracle, strategy_ctor):
    cfg = FC.RAFT5
    model = M.raft_model(5)
    sc = SchedulerConfig(model=model)
    gen = lambda i: F.events_to_array(FC.mirror_test(cfg, CAMPAIGN_SEED + i))
    args = (cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix)
    kw = dict(maxMessages=200, invariant_check_interval=30, randomizationStrategyCtor=strategy_ctor, validate_replay=lambda: ReplayScheduler(sc))
    max_tests = 40 if not EMU else 24
    want = fuzz(gen, sc, executions_per_test=CAMPAIGN_EPC, max_tests=max_tests, provenance_device=0, **kw)
    got = fuzz_campaign(args, sc, executions_per_test=CAMPAIGN_EPC, max_tests=max_tests, tests_per_launch=8, test_seed_base=CAMPAIGN_SEED, **kw)
    assert want is not None
    _same(got, want)
    if strategy_ctor is FullyRandom:
        # the first violating test lies beyond the first launch of 8 tests
        lim = T.Limits(200, 30, 64, 0, 0, 0)
        first = [bool((oracle.random_explore(model, gen(i), CAMPAIGN_EPC, seed_base=0, limits=lim)["flags"] & T.V_VIOLATION).any()) for i in range(17)]
        assert first == [False] * 16 + [True]
        assert got[0].original_externals.tobytes() == gen(16)[:len(got[0].original_externals)].tobytes()
        ctx = _native.Context(0)
        ctx.model_load(model.to_struct())
        res, ev = ctx.fuzz_campaign(*args, lim, executions_per_test=CAMPAIGN_EPC, tests_per_launch=8, max_tests=max_tests, test_seed_base=CAMPAIGN_SEED)
        assert (res.found, res.test_index, res.exec_index, res.launches, res.tests_run, res.capacity_aborts) == (1, 16, 4, 3, 24, 0)
        assert ev.tobytes() == gen(16).tobytes()
        ctx.close()
        # a filter that rejects the first violation sends both drivers on to the next violating test
        seen = []

        def second(fp):
            seen.append(fp)
            return len(seen) != 1
        want2 = fuzz(gen, sc, executions_per_test=CAMPAIGN_EPC, max_tests=max_tests, provenance_device=0, violationWereLookingFor=second, **kw)
        seen.clear()
        got2 = fuzz_campaign(args, sc, executions_per_test=CAMPAIGN_EPC, max_tests=max_tests, tests_per_launch=8, test_seed_base=CAMPAIGN_SEED,
                             violationWereLookingFor=second, **kw)
        _same(got2, want2)
        assert got2[0].original_externals.tobytes() != got[0].original_externals.tobytes()


def test_campaign_with_executions_beyond_p_max_answers_what_fuzz_answers(oracle):
    """p_max 30: most tests have executions that overflow it (no verdict).  fuzz() decides each such execution alone with the
    largest pending set; the campaign goes on with the largest pending set from the first such test.  Same four values."""
    from demi_amd.schedulers import CapacityExceeded, RandomScheduler
    cfg = FC.RAFT5
    model = M.raft_model(5)
    sc = SchedulerConfig(model=model)
    gen = lambda i: F.events_to_array(FC.mirror_test(cfg, CAMPAIGN_SEED + i))
    lim = T.Limits(200, 30, 30, 0, 0, 0)
    assert any((oracle.random_explore(model, gen(i), CAMPAIGN_EPC, seed_base=0, limits=lim)["flags"] & OVF).any() for i in range(16))
    kw = dict(maxMessages=200, invariant_check_interval=30, executions_per_test=CAMPAIGN_EPC, max_tests=24)
    want = fuzz(gen, sc, provenance_device=0, scheduler_ctor=lambda *a, **k: RandomScheduler(*a, p_max=30, **k), **kw)
    got = fuzz_campaign((cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix), sc, tests_per_launch=8, test_seed_base=CAMPAIGN_SEED, p_max=30, **kw)
    assert want is not None
    _same(got, want)
    assert got[0].original_externals.tobytes() == gen(16)[:len(got[0].original_externals)].tobytes()
    # the device's own report of it
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    res, _ = ctx.fuzz_campaign(cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, lim, executions_per_test=CAMPAIGN_EPC, tests_per_launch=8,
                               max_tests=16, test_seed_base=CAMPAIGN_SEED)
    assert not res.found and res.capacity_aborts > 0
    ctx.close()
    # beyond the largest pending set there is no answer: both drivers say so
    tiny = FC.Config("flood", 5, 200, F.FuzzerWeights(kill=0.0, send=1.0, wait_quiescence=0.0, partition=0.0, unpartition=0.0))
    with pytest.raises(CapacityExceeded):
        fuzz_campaign((tiny.num_events, tiny.weights, tiny.gen(), tiny.prefix), sc, tests_per_launch=4, test_seed_base=1, maxMessages=0,
                      invariant_check_interval=0, executions_per_test=4, max_tests=4)


def test_campaign_without_a_violation_returns_none():
    cfg = FC.RAFT5
    sc = SchedulerConfig(model=M.raft_model(5))
    gen = lambda i: F.events_to_array(FC.mirror_test(cfg, CAMPAIGN_SEED + i))
    kw = dict(maxMessages=200, invariant_check_interval=30, executions_per_test=CAMPAIGN_EPC, max_tests=12)
    assert fuzz(gen, sc, **kw) is None
    assert fuzz_campaign((cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix), sc, tests_per_launch=8, test_seed_base=CAMPAIGN_SEED, **kw) is None
