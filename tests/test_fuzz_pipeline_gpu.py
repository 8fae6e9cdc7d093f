"""GPU suite of the pipelined fuzz campaign: demi_fuzz_launch_summary (csrc/k_fuzz_reduce.hpp) on crafted planes against a numpy
restatement of demi_fuzz_campaign's host loop and on resident results against the copied ones, and demi_fuzz_campaign_pipelined
against the synchronous campaign field for field.  The cases and what they must contain are tests/fuzz_pipeline_cases.py's,
asserted in tests/test_fuzz_pipeline_cpu.py."""
import os

import numpy as np
import pytest

from demi_amd import _native, fuzzer as F, model as M, types as T
from demi_amd.runner_utils import fuzz_campaign
from demi_amd.schedulers import SchedulerConfig

from . import fuzz_campaign_cases as FC
from . import fuzz_fields_cases as FF
from . import fuzz_pipeline_cases as FP

pytestmark = pytest.mark.gpu
EMU = os.environ.get("DEMI_EMU") == "1"
CAMPAIGN_SEED, CAMPAIGN_EPC = 0xC0DE0000, 16        # tests/test_fuzz_campaign_gpu.py's campaign workload
LIM = T.Limits(200, 30, 64, 0, 0, 0)
SIZES = [(n, 1) for n in (1, 63, 64, 65, 255, 256, 257, 1025, 70001)] + [(65, e) for e in (63, 64, 65, 4097)]


@pytest.fixture(scope="module")
def ctxs():
    """one context per table: (raft5 | wide | big | ledger, specialised or not)"""
    made = {}

    def get(table="raft5", specialize=False):
        key = (table, specialize)
        if key not in made:
            if table == "big":
                from demi_amd.apps import raft11_config2
                model = raft11_config2()[0]
            else:
                model = {"raft5": lambda: M.raft_model(5), "wide": lambda: M.raft_model(5, term0=1000, loglen0=300), "ledger": FF.ledger_model}[table]()
            made[key] = _native.Context(0)
            made[key].model_load(model.to_struct())
            if specialize:
                made[key].model_specialize()
        return made[key]
    yield get
    for c in made.values():
        c.close()


# ------------------------------------------------------------------------------------------------ the summary on crafted planes
def _check(ctx, flags, verdicts):
    n, epc = verdicts.shape
    want = FP.summary_reference(flags, verdicts)
    if want == "device":
        with pytest.raises(_native.DemiError, match="is flagged and none of its verdicts violates") as e:
            ctx.fuzz_launch_summary(n, epc, flags, verdicts)
        assert e.value.code == T.ERR_DEVICE
        return None
    s = ctx.fuzz_launch_summary(n, epc, flags, verdicts)
    assert FP.summary_tuple(s) == want, (n, epc)
    assert s.n_events == 0 and s.reserved == 0
    return s


@pytest.mark.parametrize("n,epc", SIZES)
def test_summary_of_crafted_planes(ctxs, n, epc):
    ctx = ctxs()
    last = n - 1
    s = _check(ctx, *FP.plane(n, epc))                                           # no flag set
    assert s.first_hit == n and s.exec_index == epc and not s.capacity_aborts
    assert _check(ctx, *FP.plane(n, epc, hits=[0])).first_hit == 0               # the only hit at index 0
    assert _check(ctx, *FP.plane(n, epc, hits=[last])).first_hit == last         # ... in the last lane of the last wave
    if n > 1:
        assert _check(ctx, *FP.plane(n, epc, aborts=[0, last])).capacity_aborts == 2         # aborts and no hit: all of them count
        mid = n // 2
        # a hit with aborts below and above it, and a test with both bits below it: that one is the hit, and no abort
        s = _check(ctx, *FP.plane(n, epc, hits=[mid], aborts=[i for i in (0, mid - 1, mid + 1, last) if 0 <= i < n and i != mid]))
        assert s.first_hit == mid and s.capacity_aborts == len({i for i in (0, mid - 1) if 0 <= i < mid})
        if mid >= 2:
            s = _check(ctx, *FP.plane(n, epc, hits=[mid], aborts=[0], both=[mid - 1]))
            assert s.first_hit == mid - 1 and s.capacity_aborts == (1 if mid - 1 > 0 else 0)
    if n > 256:
        # hits in two different workgroups (and, at 70 001, in two passes of the grid): the lower one wins
        for lo, hi in ((200, 300), (255, 256), (n - 300, n - 1), (n // 2, n - 1)):
            if not 2 <= lo < hi < n:
                continue
            s = _check(ctx, *FP.plane(n, epc, hits=[lo, hi], aborts=[lo - 1, hi - 1 if hi - 1 != lo else lo - 2]))
            assert s.first_hit == lo
    # the first violating execution at k, aborted executions before it and only behind it
    for k in sorted({0, 63, 64, epc - 1} & set(range(epc))):
        s = _check(ctx, *FP.plane(n, epc, hits=[last], viol_at=k))
        assert s.exec_index == k and not s.aborted_before
        if k > 0:
            for at in sorted({0, k - 1}):
                assert _check(ctx, *FP.plane(n, epc, hits=[last], viol_at=k, abort_at=[at])).aborted_before == 1
        if k + 2 < epc:
            s = _check(ctx, *FP.plane(n, epc, hits=[last], viol_at=k, abort_at=[k + 1]))
            assert s.exec_index == k and not s.aborted_before
    # a flagged row without a violating verdict
    flags, v = FP.plane(n, epc, aborts=[0])
    flags[last] |= 1
    assert _check(ctx, flags, v) is None


def test_summary_refusals(ctxs):
    ctx = ctxs()
    flags, v = FP.plane(4, 2)
    for kw in (dict(flags=flags), dict(verdicts=v)):
        with pytest.raises(_native.DemiError, match="given together") as e:
            ctx.fuzz_launch_summary(4, 2, **kw)
        assert e.value.code == T.ERR_INVALID_ARG
    with pytest.raises(_native.DemiError, match="65536 executions") as e:
        ctx.fuzz_launch_summary(1, 65537)
    assert e.value.code == T.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ resident results
@pytest.mark.parametrize("specialize", [False, True])
@pytest.mark.parametrize("strategy", [T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO])
def test_summary_of_resident_results_equals_the_summary_of_copied_results(ctxs, strategy, specialize):
    ctx = ctxs("raft5", specialize)
    cfg = FC.RAFT5
    n, epc = (70, 16) if not EMU else (20, 4)
    lim = FC.k1_limits(strategy)
    ctx.fuzz_generate(n, cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed_base=FC.SEED_BASE, copy_out=False)
    with pytest.raises(_native.DemiError) as e:                      # generated, not explored: no results are resident
        ctx.fuzz_launch_summary(n, epc)
    assert e.value.code == T.ERR_NO_TRACE
    ev, n_ev, _ = ctx.fuzz_generate(n, cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed_base=FC.SEED_BASE)
    v, f = ctx.random_explore_tests(None, epc, lim, seed_base=FC.K1_SEED_BASE, n_tests=n)
    s, row, areas = ctx.fuzz_launch_summary(n, epc, row=True)
    want = FP.summary_reference(f, v)
    assert want != "device" and want[0] < n                          # (the workload holds a violating test)
    assert FP.summary_tuple(s) == want
    assert s.n_events == n_ev[s.first_hit] and row.tobytes() == ev[s.first_hit, :s.n_events].tobytes() and not areas.any()
    # the same arrays uploaded: the same record but for the length
    up = ctx.fuzz_launch_summary(n, epc, f, v)
    assert FP.summary_tuple(up) == want and up.n_events == 0
    assert FP.summary_tuple(ctx.fuzz_launch_summary(n, epc)) == want            # (still resident: a summary changes nothing)
    # another launch of the context writes the verdict plane: the results are no longer the test launch's
    ctx.trace_load(ev[0, :n_ev[0]])
    ctx.random_explore(8, lim, seed_base=1)
    with pytest.raises(_native.DemiError) as e:
        ctx.fuzz_launch_summary(n, epc)
    assert e.value.code == T.ERR_NO_TRACE


def test_summary_of_resident_results_with_payload_areas(ctxs):
    ctx = ctxs("ledger", True)
    n, epc = 12, FF.CAMPAIGN_EPC
    ev, ar, n_ev, _ = ctx.fuzz_generate(n, FF.CAMPAIGN_NUM_EVENTS, FF.CAMPAIGN_WEIGHTS, FF.campaign_gen(), FF.CAMPAIGN_PREFIX, seed_base=FF.CAMPAIGN_SEED)
    v, f = ctx.random_explore_tests(None, epc, FF.campaign_limits(), seed_base=0, n_tests=n, with_areas=True)
    s, row, areas = ctx.fuzz_launch_summary(n, epc, row=True)
    assert FP.summary_tuple(s) == FP.summary_reference(f, v) and (s.first_hit, s.exec_index) == (FF.CAMPAIGN_TEST, FF.CAMPAIGN_EXEC)
    assert row.tobytes() == ev[s.first_hit, :s.n_events].tobytes() and areas.tobytes() == ar[s.first_hit, :s.n_events].tobytes() and areas.any()


# ------------------------------------------------------------------------------------------------ the pipelined campaign
def _raft_args(cfg=FC.RAFT5):
    return (cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix)


def _equal(sync, piped):
    assert len(sync) == len(piped) and bytes(sync[0]) == bytes(piped[0])
    for a, b in zip(sync[1:], piped[1:]):
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())


def _stats_ok(ctx, res, in_flight):
    st = ctx.fuzz_pipeline_stats
    assert st.launches_submitted - st.launches_discarded == res.launches
    assert st.launches_discarded <= in_flight - 1
    return int(st.launches_discarded)


CASES = FP.CAMPAIGN_CASES if not EMU else [c for c in FP.CAMPAIGN_CASES if c[:2] in ((8, 20), (3, 17), (64, 13))]


@pytest.mark.parametrize("tpl,max_tests,launch,where", CASES)
@pytest.mark.parametrize("strategy", [T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO])
def test_pipelined_campaign_equals_the_synchronous_one(ctxs, strategy, tpl, max_tests, launch, where):
    ctx = ctxs()
    lim = T.Limits(200, 30, 64, 0, 0, 0, strategy)
    kw = dict(executions_per_test=CAMPAIGN_EPC, tests_per_launch=tpl, max_tests=max_tests, test_seed_base=CAMPAIGN_SEED)
    sync = ctx.fuzz_campaign(*_raft_args(), lim, **kw)
    if strategy == T.STRATEGY_FULLY_RANDOM:
        assert (sync[0].found, sync[0].launches) == ((1, launch + 1) if launch is not None else (0, -(-max_tests // tpl)))
        assert not sync[0].found or sync[0].test_index == FP.CAMPAIGN_FIRST
    discarded = []
    for in_flight in (1, 2, 3):
        piped = ctx.fuzz_campaign(*_raft_args(), lim, in_flight=in_flight, **kw)
        _equal(sync, piped)
        discarded.append(_stats_ok(ctx, piped[0], in_flight))
    assert discarded[0] == 0
    if strategy == T.STRATEGY_FULLY_RANDOM and where == "middle":      # (the positions are FullyRandom's: test_fuzz_pipeline_cpu.py)
        assert discarded[1:] == [1, 2]                                # (launches behind the one with the hit were in flight)
    if (strategy == T.STRATEGY_FULLY_RANDOM and where == "partial_last") or not sync[0].found:
        assert discarded == [0, 0, 0]


def test_in_flight_zero_is_two(ctxs):
    ctx = ctxs()
    kw = dict(executions_per_test=CAMPAIGN_EPC, tests_per_launch=8, max_tests=40, test_seed_base=CAMPAIGN_SEED)
    _equal(ctx.fuzz_campaign(*_raft_args(), LIM, **kw), ctx.fuzz_campaign(*_raft_args(), LIM, in_flight=0, **kw))
    assert (ctx.fuzz_pipeline_stats.launches_submitted, ctx.fuzz_pipeline_stats.launches_discarded) == (4, 1)


@pytest.mark.parametrize("table", ["raft5", "wide", "big"])
def test_pipelined_campaign_through_the_compiled_tables(ctxs, table):
    """the specialised raft table, one wide and one BIG table: whatever the synchronous campaign finds"""
    ctx = ctxs(table, True)
    if table == "big":
        from demi_amd.apps import raft11_config2
        lim, n_actors = raft11_config2()[2], 11
    else:
        lim, n_actors = LIM, 5
    cfg = FC.RAFT5 if table == "raft5" else FC.Config(table, n_actors, 24, F.FuzzerWeights(kill=0.05))
    kw = dict(executions_per_test=CAMPAIGN_EPC if not EMU else 4, tests_per_launch=8 if not EMU else 3, max_tests=40 if not EMU else 7,
              test_seed_base=CAMPAIGN_SEED)
    sync = ctx.fuzz_campaign(*_raft_args(cfg), lim, **kw)
    for in_flight in (1, 2, 3):
        _equal(sync, ctx.fuzz_campaign(*_raft_args(cfg), lim, in_flight=in_flight, **kw))
        _stats_ok(ctx, sync[0], in_flight)


def test_pipelined_campaign_with_payload_areas(ctxs):
    ctx = ctxs("ledger", True)
    args = (FF.CAMPAIGN_NUM_EVENTS, FF.CAMPAIGN_WEIGHTS, FF.campaign_gen(), FF.CAMPAIGN_PREFIX)
    for strategy in (T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO):
        for tpl, max_tests in ((4, 12), (2, 12), (4, 4)):
            kw = dict(executions_per_test=FF.CAMPAIGN_EPC, tests_per_launch=tpl, max_tests=max_tests, test_seed_base=FF.CAMPAIGN_SEED)
            sync = ctx.fuzz_campaign(*args, FF.campaign_limits(strategy), **kw)
            assert len(sync) == 3 and (max_tests == 4 or (sync[0].found and sync[2].any()))
            for in_flight in (1, 2, 3):
                _equal(sync, ctx.fuzz_campaign(*args, FF.campaign_limits(strategy), in_flight=in_flight, **kw))
                _stats_ok(ctx, sync[0], in_flight)


# ------------------------------------------------------------------------------------------------ executions beyond p_max
def test_executions_beyond_p_max(ctxs):
    """the p_max = 30 workload of test_campaign_with_executions_beyond_p_max_answers_what_fuzz_answers"""
    ctx = ctxs()
    lim = T.Limits(200, 30, 30, 0, 0, 0)
    for max_tests in (16, 24):
        kw = dict(executions_per_test=CAMPAIGN_EPC, tests_per_launch=8, max_tests=max_tests, test_seed_base=CAMPAIGN_SEED)
        sync = ctx.fuzz_campaign(*_raft_args(), lim, **kw)
        assert sync[0].capacity_aborts > 0
        for in_flight in (1, 2, 3):
            piped = ctx.fuzz_campaign(*_raft_args(), lim, in_flight=in_flight, **kw)
            _equal(sync, piped)
            assert piped[0].capacity_aborts == sync[0].capacity_aborts
    sc = SchedulerConfig(model=M.raft_model(5))
    kw = dict(maxMessages=200, invariant_check_interval=30, executions_per_test=CAMPAIGN_EPC, max_tests=24, tests_per_launch=8,
              test_seed_base=CAMPAIGN_SEED, p_max=30, provenance_device=None)
    want = fuzz_campaign(_raft_args(), sc, **kw)
    got = fuzz_campaign(_raft_args(), sc, in_flight=2, **kw)
    assert want is not None and got is not None
    (t1, v1, i1, f1), (t2, v2, i2, f2) = want, got
    assert t1.events.tobytes() == t2.events.tobytes() and t1.original_externals.tobytes() == t2.original_externals.tobytes()
    assert v1 == v2 and i1.tobytes() == i2.tobytes() and f1.tobytes() == f2.tobytes()


# ------------------------------------------------------------------------------------------------ the context afterwards
def test_the_context_after_a_campaign_that_discarded_launches():
    cfg = FC.RAFT5
    kw = dict(executions_per_test=CAMPAIGN_EPC, tests_per_launch=3 if not EMU else 8, max_tests=40, test_seed_base=CAMPAIGN_SEED)
    test0 = F.events_to_array(FC.mirror_test(cfg, CAMPAIGN_SEED))

    def answers(ctx, in_flight):
        out = [ctx.fuzz_campaign(*_raft_args(), LIM, **kw)]
        ctx.trace_load(test0)
        out.append(ctx.random_explore(64, LIM, seed_base=7))
        out.append(ctx.fuzz_campaign(*_raft_args(), LIM, in_flight=in_flight, **kw))
        return out

    fresh = _native.Context(0)
    used = _native.Context(0)
    try:
        for c in (fresh, used):
            c.model_load(M.raft_model(5).to_struct())
        first = used.fuzz_campaign(*_raft_args(), LIM, in_flight=3, **kw)
        assert first[0].found and used.fuzz_pipeline_stats.launches_discarded == 2
        want, got = answers(fresh, 2), answers(used, 2)
        _equal(want[0], got[0])
        assert want[1].tobytes() == got[1].tobytes()
        _equal(want[2], got[2])
        _equal(first, got[2])
        # no resident tests are left behind
        with pytest.raises(_native.DemiError) as e:
            used.random_explore_tests(None, 4, LIM, n_tests=1)
        assert e.value.code == T.ERR_NO_TRACE
        # an output that is too small: the length by name, every launch waited for, and the context still works
        with pytest.raises(_native.DemiError, match=r"the violating test has %d events, the buffer holds 5" % first[0].n_events) as e:
            used.fuzz_campaign(*_raft_args(), LIM, in_flight=3, cap=5, **kw)
        assert e.value.code == T.ERR_CAPACITY
        with pytest.raises(_native.DemiError, match=r"the violating test has %d events, the buffer holds 5" % first[0].n_events):
            used.fuzz_campaign(*_raft_args(), LIM, cap=5, **kw)                  # (the synchronous one: the same words)
        _equal(first, used.fuzz_campaign(*_raft_args(), LIM, in_flight=3, **kw))
        used.trace_load(test0)
        assert used.random_explore(64, LIM, seed_base=7).tobytes() == want[1].tobytes()
    finally:
        fresh.close()
        used.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctxs):
    import ctypes as C
    ctx = ctxs()
    kw = dict(executions_per_test=4, tests_per_launch=4, max_tests=4)
    with pytest.raises(_native.DemiError, match="in_flight 4") as e:
        ctx.fuzz_campaign(*_raft_args(), LIM, in_flight=4, **kw)
    assert e.value.code == T.ERR_INVALID_ARG
    # null pointers
    L = _native.lib()
    par, keep = ctx.fuzz_params(*_raft_args(), ())
    cp, pp, res = T.FuzzCampaignParams(max_tests=4), T.FuzzPipelineParams(), T.FuzzCampaignResult()
    ev = np.zeros(T.MAX_EXT_EVENTS, dtype=T.EXT_EVENT_DTYPE)
    for a in ((None, C.byref(cp), C.byref(pp), C.byref(res)), (C.byref(par), None, C.byref(pp), C.byref(res)),
              (C.byref(par), C.byref(cp), None, C.byref(res)), (C.byref(par), C.byref(cp), C.byref(pp), None)):
        rc = L.demi_fuzz_campaign_pipelined(ctx._h, a[0], None, a[1], a[2], C.byref(LIM), ev.ctypes.data, None, T.MAX_EXT_EVENTS, a[3], None)
        assert rc == T.ERR_INVALID_ARG and "null pointer" in L.demi_last_error(ctx._h).decode()
    rc = L.demi_fuzz_campaign_pipelined(ctx._h, C.byref(par), None, C.byref(cp), C.byref(pp), C.byref(LIM), None, None, 4, C.byref(res), None)
    assert rc == T.ERR_INVALID_ARG and "null output" in L.demi_last_error(ctx._h).decode()
    assert L.demi_fuzz_launch_summary(ctx._h, None, None, 4, 4, None) == T.ERR_INVALID_ARG
    # what the synchronous entry points refuse, in their words: a stride beyond the boundary, per-instance executions, a
    # DEMI_MODEL_PAYLOADS table through the two-field generator
    big = FC.STRIDE_256
    msgs = []
    pay = _native.Context(0)
    pay.model_load(M.raft_model(5, log_cap=8, real_fields=True).to_struct())
    for in_flight in (None, 2):
        with pytest.raises(_native.DemiError) as e:
            ctx.fuzz_campaign(big.num_events, big.weights, big.gen(), big.prefix, LIM, in_flight=in_flight, **kw)
        msgs.append(str(e.value))
        with pytest.raises(_native.DemiError) as e:
            ctx.fuzz_campaign(*_raft_args(), T.Limits(200, 30, 64, 0, 0, 0, 0, 0, 4), in_flight=in_flight, **kw)
        msgs.append(str(e.value))
        with pytest.raises(_native.DemiError) as e:
            pay.fuzz_campaign(*_raft_args(), LIM, in_flight=in_flight, **kw)
        msgs.append(str(e.value))
    pay.close()
    assert msgs[:3] == msgs[3:] and "DEMI_MAX_EXT_EVENTS" in msgs[0] and "executions_per_instance" in msgs[1] and "DEMI_MODEL_PAYLOADS" in msgs[2]
    del keep
