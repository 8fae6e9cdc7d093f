"""GPU suite: K3 with wildcard entries (csrc/k3_wildcard.hpp) and testWithDpor around it (csrc/wcdpor_host.hpp) through the C ABI,
bit for bit against the transliteration of tests/wildcard_dpor_transliteration.py - verdict triple, trace entries, ignored
positions, picked-by-wildcard marks and alternative records of every interleaving; hit, interleavings and trace of every
proposal; then WildcardMinimizer(testScheduler = DPORwHeuristics) and run_the_gamut(..., "Wildcards") end to end.  No tolerance."""
import numpy as np
import pytest

from demi_amd import _native
from demi_amd import model as M
from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.incremental_ddmin import convertToDPORTrace
from demi_amd.schedulers import MinimizationStats, SchedulerConfig

from . import test_wildcard_transliteration_cpu as X
from . import wildcard_dpor_cases as K
from . import wildcard_dpor_transliteration as D

pytestmark = pytest.mark.gpu

BUDGET = 16           # dpor_budget of the pass whose interleavings are compared: at 8 no proposal's queue empties
E2E_BUDGET = 6        # ... and of the end-to-end passes: what bounds them, not a smaller trace


def _ctx(model, specialised, externals):
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if specialised or model.compiled_only:
        ctx.model_specialize()
    ctx.dpor_load(externals)
    return ctx


_REF = {}


def _raft_reference(oracle, clustering="ClockClusterizer", budget=BUDGET):
    """The transliteration's whole pass over one raft5 workload, computed once and shared."""
    if (clustering, budget) not in _REF:
        model, trace, fp = X.raft5_workload(oracle, X.WORKLOAD_SKIPS[2], **X.WORKLOAD_MODEL)
        ref = D.ScalaWildcardDporMinimizer(oracle, model, trace.original_externals, trace, fp, clusteringStrategy=clustering, dpor_budget=budget)
        _REF[(clustering, budget)] = (model, trace, fp, ref, ref.minimize())
    return _REF[(clustering, budget)]


def _interesting(ref):
    """Proposals of a pass that between them hold a first-interleaving miss, a backtracked hit, an emptied queue, a budget cut,
    interleavings with two or more points, ignored positions and an explored pair skipped."""
    picks = {}
    for k, d in enumerate(ref.tests):
        hit = bool(d.records[-1]["verdict"][0] & T.V_VIOLATION)
        for name, cond in (("backtracked", hit and len(d.records) > 1), ("emptied", d.exhausted), ("cut", d.budget_reached),
                           ("skipped", d.skipped_explored > 0), ("multi", any(len(r["alts"]) >= 2 for r in d.records)),
                           ("ignored", any(r["ignored"] for r in d.records))):
            if cond and name not in picks:
                picks[name] = k
    assert set(picks) == {"backtracked", "emptied", "cut", "skipped", "multi", "ignored"}, picks
    return sorted(set(picks.values()))


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("specialised", [False, True])
def test_batch_equals_the_transliterations_interleavings(oracle, monkeypatch, specialised, lanes):
    monkeypatch.setenv("DEMI_K3_LANES_PER_WAVE", str(lanes))
    # the hand-made table, narrow and (compiled only) wide: every strategy, two and three payloads
    # (one context per table: a specialised one compiles its modules once for all four strategies)
    for wide, n in ((False, 2), (False, 3), (True, 3)) if specialised else ((False, 2), (False, 3)):
        ctx = _ctx(K.first_writer_model(n, wide), specialised, K.first_writer_externals())
        try:
            for strategy in sorted(X.STRATEGIES):
                d, _ = K.first_writer_test(oracle, strategy, n, wide=wide)
                K.compare_launch(ctx, d, d.records, K.first_writer_selector(strategy), T.DporParams(0, n + 1, 0, 0, 64, 0, 1))
            if n == 2:
                # two Go messages: W(2) is pending twice, as two nodes with one word - LAST takes the youngest of them, not the
                # head of their fingerprint group (which is what STSScheduler's wildcard delivers)
                d, _ = K.first_writer_test(oracle, "LastOnlyStrategy", n, wide=wide, gos=2)
                assert [int(x) for x in d.records[0]["trace"]["parent"][3:]] == [2, 2, 1, 1]
                ctx.dpor_load(K.first_writer_externals(2))
                K.compare_launch(ctx, d, d.records, K.first_writer_selector("LastOnlyStrategy"), T.DporParams(0, 6, 0, 0, 64, 0, 1))
        finally:
            ctx.close()
    # raft5: the interleavings of the proposals that hold every condition of test_workload_conditions, one launch per proposal
    model, trace, fp, ref, _ = _raft_reference(oracle)
    mirror = W.ClockClusterizer(trace, model, W.BackTrackStrategy())
    ctx = _ctx(model, specialised, convertToDPORTrace(trace.original_externals, ignoreQuiescence=False))
    try:
        for k in _interesting(ref):
            d = ref.tests[k]
            par = T.DporParams(0, len(d._initialTrace), 1, fp.code, 128, 0, 1)
            K.compare_launch(ctx, d, d.records, K.selector_of(mirror), par)
    finally:
        ctx.close()


@pytest.mark.parametrize("batch", [1, 4, 64])
def test_wildcard_dpor_test_equals_testWithDpor(oracle, batch):
    """demi_wildcard_dpor_test: same hit, same `interleavings`, same trace and ignored positions, same end (exhausted / budget),
    same points and skipped pairs, whatever the width of the speculation."""
    d, hit = K.first_writer_test(oracle, "BackTrackStrategy", 3)
    ctx = _ctx(d.model, False, K.first_writer_externals())
    try:
        init = D.next_trace_entries(d, d.records[0]["next"], K.first_writer_selector("BackTrackStrategy"))
        tr, ignored, res = ctx.wildcard_dpor_test(init, T.DporParams(0, 4, 0, 0, 64, 0, 1), batch=batch)
        assert res.hit and res.interleavings == 3 and tr.tobytes() == d.records[-1]["trace"].tobytes() and ignored == []
        assert res.points == d.points and res.launches == (3 if batch == 1 else 2) and res.speculated == (0 if batch == 1 else 1)
    finally:
        ctx.close()
    model, trace, fp, ref, _ = _raft_reference(oracle)
    mirror = W.ClockClusterizer(trace, model, W.BackTrackStrategy())
    ctx = _ctx(model, True, convertToDPORTrace(trace.original_externals, ignoreQuiescence=False))
    try:
        for k in _interesting(ref):
            d = ref.tests[k]
            init = D.next_trace_entries(d, d.records[0]["next"], K.selector_of(mirror))
            tr, ignored, res = ctx.wildcard_dpor_test(init, T.DporParams(0, len(init), 1, fp.code, 128, 0, 1), dpor_budget=BUDGET, batch=batch)
            want_hit = bool(d.records[-1]["verdict"][0] & T.V_VIOLATION)
            assert bool(res.hit) == want_hit and res.interleavings == len(d.records), k
            assert (bool(res.exhausted), bool(res.budget_reached)) == (d.exhausted, d.budget_reached), k
            assert res.skipped_explored == d.skipped_explored, k
            if want_hit:
                assert tr.tobytes() == d.records[-1]["trace"].tobytes() and ignored == sorted(d.records[-1]["ignored"]), k
            if batch == 1:
                assert res.speculated == 0 and res.launches == res.interleavings
            else:
                assert res.launches <= res.interleavings
    finally:
        ctx.close()


def test_max_alts_reached_and_one_beyond(oracle):
    """The first interleaving of the three-payload table writes exactly three records: max_alts = 3 holds them, max_alts = 2 is
    one beyond - DEMI_V_ALTS_OVF, nothing silently dropped - and the capacity rule runs it again with the largest capacities."""
    d, hit = K.first_writer_test(oracle, "BackTrackStrategy", 3)
    ctx = _ctx(d.model, False, K.first_writer_externals())
    try:
        sel = K.first_writer_selector("BackTrackStrategy")
        par = T.DporParams(0, 4, 0, 0, 64, 0, 1)
        K.compare_launch(ctx, d, d.records[:1], sel, par, max_alts=3)
        init = D.next_trace_entries(d, d.records[0]["next"], sel)
        v, traces, ignored, wild, alts = ctx.dpor_wildcard_batch([init], par, max_alts=2)
        assert int(v["flags"][0]) == T.V_ALTS_OVF and len(traces[0]) == 0 and len(alts[0]) == 0
        tr, _, res = ctx.wildcard_dpor_test(init, par, batch=4, max_alts=2)
        assert res.hit and res.interleavings == 3 and res.retried == 1 and tr.tobytes() == d.records[-1]["trace"].tobytes()
        # nothing larger to run it again with: DEMI_ERR_CAPACITY, never "does not reproduce"
        with pytest.raises(_native.DemiError, match="aborted on a capacity") as e:
            ctx.wildcard_dpor_test(init, T.DporParams(0, 4, 0, 0, 128, 0, 1), max_alts=2)
        assert e.value.code == T.ERR_CAPACITY
    finally:
        ctx.close()


@pytest.mark.parametrize("budget,hit,n", [(1, False, 1), (3, True, 3), (2, False, 2)])
def test_dpor_budget_of_one_of_the_hitting_number_and_of_one_less(oracle, budget, hit, n):
    d, want = K.first_writer_test(oracle, "BackTrackStrategy", 3, dpor_budget=budget)
    assert (want is not None) == hit and len(d.records) == n
    ctx = _ctx(d.model, False, K.first_writer_externals())
    try:
        init = D.next_trace_entries(d, d.records[0]["next"], K.first_writer_selector("BackTrackStrategy"))
        for batch in (1, 4):
            tr, _, res = ctx.wildcard_dpor_test(init, T.DporParams(0, 4, 0, 0, 64, 0, 1), dpor_budget=budget, batch=batch)
            assert bool(res.hit) == hit and res.interleavings == n and bool(res.budget_reached) == (not hit) and not res.exhausted
    finally:
        ctx.close()


@pytest.mark.parametrize("clustering", ["ClockClusterizer", "SingletonClusterizer", "ClockThenSingleton"])
def test_wildcard_minimizer_over_dpor_is_the_transliterations(oracle, clustering):
    model, trace, fp, ref, want = _raft_reference(oracle, clustering, E2E_BUDGET)
    # (what the pass holds at this budget: proposals cut by it everywhere; hits, all of them in backtracked interleavings, with the
    # clock clusters - one delivery at a time nothing reproduces within six interleavings)
    assert ref.cut_by_budget > 0 and (ref.backtracked_hits > 0) == (clustering != "SingletonClusterizer")
    stats = MinimizationStats()
    m = W.WildcardMinimizer(SchedulerConfig(model=model), trace.original_externals, trace, fp, clusteringStrategy=clustering, stats=stats,
                            testScheduler=W.TestScheduler.DPORwHeuristics, dpor_budget=E2E_BUDGET, batch=16, p_max=128)
    _, got = m.minimize()
    assert len(m.proposals) == len(ref.proposals) and all((a == b).all() for a, b in zip(m.proposals, ref.proposals))
    assert stats.total_replays == ref.total_replays and m.dropped_ignored == ref.dropped_ignored
    assert len(got.events) == len(want.events) and got.events.tobytes() == want.events.tobytes()


def test_run_the_gamut_wildcards_stage(oracle):
    from demi_amd.runner_utils import run_the_gamut
    model, trace, fp, ref, want = _raft_reference(oracle, budget=E2E_BUDGET)
    out = run_the_gamut(SchedulerConfig(model=model), trace, fp, stages=("Wildcards",), p_max=128, dpor_budget=E2E_BUDGET)
    assert out["wildcard_replays"] == {"Wildcards": ref.total_replays}
    assert out["wildcard_minimized"].events.tobytes() == want.events.tobytes()


def test_refusals_by_name(oracle):
    d, _ = K.first_writer_test(oracle, "BackTrackStrategy")
    sel = K.first_writer_selector("BackTrackStrategy")
    init = D.next_trace_entries(d, d.records[0]["next"], sel)
    par = T.DporParams(0, 3, 0, 0, 64, 0, 1)
    ctx = _native.Context(0)
    try:
        ctx.model_load(d.model.to_struct())
        with pytest.raises(_native.DemiError, match="demi_dpor_load must precede demi_dpor_wildcard_batch") as e:
            ctx.dpor_wildcard_batch([init], par)
        assert e.value.code == T.ERR_NO_TRACE
        ctx.dpor_load(K.first_writer_externals())
        bad = init.copy()
        bad["key"][1] = T.wildcard_selector_key(2, 3, 0)             # no demi_wildcard_policy
        with pytest.raises(_native.DemiError, match="no entry kind or selector"):
            ctx.dpor_wildcard_batch([bad], par)
        bad = init.copy()
        bad["kind"][0] = 5
        with pytest.raises(_native.DemiError, match="no entry kind or selector"):
            ctx.wildcard_dpor_test(bad, par)
        with pytest.raises(_native.DemiError, match="more than 256 entries") as e:
            ctx.dpor_wildcard_batch([np.tile(init, 100)], par)
        assert e.value.code == T.ERR_INVALID_ARG
        with pytest.raises(_native.DemiError, match="max_alts 257 above 256"):
            ctx.dpor_wildcard_batch([init], par, max_alts=257)
        gather = _native.ALLGATHER_FN(lambda user, send, recv, nbytes: 0)
        assert _native.lib().demi_comm_create_host(ctx._h, 0, 1, gather, None) == 0
        for call in (lambda: ctx.dpor_wildcard_batch([init], par), lambda: ctx.wildcard_dpor_test(init, par)):
            with pytest.raises(_native.DemiError, match="single rank") as e:
                call()
            assert e.value.code == T.ERR_INVALID_ARG
        assert _native.lib().demi_comm_destroy(ctx._h) == 0
        K.compare_launch(ctx, d, d.records, sel, par)              # the refusals left the context usable
    finally:
        ctx.close()
    # a table of more than 8 actors
    from demi_amd.fuzzer import events_to_array, send, start
    big = M.raft_model(11)
    ctx = _native.Context(0)
    try:
        ctx.model_load(big.to_struct())
        ctx.model_specialize()
        ctx.dpor_load(events_to_array([start(a) for a in range(11)] + [send(0, M.M_BOOTSTRAP)]))
        for call in (lambda: ctx.dpor_wildcard_batch([init], par), lambda: ctx.wildcard_dpor_test(init, par)):
            with pytest.raises(_native.DemiError, match="tables of more than 8 actors are not supported") as e:
                call()
            assert e.value.code == T.ERR_INVALID_ARG
    finally:
        ctx.close()
