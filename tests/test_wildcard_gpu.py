"""GPU suite: the wildcard replay kernel (csrc/k2_wildcard.hpp) through the C ABI, bit for bit against the transliteration of
tests/test_wildcard_transliteration_cpu.py - flags, fingerprint and hash of every verdict, the kept marks and the recorded
executed trace; no tolerance anywhere.  Interpreted and specialised kernel, narrow and wide table, lanes_per_wave 1 and 64;
then WildcardMinimizer and run_the_gamut end to end, and the tie to demi_replay_removal_batch."""
import numpy as np
import pytest

from demi_amd import _native
from demi_amd import model as M
from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.apps import raft5_config2
from demi_amd.schedulers import EventTrace, MinimizationStats, SchedulerConfig, ViolationFingerprint

from . import test_wildcard_transliteration_cpu as X

pytestmark = pytest.mark.gpu

P_MAX = 128          # (the transliteration has no pending capacity: no replay below may overflow, and that is asserted)
BUDGET2 = X.WORKLOAD_MODEL          # the workloads on which wildcards are ambiguous and clock clusters go (X.test_workload_conditions)


def _ctx(model, specialised):
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if specialised or model.compiled_only:
        ctx.model_specialize()
    return ctx


def _candidates(oracle, model, trace, rng, n_random):
    """[(type_sets, policies, [present ...])]: random presence masks under every policy, plus the exact sequences both
    clusterizers propose (as the transliteration's minimizer walks them)."""
    ev = trace.events
    is_ev = ev["kind"] == T.REC_MSG_EVENT
    internal = np.array([bool(is_ev[i]) and model.msg_class[int(ev["msg_type"][i])] != T.MSG_EXTERNAL for i in range(len(ev))])
    out = []
    for policy in (T.WILDCARD_HEAD, T.WILDCARD_FIRST, T.WILDCARD_LAST):
        ts = np.where(internal, np.uint32(1) << ev["msg_type"].astype(np.uint32), 0).astype(np.uint32)
        po = np.full(len(ev), policy, dtype=np.uint8)
        presents = [np.ones(len(ev), dtype=bool)] + [~internal | (rng.random(len(ev)) < p) for p in (0.97, 0.9, 0.8) for _ in range(n_random)]
        out.append((ts, po, presents))
    for strategy, clustering in (("BackTrackStrategy", W.ClusteringStrategy.ClockClusterizer), ("LastOnlyStrategy", W.ClusteringStrategy.ClockClusterizer),
                                 ("LastOnlyStrategy", W.ClusteringStrategy.SingletonClusterizer)):
        ref = X.ScalaWildcardMinimizer(oracle, model, trace.original_externals, trace, ViolationFingerprint(0x1000103),
                                       resolutionStrategy=X.STRATEGIES[strategy][0](), clusteringStrategy=clustering)
        mirror = (W.ClockClusterizer if clustering == W.ClusteringStrategy.ClockClusterizer else W.SingletonClusterizer)(
            trace, model, X.STRATEGIES[strategy][1]())
        ts, po = mirror.selectors()
        presents, c = [], mirror
        p = c.getNextTrace(False, frozenset())
        while p is not None and len(presents) < 40:
            presents.append(p)
            p = c.getNextTrace(False, frozenset())
        out.append((ts, po, presents))
    return out


def _compare(oracle, ctx, model, trace, fp, sets, traced_every=7):
    lim = T.Limits(0, 0, P_MAX, 1, fp.code, 0, 0, 0)
    ctx.replay_load(trace.original_externals, trace.events)
    n = ambiguous = left = 0
    loaded_words = {(int(e["snd"]), int(e["rcv"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"])) for e in trace.events if int(e["kind"]) == T.REC_MSG_EVENT}
    for ts, po, presents in sets:
        ctx.replay_wildcard_load(ts, po)
        got = ctx.replay_wildcard_batch(np.array(presents), lim)
        assert not (got["flags"] & (T.V_PENDING_OVF | T.V_QUEUE_OVF)).any()
        wild = X.wildcards_of(ts, po)
        for k, present in enumerate(presents):
            v, kept, executed, ignored, s = X.run_candidate(oracle, model, trace, fp, wild, present)
            ambiguous += s.ambiguous
            left += bool({(int(e["snd"]), int(e["rcv"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"]))
                          for e in executed if int(e["kind"]) == T.REC_MSG_EVENT} - loaded_words)
            assert (int(got["flags"][k]), int(got["fingerprint"][k]), int(got["hash"][k])) == v, (k, v)
            if k % traced_every == 0:
                v1, kept1, rec1 = ctx.replay_wildcard_get_trace(present, lim)
                assert (int(v1.flags), int(v1.fingerprint), int(v1.hash)) == v
                assert (kept1 == kept).all()
                assert len(rec1) == len(executed) and rec1.tobytes() == executed.tobytes()
                assert {int(i) for i in np.nonzero((trace.events["kind"] == T.REC_MSG_EVENT) & present & (kept1 == 0))[0]} == ignored
            n += 1
    return n, ambiguous, left


@pytest.mark.parametrize("lanes", [None, 1, 64])
@pytest.mark.parametrize("specialised", [False, True])
def test_wildcard_replays_equal_the_transliteration(oracle, monkeypatch, specialised, lanes):
    if lanes is not None:
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_K2_LANES_PER_WAVE", str(lanes))
    rng = np.random.default_rng(11)
    total = ambiguous = left = 0
    for skip in X.WORKLOAD_SKIPS:
        model, trace, fp = X.raft5_workload(oracle, skip, **BUDGET2)
        ctx = _ctx(model, specialised)
        try:
            n, a, l = _compare(oracle, ctx, model, trace, fp, _candidates(oracle, model, trace, rng, 6 if lanes is None else 2))
        finally:
            ctx.close()
        total, ambiguous, left = total + n, ambiguous + a, left + l
    assert total >= (300 if lanes is None else 150) and ambiguous > 0 and left > 0


@pytest.mark.parametrize("specialised", [False, True])
def test_fault_heavy_wildcard_replays_equal_the_transliteration(oracle, specialised):
    rng = np.random.default_rng(12)
    total = 0
    for seed in (1, 2, 3):
        model, trace, fp = X.fault_heavy_workload(oracle, seed)
        ctx = _ctx(model, specialised)
        try:
            total += _compare(oracle, ctx, model, trace, fp, _candidates(oracle, model, trace, rng, 4)[:3])[0]
        finally:
            ctx.close()
    assert total >= 100


def test_wide_table_wildcard_replays_equal_the_transliteration(oracle):
    """The wide raft table of tests/test_wide_gpu.py (terms from 1000, logs from 300: payloads that need 16 bits)."""
    rng = np.random.default_rng(13)
    model = M.raft_model(5, term0=1000, loglen0=300, election_budget=2)
    assert model.wide
    _, events, lim = raft5_config2()
    trace, fp = X._verified_mcs(oracle, model, events, lim, 0)
    assert int(trace.events["p0"].max()) > 255
    ctx = _ctx(model, True)
    try:
        n, ambiguous, _ = _compare(oracle, ctx, model, trace, fp, _candidates(oracle, model, trace, rng, 4))
    finally:
        ctx.close()
    assert n >= 100 and ambiguous > 0


@pytest.mark.parametrize("specialised", [False, True])
def test_exact_selectors_are_the_removal_replay(oracle, specialised):
    """All ones and every type set 0: demi_replay_removal_batch without a removal; one cleared bit: that skip."""
    model, trace, fp = X.raft5_workload(oracle, 0)
    ev = trace.events
    ctx = _ctx(model, specialised)
    try:
        lim = T.Limits(0, 0, 64, 1, fp.code, 0, 0, 0)
        ctx.replay_load(trace.original_externals, ev)
        dels = [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]]
        skips = [0xFFFFFFFF] + dels
        want = ctx.replay_removal_batch(skips, lim)
        ctx.replay_wildcard_load(np.zeros(len(ev), dtype=np.uint32), np.zeros(len(ev), dtype=np.uint8))
        presents = np.ones((len(skips), len(ev)), dtype=bool)
        for k, i in enumerate(dels):
            presents[k + 1, i] = False
        got = ctx.replay_wildcard_batch(presents, lim)
        assert (got == want).all() and (want["flags"] & T.V_VIOLATION).any() and not (want["flags"] & T.V_VIOLATION).all()
        rng = np.random.default_rng(2)
        masks = rng.integers(0, 1 << 63, size=(len(skips), 4), dtype=np.uint64)
        assert (ctx.replay_wildcard_batch(presents, lim, masks=masks) == ctx.replay_removal_batch(skips, lim, masks=masks)).all()
        v, kept, rec = ctx.replay_wildcard_get_trace(presents[0], lim)
        v0, kept0 = ctx.replay_get_kept(len(ev), 0xFFFFFFFF, lim)
        lowered = (ev["kind"] != T.REC_MSG_SEND) | ((ev["flags"] & 1) != 0)
        assert (kept[lowered] == kept0[lowered]).all() and int(v.hash) == int(v0.hash)
        # the executed trace is loadable in turn and replays to the same verdict
        ctx.replay_load(trace.original_externals, rec)
        again = ctx.replay_removal_batch([0xFFFFFFFF], lim)[0]
        assert int(again["hash"]) == int(v.hash) and int(again["flags"]) == int(v.flags)
    finally:
        ctx.close()


def test_limits_are_refused_by_name(oracle):
    model, trace, fp = X.raft5_workload(oracle, 0)
    ctx = _ctx(model, False)
    try:
        ctx.replay_load(trace.original_externals, trace.events)
        n = len(trace.events)
        ctx.replay_wildcard_load(np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
        with pytest.raises(_native.DemiError, match="filter_known_absents"):
            ctx.replay_wildcard_batch(np.ones((1, n), dtype=bool), T.Limits(0, 0, 64, 1, fp.code, 0, 0, T.FILTER_ABSENTS_CORRECTED))
        with pytest.raises(_native.DemiError, match="policy"):
            ctx.replay_wildcard_load(np.zeros(n, dtype=np.uint32), np.full(n, 3, dtype=np.uint8))
    finally:
        ctx.close()


@pytest.mark.parametrize("clustering", [W.ClusteringStrategy.ClockClusterizer, W.ClusteringStrategy.SingletonClusterizer,
                                        W.ClusteringStrategy.ClockThenSingleton])
def test_wildcard_minimizer_on_the_gpu_is_the_transliterations(oracle, clustering):
    model, trace, fp = X.raft5_workload(oracle, X.WORKLOAD_SKIPS[0], **BUDGET2)
    ref = X.ScalaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=X.ScalaLastOnlyStrategy(),
                                   clusteringStrategy=clustering)
    want = ref.minimize()
    for max_batch in (1 << 14, 1):
        stats = MinimizationStats()
        m = W.WildcardMinimizer(SchedulerConfig(model=model), trace.original_externals, trace, fp, resolutionStrategy=W.LastOnlyStrategy(),
                                clusteringStrategy=clustering, stats=stats, max_batch=max_batch, p_max=P_MAX)
        _, got = m.minimize()
        assert stats.total_replays == ref.total_replays
        assert len(got.events) == len(want.events) and got.events.tobytes() == want.events.tobytes()
        if max_batch == 1:
            break                    # (the sequential loop once, on the shortest strategy's first pass: same numbers, many launches)


def test_the_gamut_with_wildcard_stages_ends_in_a_violating_trace(oracle):
    from demi_amd.runner_utils import run_the_gamut
    from .test_minification_cpu import _violating_execution
    model, events, lim = raft5_config2()
    model = M.raft_model(5, **BUDGET2)
    vv, rec, used = _violating_execution(oracle, model, events, lim, X.WORKLOAD_SKIPS[2])
    fp = ViolationFingerprint(vv.fingerprint)
    out = run_the_gamut(SchedulerConfig(model=model), EventTrace(rec, used), fp,
                        stages=("DDMin", "IntMin", "WildcardsNoBackTracks", "WildcardsLastOnly"), p_max=P_MAX)
    final = out["wildcard_minimized"]
    assert out["wildcard_deliveries"] <= out["minimized_deliveries"]
    ctx = _ctx(model, False)
    try:
        ctx.replay_load(final.original_externals, final.events)
        v = ctx.replay_batch(np.full((1, 4), ~np.uint64(0), dtype=np.uint64), T.Limits(0, 0, P_MAX, 1, fp.code, 0))[0]
        assert int(v["flags"]) & T.V_VIOLATION and not int(v["flags"]) & T.V_DIVERGED
    finally:
        ctx.close()
    # the default stages are what they were
    plain = run_the_gamut(SchedulerConfig(model=model), EventTrace(rec, used), fp, p_max=P_MAX)
    assert "wildcard_minimized" not in plain and plain["minimized_deliveries"] == out["minimized_deliveries"]
