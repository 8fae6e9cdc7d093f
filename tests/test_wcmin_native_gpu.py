"""demi_replay_wildcard_round and demi_minimize_wildcards through the C ABI: one round of WildcardMinimizer.doMinimize reduced on
the device (csrc/k2_wildcard_round.hpp) against the existing pair demi_replay_wildcard_batch / demi_replay_wildcard_get_trace, and
the whole loop (csrc/wcmin_host.hpp) against the Python mirror over the transliterated device and the transliterated Scala
minimizers.  Every comparison is for equality."""
import numpy as np
import pytest

from demi_amd import _native, types as T
from demi_amd import model as M
from demi_amd import wildcard_minimization as W
from demi_amd.internal_minimization import countMsgEvents
from demi_amd.schedulers import EventTrace, MinimizationStats, SchedulerConfig

from . import test_wildcard_transliteration_cpu as X
from . import wcmin_cases as Wc
from . import wildcard_payload_cases as Pc

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NO_SKIP = 0xFFFFFFFF
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
P_MAX = Pc.P_MAX
COMPILED_ONLY = {"real3", "array5"}
_cache = {}


def limits(fp, p_max=P_MAX):
    return T.Limits(0, 0, p_max, 1, fp.code, 0, 0, 0)


def context(oracle, name, specialised):
    """One context per (workload, flavour) for the whole module: the table is compiled once."""
    if ("ctx", name, specialised) not in _cache:
        model = Wc.workload(oracle, name)[0]
        ctx = _native.Context(0)
        ctx.model_load(model.to_struct())
        if specialised:
            ctx.model_specialize()
            assert ctx.is_specialized()
        _cache["ctx", name, specialised] = ctx
    return _cache["ctx", name, specialised]


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
    yield
    for key in [k for k in _cache if k[0] == "ctx"]:
        _cache.pop(key).close()


# ------------------------------------------------------------------ 1. a round against the existing pair
def _pool(oracle, name):
    """(selectors, presence rows): the real proposal sequences of the mirror's clusterizers over the workload - each assuming
    the one before it failed, and the ClockClusterizer's as the mirror's own run walks it, adoptions fed back - and random rows."""
    if ("pool", name) not in _cache:
        model, trace, fp, _ = Wc.workload(oracle, name)
        ev = trace.events
        clock = W.ClockClusterizer(trace, model, W.LastOnlyStrategy())
        rows = []
        for c in (clock, W.SingletonClusterizer(trace, model, W.LastOnlyStrategy())):
            p = c.getNextTrace(False, frozenset())
            while p is not None and len(rows) < 200:
                rows.append(p)
                p = c.getNextTrace(False, frozenset())
        first_pass = Wc.mirror(oracle, name, "ClockClusterizer", "LAST", 0, 0)["segments"][0]
        assert (first_pass["type_sets"] == clock.selectors()[0]).all() and (first_pass["policies"] == clock.selectors()[1]).all()
        rows += [r["present"] for r in first_pass["rows"].values()]
        is_ev = ev["kind"] == T.REC_MSG_EVENT
        internal = np.array([bool(is_ev[i]) and model.msg_class[int(ev["msg_type"][i])] != T.MSG_EXTERNAL for i in range(len(ev))])
        rng = np.random.default_rng(17)
        rows += [~internal | (rng.random(len(ev)) < p) for p in (0.98, 0.95, 0.9, 0.8) for _ in range(12)]
        _cache["pool", name] = (clock.selectors(), np.array(rows, dtype=bool))
    return _cache["pool", name]


def _round_setup(oracle, name, specialised):
    """The context with the workload and the selectors loaded; the pool's rows split by demi_replay_wildcard_batch into those
    that reproduce and those that do not."""
    ctx = context(oracle, name, specialised)
    model, trace, fp, _ = Wc.workload(oracle, name)
    (ts, po), rows = _pool(oracle, name)
    ctx.replay_load(trace.original_externals, trace.events)
    ctx.replay_wildcard_load(ts, po)
    if ("split", name) not in _cache:
        v = ctx.replay_wildcard_batch(rows, limits(fp))
        assert not (v["flags"] & OVF).any()
        ok = rows[(v["flags"] & T.V_VIOLATION) != 0]
        bad = rows[(v["flags"] & T.V_VIOLATION) == 0]
        assert len(ok) >= 2 and len(bad) >= 2
        _cache["split", name] = (ok, bad)
    return ctx, limits(fp), len(trace.events), rows, _cache["split", name]


def _round_lists(n, rows, ok, bad):
    """Rounds of n rows: the pool as it is (real proposals first), then failing rows with a hit at index 0, at the last index, two
    hits (the lower wins), and none."""
    cyc = lambda a, k: a[np.arange(k) % len(a)]
    out = [cyc(rows, n)]
    for hits in ([0], [n - 1], [n // 3, n - 1], []):
        r = cyc(bad, n).copy()
        for k, h in enumerate(hits):
            r[h] = ok[k % len(ok)]
        out.append(r)
    return out


def _check_round(ctx, rows, lim, n_rec):
    v = ctx.replay_wildcard_batch(rows, lim)
    assert not (v["flags"] & OVF).any()
    hits = np.nonzero(v["flags"] & T.V_VIOLATION)[0]
    res, kept = ctx.replay_wildcard_round(rows, lim)
    if len(hits) == 0:
        assert res.first_hit == NONE and kept is None and res.verdict.flags == 0 and res.n_kept == 0 and res.executed_len == 0
        return res
    assert res.first_hit == int(hits[0])
    gv, gk, rec = ctx.replay_wildcard_get_trace(rows[res.first_hit], lim)
    assert kept.tobytes() == gk.tobytes() and res.n_kept == int(gk.astype(bool).sum())
    assert bytes(res.verdict) == bytes(gv) and int(gv.flags) & T.V_VIOLATION
    assert res.executed_len == len(rec)
    return res


@pytest.mark.parametrize("lanes", [None, 1, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("specialised", [False, True])
def test_round_equals_wildcard_batch_and_get_trace(oracle, monkeypatch, specialised, n, lanes):
    if lanes is not None:
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_K2_LANES_PER_WAVE", str(lanes))
    ctx, lim, n_rec, rows, (ok, bad) = _round_setup(oracle, "narrow0", specialised)
    firsts = set()
    for r in _round_lists(n, rows, ok, bad):
        res = _check_round(ctx, r, lim, n_rec)
        assert res.launches == 1 and res.retried == 0            # the default budget holds the whole round
        firsts.add(res.first_hit)
    assert {0, NONE} <= firsts and (n == 1 or n - 1 in firsts)
    res, kept = ctx.replay_wildcard_round(np.zeros((0, n_rec), dtype=bool), lim)
    assert res.first_hit == NONE and kept is None and res.launches == 0


@pytest.mark.parametrize("name", ["real3", "array5"])
def test_round_on_tables_that_run_only_compiled(oracle, name):
    ctx, lim, n_rec, rows, (ok, bad) = _round_setup(oracle, name, True)
    for r in _round_lists(65, rows, ok, bad):
        _check_round(ctx, r, lim, n_rec)


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("specialised", [False, True])
def test_a_round_wider_than_the_kept_budget_is_split(oracle, monkeypatch, specialised, n):
    ctx, lim, n_rec, rows, (ok, bad) = _round_setup(oracle, "narrow0", specialised)
    lists = _round_lists(n, rows, ok, bad)
    whole = [ctx.replay_wildcard_round(r, lim) for r in lists]
    # a plane of 16 x (recorded events) bytes: the lowered events are fewer than the recorded ones, but more than a quarter of
    # them (every delivery is lowered), so a launch holds 16 .. 63 proposals
    monkeypatch.setenv("DEMI_EXPERIMENT", "1")
    monkeypatch.setenv("DEMI_INTMIN_KEPT_BYTES", str(16 * n_rec))
    for r, (w, wk) in zip(lists, whole):
        res = _check_round(ctx, r, lim, n_rec)
        assert res.first_hit == w.first_hit and bytes(res.verdict) == bytes(w.verdict) and res.executed_len == w.executed_len
        last = n - 1 if res.first_hit == NONE else res.first_hit          # the launch that holds it is the last one
        assert last // 63 + 1 <= res.launches <= last // 16 + 1
        if last == n - 1:
            assert res.launches > 1                                         # the round was split
    # one byte: a proposal per launch, and the round stops at the launch that holds the hit
    monkeypatch.setenv("DEMI_INTMIN_KEPT_BYTES", "1")
    r = bad[np.arange(n) % len(bad)].copy()
    r[n // 4] = ok[0]
    res = _check_round(ctx, r, lim, n_rec)
    assert res.first_hit == n // 4 and res.launches == n // 4 + 1


# ------------------------------------------------------------------ 2. the loop against the mirror and the transliteration
def scala_minimizer(oracle, name, clustering, policy):
    """(trace bytes, total_replays) of the transliterated Scala minimizer, once per case."""
    key = ("scala", name, clustering, policy)
    if key not in _cache:
        model, trace, fp, device = Wc.workload(oracle, name)
        cls = Pc.AreaWildcardMinimizer if device is Pc.AreaTransliteratedDevice else X.ScalaWildcardMinimizer
        ref = cls(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=X.STRATEGIES[Wc.POLICIES[policy]][0](),
                  clusteringStrategy=clustering)
        want = ref.minimize()
        _cache[key] = (T.rec_events(want.events).tobytes(), ref.total_replays)
    return _cache[key]


def check_native_loop(ctx, oracle, name, clustering, policy, max_batch, skip_clock=0, lim=None):
    """demi_minimize_wildcards on the workload = the mirror at the same max_batch; returns its stats."""
    model, trace, fp, _ = Wc.workload(oracle, name)
    want = Wc.mirror(oracle, name, clustering, policy, skip_clock, max_batch)
    ctx.replay_load(trace.original_externals, trace.events)
    events, sizes, batches, st = ctx.minimize_wildcards(lim or limits(fp), Wc.params_of(model, clustering, policy, skip_clock, max_batch))
    assert events.tobytes() == want["trace"].tobytes()
    assert int(st.total_replays) == want["total_replays"] and sizes == want["internal_sizes"]
    assert batches == want["batches"] and int(st.rounds) == len(batches) and int(st.adoptions) == want["adoptions"]
    assert int(st.deliveries_before) == countMsgEvents(trace) and int(st.deliveries_after) == int((events["kind"] == T.REC_MSG_EVENT).sum())
    if not skip_clock:
        s_trace, s_total = scala_minimizer(oracle, name, clustering, policy)
        assert events.tobytes() == s_trace and int(st.total_replays) == s_total
    # the context's loaded execution IS the minimized one, without selectors: it replays strictly, and it reloads
    assert int(_native.lib().demi_replay_recorded_len(ctx._h)) == len(events)
    with pytest.raises(_native.DemiError, match="demi_replay_wildcard_load must precede"):
        ctx.replay_wildcard_batch(np.ones((1, len(events)), dtype=bool), limits(fp))
    for _ in range(2):
        v = ctx.replay_removal_batch([NO_SKIP], limits(fp))[0]
        assert int(v["flags"]) & T.V_VIOLATION and not int(v["flags"]) & T.V_DIVERGED
        assert T.verdict_deliveries(int(v["flags"])) == int(st.deliveries_after)
        ctx.replay_load(trace.original_externals, events)
    return st


@pytest.mark.parametrize("max_batch", [0, 7, 1])
@pytest.mark.parametrize("policy", ["LAST", "FIRST"])
@pytest.mark.parametrize("clustering", sorted(Wc.CLUSTERINGS))
@pytest.mark.parametrize("name", ["narrow0", "real3", "array5"])
def test_native_loop_equals_the_mirror_and_the_transliteration(oracle, name, clustering, policy, max_batch):
    ctx = context(oracle, name, name in COMPILED_ONLY)
    st = check_native_loop(ctx, oracle, name, clustering, policy, max_batch)
    assert st.retried == 0
    # one replay launch per round, and one recorded replay per pass that adopted a trace - not one per adoption
    passes = 2 if clustering == "ClockThenSingleton" else 1
    assert st.rounds <= st.launches <= st.rounds + passes


def test_native_loop_on_the_specialised_narrow_table_and_with_skip_clock_clusters(oracle):
    ctx = context(oracle, "narrow0", True)
    check_native_loop(ctx, oracle, "narrow0", "ClockThenSingleton", "LAST", 0)
    for max_batch in (0, 1):
        check_native_loop(ctx, oracle, "narrow1", "ClockClusterizer", "FIRST", max_batch, skip_clock=1)


def test_launches_fall_by_one_per_adoption(oracle):
    """What the native call is for: the mirror pays a second, recording launch per adoption, the native loop one per pass."""
    model, trace, fp, _ = Wc.workload(oracle, "narrow0")
    ctx = context(oracle, "narrow0", False)
    st = check_native_loop(ctx, oracle, "narrow0", "ClockThenSingleton", "LAST", 0)
    orc = W.StsWildcardOracle(SchedulerConfig(model=model), p_max=P_MAX)
    try:
        m = W.WildcardMinimizer(SchedulerConfig(model=model), trace.original_externals, trace, fp, resolutionStrategy=W.LastOnlyStrategy(),
                                clusteringStrategy="ClockThenSingleton", oracle=orc)
        m.minimize()
        assert st.adoptions >= 2 and orc.launches == st.rounds + st.adoptions and st.launches <= st.rounds + 2
    finally:
        orc.shutdown()


# ------------------------------------------------------------------ 3. capacity
def test_a_capacity_before_the_hit_is_evaluated_again(oracle):
    """A pending set so small that a proposal BEFORE the round's first hit aborts - the premise asserted on the transliteration
    (the most messages pending at once in that proposal's replay) and on the device: the round answers what it answers with the
    largest pending set, and so does the loop, with retried > 0."""
    name = "real3"
    model, trace, fp, _ = Wc.workload(oracle, name)
    ctx, lim, n_rec, rows, (ok, bad) = _round_setup(oracle, name, True)
    (ts, po), _ = _pool(oracle, name)
    most = lambda row: Pc.run_candidate(oracle, model, trace, fp, X.wildcards_of(ts, po), row)[4].max_pending
    ok_most, bad_most = [most(r) for r in ok[:24]], [most(r) for r in bad[:48]]
    print("most pending at once: reproducing rows", sorted(set(ok_most)), "failing rows", sorted(set(bad_most)))
    hit, deep = ok[int(np.argmin(ok_most))], bad[int(np.argmax(bad_most))]
    assert max(bad_most) > min(ok_most), "no failing proposal holds more pending messages than a reproducing one"
    p_small = max(bad_most) - 1                                         # the reproducing proposal fits, the failing one does not
    r = np.array([deep, bad[1], hit, deep])
    g = ctx.replay_wildcard_batch(r, limits(fp, p_small))
    assert int(g["flags"][0]) & OVF and not int(g["flags"][2]) & OVF    # the overflow really happens on the device
    big, big_kept = ctx.replay_wildcard_round(r, limits(fp, T.MAX_PENDING))
    res, kept = ctx.replay_wildcard_round(r, limits(fp, p_small))
    assert res.first_hit == big.first_hit == 2 and bytes(res.verdict) == bytes(big.verdict) and kept.tobytes() == big_kept.tobytes()
    assert res.executed_len == big.executed_len
    assert res.retried == 3 and res.launches == 2 and big.retried == 0 and big.launches == 1
    # an abort AFTER the hit is ignored: the sequential loop never gets there
    res, _ = ctx.replay_wildcard_round(np.array([hit, deep]), limits(fp, p_small))
    assert res.first_hit == 0 and res.retried == 0 and res.launches == 1
    st = check_native_loop(ctx, oracle, name, "ClockThenSingleton", "LAST", 0, lim=limits(fp, p_small))
    assert st.retried > 0 and st.launches > st.rounds


def test_a_capacity_that_stays_is_an_error_by_name(oracle):
    """tests/test_intmin_native_gpu.py's capacity case: without the Arm's delivery Kick runs a ninth effect row -
    DEMI_V_QUEUE_OVF whatever the pending capacity, so an already-maximal p_max leaves nothing to evaluate again."""
    from .test_intmin_native_gpu import _beyond_case
    from demi_amd import internal_minimization as IM
    model, ev, rec = _beyond_case(oracle)
    lim = T.Limits(0, 0, T.MAX_PENDING, 1, 0x1000103, 0, 0, 0)
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        ctx.replay_load(ev, rec)
        n = len(rec)
        arm_id = int(rec["id"][(rec["kind"] == T.REC_MSG_SEND) & (rec["ext_idx"] == 1)][0])
        arm = int(np.nonzero((rec["kind"] == T.REC_MSG_EVENT) & (rec["id"] == arm_id))[0][0])
        ctx.replay_wildcard_load(np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
        row = np.ones((1, n), dtype=bool)
        row[0, arm] = False
        assert int(ctx.replay_wildcard_batch(row, lim)[0]["flags"]) & T.V_QUEUE_OVF
        with pytest.raises(_native.DemiError, match="capacities") as e:
            ctx.replay_wildcard_round(row, lim)
        assert e.value.code == T.ERR_CAPACITY
        # the loop: the execution re-based on [Start, WaitQuiescence, Kick] - every proposal of it runs the ninth row
        keep = ~(((rec["kind"] == T.REC_MSG_SEND) | (rec["kind"] == T.REC_MSG_EVENT)) & (rec["id"] == arm_id))
        based = IM.executed_trace(EventTrace(rec, ev), keep, subseq=[0, 2, 3])
        ctx.replay_load(based.original_externals, based.events)
        ctx.replay_wildcard_load(np.zeros(len(based.events), dtype=np.uint32), np.zeros(len(based.events), dtype=np.uint8))
        assert int(ctx.replay_wildcard_batch(np.ones((1, len(based.events)), dtype=bool), lim)[0]["flags"]) & T.V_QUEUE_OVF
        for clustering in (T.CLUSTER_CLOCK, T.CLUSTER_SINGLETON):
            with pytest.raises(_native.DemiError, match="capacities") as e:
                ctx.minimize_wildcards(lim, T.WcminParams(clustering, T.WILDCARD_FIRST))
            assert e.value.code == T.ERR_CAPACITY
            # the context still holds the loaded execution (nothing was adopted), and no selectors
            assert int(_native.lib().demi_replay_recorded_len(ctx._h)) == len(based.events)
            assert ctx.replay_removal_batch([NO_SKIP], lim) is not None
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals_by_name(oracle):
    model, trace, fp, _ = Wc.workload(oracle, "narrow0")
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        lim = limits(fp)
        par = Wc.params_of(model, "ClockClusterizer", "LAST", 0, 0)
        with pytest.raises(_native.DemiError, match="demi_replay_load must precede demi_minimize_wildcards") as e:
            ctx.minimize_wildcards(lim, par)
        assert e.value.code == T.ERR_NO_TRACE
        ctx.replay_load(trace.original_externals, trace.events)
        with pytest.raises(_native.DemiError, match="must precede demi_replay_wildcard_round") as e:     # (no selectors loaded)
            ctx.replay_wildcard_round(np.ones((1, len(trace.events)), dtype=bool), lim)
        assert e.value.code == T.ERR_NO_TRACE
        with pytest.raises(_native.DemiError, match="looking_for_valid") as e:
            ctx.minimize_wildcards(T.Limits(0, 0, 64, 0, fp.code, 0, 0, 0), par)
        assert e.value.code == T.ERR_INVALID_ARG
        with pytest.raises(_native.DemiError, match="filter_known_absents") as e:
            ctx.minimize_wildcards(T.Limits(0, 0, 64, 1, fp.code, 0, 0, T.FILTER_ABSENTS_CORRECTED), par)
        assert e.value.code == T.ERR_INVALID_ARG
        with pytest.raises(_native.DemiError, match="unknown clustering strategy 7"):
            ctx.minimize_wildcards(lim, T.WcminParams(7, T.WILDCARD_LAST))
        with pytest.raises(_native.DemiError, match="unknown wildcard policy 9"):
            ctx.minimize_wildcards(lim, T.WcminParams(T.CLUSTER_CLOCK, 9))
        gather = _native.ALLGATHER_FN(lambda user, send, recv, nbytes: 0)
        assert _native.lib().demi_comm_create_host(ctx._h, 0, 1, gather, None) == 0
        with pytest.raises(_native.DemiError, match="single rank") as e:
            ctx.minimize_wildcards(lim, par)
        assert e.value.code == T.ERR_INVALID_ARG
        assert _native.lib().demi_comm_destroy(ctx._h) == 0
        # the refusals left the loaded execution alone
        assert int(_native.lib().demi_replay_recorded_len(ctx._h)) == len(trace.events)
        # a buffer below the result's length: DEMI_ERR_CAPACITY with the length needed, and the minimized execution is loaded
        want = Wc.mirror(oracle, "narrow0", "ClockClusterizer", "LAST", 0, 0)
        with pytest.raises(_native.DemiError, match="has %d events" % len(want["trace"])) as e:
            ctx.minimize_wildcards(lim, par, cap=len(want["trace"]) - 1)
        assert e.value.code == T.ERR_CAPACITY
        assert int(_native.lib().demi_replay_recorded_len(ctx._h)) == len(want["trace"])
    finally:
        ctx.close()
    # a table of more than 8 actors
    from demi_amd.fuzzer import events_to_array, send, start
    big = M.raft_model(11)
    ev = events_to_array([start(a) for a in range(11)] + [send(a, M.M_BOOTSTRAP) for a in range(11)])
    _, rec, _ = oracle.random_execute(big, ev, 1, T.Limits(40, 0, 128, 0, 0, 0))
    ctx = _native.Context(0)
    try:
        ctx.model_load(big.to_struct())
        ctx.replay_load(ev, rec)
        with pytest.raises(_native.DemiError, match="more than 8 actors") as e:
            ctx.minimize_wildcards(T.Limits(0, 0, 64, 1, 0x1000103, 0, 0, 0), T.WcminParams())
        assert e.value.code == T.ERR_INVALID_ARG
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5. the Python entry points
def test_python_entry_points_return_what_their_default_paths_return(oracle):
    from demi_amd.runner_utils import run_the_gamut
    from .test_minification_cpu import _violating_execution
    model, trace, fp, _ = Wc.workload(oracle, "narrow0")
    cfg = SchedulerConfig(model=model)
    for clustering in sorted(Wc.CLUSTERINGS):
        out = []
        for native in (False, True):
            stats = MinimizationStats()
            m = W.WildcardMinimizer(cfg, trace.original_externals, trace, fp, resolutionStrategy=W.LastOnlyStrategy(),
                                    clusteringStrategy=clustering, stats=stats, p_max=P_MAX, native=native)
            _, t = m.minimize()
            out.append((t.events.tobytes(), t.original_externals.tobytes(), stats.total_replays, m.internal_sizes, m.batches))
        assert out[0] == out[1] and out[0][2] > 0
    # a trace with the payload areas of its externals keeps them
    model3, trace3, fp3, _ = Wc.workload(oracle, "real3")
    areas = np.arange(len(trace3.original_externals), dtype=np.uint64)
    t3 = EventTrace(trace3.events, trace3.original_externals, areas)
    _, got = W.WildcardMinimizer(SchedulerConfig(model=model3), t3.original_externals, t3, fp3, p_max=P_MAX, native=True).minimize()
    assert (got.ext_areas == areas).all() and (got.original_externals == trace3.original_externals).all()
    events, lim = Pc._events_and_limits(dict(n=5))
    vv, rec, used = _violating_execution(oracle, model, events, lim, X.WORKLOAD_SKIPS[0])
    stages = ("DDMin", "IntMin", "WildcardsNoBackTracks", "WildcardsLastOnly")
    from demi_amd.schedulers import ViolationFingerprint
    a = run_the_gamut(cfg, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint), stages=stages, p_max=P_MAX)
    b = run_the_gamut(cfg, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint), stages=stages, p_max=P_MAX, native_wildcards=True)
    assert a["wildcard_replays"] == b["wildcard_replays"] and a["wildcard_deliveries"] == b["wildcard_deliveries"]
    assert a["wildcard_minimized"].events.tobytes() == b["wildcard_minimized"].events.tobytes()
