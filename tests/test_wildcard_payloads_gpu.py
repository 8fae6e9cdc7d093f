"""GPU suite: the wildcard replay kernels (csrc/k2_wildcard.hpp, k2_wildcard_cand.hpp) compiled for DEMI_MODEL_PAYLOADS and
DEMI_MODEL_ARRAY tables, through the C ABI, bit for bit against the (type, area) transliteration of
tests/wildcard_payload_cases.py: flags, fingerprint and hash of every verdict, the kept marks and the executed trace with p_hi;
the candidates launch and demi_wildcard_ddmin; WildcardMinimizer and run_the_gamut end to end; the refusals.  No tolerance."""
import numpy as np
import pytest

from demi_amd import _native
from demi_amd import model as M
from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.minification import events_to_masks
from demi_amd.runner_utils import run_the_gamut, wildcardDDMin
from demi_amd.schedulers import EventTrace, MinimizationStats, SchedulerConfig

from . import test_wildcard_transliteration_cpu as X
from . import wildcard_payload_cases as Pc
from .test_wildcard_ddmin_cpu import assert_equals_the_transliteration

pytestmark = pytest.mark.gpu

P_MAX = Pc.P_MAX     # (sufficient: tests/test_wildcard_payloads_cpu.py test_workload_conditions; no overflow flag may appear)
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
_want = {}


def _ctx(model, specialise=True):
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if specialise:
        ctx.model_specialize()
    return ctx


def _candidates(model, trace, rng, n_random):
    """As tests/test_wildcard_gpu.py _candidates: random presence masks under the three policies, and the proposal sequences of
    the mirror's clusterizers (held against the transliteration's in the CPU suite)."""
    ev = trace.events
    is_ev = ev["kind"] == T.REC_MSG_EVENT
    internal = np.array([bool(is_ev[i]) and model.msg_class[int(ev["msg_type"][i])] != T.MSG_EXTERNAL for i in range(len(ev))])
    out = []
    for policy in (T.WILDCARD_HEAD, T.WILDCARD_FIRST, T.WILDCARD_LAST):
        ts = np.where(internal, np.uint32(1) << ev["msg_type"].astype(np.uint32), 0).astype(np.uint32)
        po = np.full(len(ev), policy, dtype=np.uint8)
        presents = [np.ones(len(ev), dtype=bool)] + [~internal | (rng.random(len(ev)) < p) for p in (0.97, 0.9, 0.8) for _ in range(n_random)]
        out.append((ts, po, presents))
    for strategy, cls in (("BackTrackStrategy", W.ClockClusterizer), ("LastOnlyStrategy", W.ClockClusterizer), ("LastOnlyStrategy", W.SingletonClusterizer)):
        c = cls(trace, model, X.STRATEGIES[strategy][1]())
        ts, po = c.selectors()
        presents = []
        p = c.getNextTrace(False, frozenset())
        while p is not None and len(presents) < 8:
            presents.append(p)
            p = c.getNextTrace(False, frozenset())
        out.append((ts, po, presents))
    return out


def _reference(oracle, table):
    """[(model, trace, fp, [(ts, po, presents, [run_candidate results])])] of a table, computed once and shared."""
    if table not in _want:
        rng = np.random.default_rng(31)
        out = []
        for spec in Pc.WORKLOADS[table]:
            model, trace, fp = Pc.get(oracle, spec)
            sets = []
            for ts, po, presents in _candidates(model, trace, rng, 3):
                wild = X.wildcards_of(ts, po)
                sets.append((ts, po, presents, [Pc.run_candidate(oracle, model, trace, fp, wild, p)[:4] for p in presents]))
            out.append((model, trace, fp, sets))
        _want[table] = out
    return _want[table]


@pytest.mark.parametrize("lanes", [None, 1, 64])
@pytest.mark.parametrize("table", sorted(Pc.WORKLOADS))
def test_wildcard_replays_equal_the_transliteration(oracle, monkeypatch, table, lanes):
    if lanes is not None:
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_K2_LANES_PER_WAVE", str(lanes))
    total = through_p_hi = 0
    for model, trace, fp, sets in _reference(oracle, table):
        lim = T.Limits(0, 0, P_MAX, 1, fp.code, 0, 0, 0)
        ctx = _ctx(model)
        try:
            ctx.replay_load(trace.original_externals, trace.events)
            for ts, po, presents, want in sets:
                ctx.replay_wildcard_load(ts, po)
                got = ctx.replay_wildcard_batch(np.array(presents), lim)
                assert not (got["flags"] & OVF).any()
                for k, present in enumerate(presents):
                    v, kept, executed, ignored = want[k]
                    assert (int(got["flags"][k]), int(got["fingerprint"][k]), int(got["hash"][k])) == v, (k, v)
                    through_p_hi += Pc.leaves_through_a_field_past_the_second(model, executed, trace.events)
                    if total % 7 == 0:
                        v1, kept1, rec1 = ctx.replay_wildcard_get_trace(present, lim)
                        assert (int(v1.flags), int(v1.fingerprint), int(v1.hash)) == v
                        assert (kept1 == kept).all()
                        assert len(rec1) == len(executed) and rec1.tobytes() == executed.tobytes()           # (p_hi included)
                        assert {int(i) for i in np.nonzero((trace.events["kind"] == T.REC_MSG_EVENT) & present & (kept1 == 0))[0]} == ignored
                    total += 1
        finally:
            ctx.close()
    assert total >= 100
    if table == "real3":
        assert through_p_hi > 0          # (replays that leave the recorded trace through a field past the second)


@pytest.mark.parametrize("with_masks", [False, True])
def test_exact_selectors_are_the_removal_replay(oracle, with_masks):
    """All ones and every type set 0: demi_replay_removal_batch without a removal; one cleared bit: that skip.  The executed trace
    reloads, with every field, and replays to the same hash."""
    model, trace, fp = Pc.get(oracle, Pc.WORKLOADS["real3"][0])
    ev = trace.events
    assert ev["p_hi"].any()
    ctx = _ctx(model)
    try:
        lim = T.Limits(0, 0, P_MAX, 1, fp.code, 0, 0, 0)
        ctx.replay_load(trace.original_externals, ev)
        dels = [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]]
        skips = [0xFFFFFFFF] + dels
        ctx.replay_wildcard_load(np.zeros(len(ev), dtype=np.uint32), np.zeros(len(ev), dtype=np.uint8))
        presents = np.ones((len(skips), len(ev)), dtype=bool)
        for k, i in enumerate(dels):
            presents[k + 1, i] = False
        masks = np.random.default_rng(2).integers(0, 1 << 63, size=(len(skips), 4), dtype=np.uint64) if with_masks else None
        want = ctx.replay_removal_batch(skips, lim, masks=masks)
        got = ctx.replay_wildcard_batch(presents, lim, masks=masks)
        assert (got == want).all() and not (want["flags"] & OVF).any()
        if not with_masks:
            assert (want["flags"] & T.V_VIOLATION).any() and not (want["flags"] & T.V_VIOLATION).all()
            v, kept, rec = ctx.replay_wildcard_get_trace(presents[0], lim)
            assert rec["p_hi"].any()
            ctx.replay_load(trace.original_externals, rec)
            again = ctx.replay_removal_batch([0xFFFFFFFF], lim)[0]
            assert int(again["hash"]) == int(v.hash) and int(again["flags"]) == int(v.flags) and int(v.flags) & T.V_VIOLATION
    finally:
        ctx.close()


def test_candidates_launch_and_native_ddmin_equal_the_transliteration(oracle):
    """demi_replay_wildcard_candidates and demi_wildcard_ddmin on the five-node real-field table against the transliterated
    WildcardTestOracle + DDMin: the reduced records of the consulted candidates, then MCS, consultations, first_hits,
    total_replays, the validated trace's bytes and the min_* record."""
    model, trace, fp, strategy = Pc.ddmin_workload(oracle)
    want = Pc.ddmin_reference(oracle)
    mirror = X.STRATEGIES[strategy][1]
    wo = W.WildcardTestOracle(SchedulerConfig(model=model), trace, resolutionStrategy=mirror(), p_max=P_MAX)
    try:
        cands = [c for c, _ in want["consulted"]]
        r = wo.oracle._ctx.replay_wildcard_candidates(events_to_masks(cands), wo.drops, wo.oracle._limits(fp))
        assert not (r["flags"] & T.WC_UNKNOWN).any()
        for x, hit, (c, passes) in zip(r, want["first_hits"], want["consulted"]):
            assert (int(x["first_hit"]) if int(x["flags"]) & T.WC_REPRODUCES else None) == hit, c
            assert passes == (hit is None or bool(int(x["flags"]) & T.WC_LONGER))
            if hit is not None:       # the executed length and hash of the reproducing proposal, as the transliteration replayed it
                present = trace.events["kind"] == T.REC_MSG_EVENT          # (the clusterizer's presence row: the deliveries)
                if hit:
                    present[int(wo.drops[hit - 1])] = False
                v, executed, _ = want["memo"][(tuple(c), present.tobytes())]
                assert int(x["executed_len"]) == len(executed) and int(x["hash"]) == v[2]
    finally:
        wo.shutdown()
    for kw in (dict(native=True), dict(native=True, sequential=True)):
        stats = MinimizationStats()
        got = wildcardDDMin(SchedulerConfig(model=model), trace, fp, resolutionStrategy=mirror(), stats=stats, p_max=P_MAX, **kw)
        assert_equals_the_transliteration(want, got, stats)
        res = got[4].result
        assert res.retried == 0
        if int(res.min_first_hit) == T.NO_HIT:
            assert want["min"] == ((), len(trace.events))
        else:
            assert (tuple(T.mask_to_events(np.array(list(res.min_externals), dtype=np.uint64))), int(res.min_executed_len)) == want["min"]


def test_wildcard_minimizer_on_the_gpu_is_the_transliterations(oracle):
    for table in ("real5", "real3"):
        model, trace, fp = Pc.get(oracle, Pc.WORKLOADS[table][0])
        ref = Pc.AreaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=X.ScalaLastOnlyStrategy(),
                                       clusteringStrategy="ClockThenSingleton")
        want = ref.minimize()
        stats = MinimizationStats()
        m = W.WildcardMinimizer(SchedulerConfig(model=model), trace.original_externals, trace, fp, resolutionStrategy=W.LastOnlyStrategy(),
                                clusteringStrategy=W.ClusteringStrategy.ClockThenSingleton, stats=stats, p_max=P_MAX)
        _, got = m.minimize()
        assert stats.total_replays == ref.total_replays
        assert len(got.events) == len(want.events) and got.events.tobytes() == want.events.tobytes()


def test_the_gamut_runs_every_stage_on_a_trace_with_ext_areas(oracle):
    """run_the_gamut with all six stages on a violating execution of the three-node real-field table whose EventTrace carries the
    payload areas of its externals: it ends in a trace that violates without divergence, with the areas of the kept externals."""
    model, trace, fp = Pc.get(oracle, Pc.WORKLOADS["real3"][0])
    ext = trace.original_externals
    npay = model.payloads
    areas = np.array([T.pay_area([int(e["p0"]) | int(e["p0_hi"]) << 8, int(e["p1"]) | int(e["p1_hi"]) << 8], npay) if int(e["kind"]) == T.EV_SEND else 0
                      for e in ext], dtype=np.uint64)
    stages = ("DDMin", "IntMin", "WildCardDDMinNoBacktracks", "WildCardDDMinLastOnly", "WildcardsNoBackTracks", "WildcardsLastOnly")
    out = run_the_gamut(SchedulerConfig(model=model), EventTrace(trace.events, ext, areas), fp, stages=stages, p_max=P_MAX)
    assert set(out["wildcard_ddmin_replays"]) == {"WildCardDDMinNoBacktracks", "WildCardDDMinLastOnly"}
    assert set(out["wildcard_replays"]) == {"WildcardsNoBackTracks", "WildcardsLastOnly"}
    final = out["wildcard_minimized"]
    assert out["wildcard_deliveries"] <= out["minimized_deliveries"] and len(final.original_externals) < len(ext)
    # the areas of the externals it kept: each kept external is one of the original ones, with that one's area
    assert final.ext_areas is not None and len(final.ext_areas) == len(final.original_externals)
    pool = {}
    for e, a in zip(ext, areas):
        pool.setdefault(e.tobytes(), set()).add(int(a))
    assert all(int(a) in pool[e.tobytes()] for e, a in zip(final.original_externals, final.ext_areas))
    assert (out["verified_mcs"].ext_areas == areas[list(out["mcs"])]).all()
    ctx = _ctx(model)
    try:
        ctx.replay_load(final.original_externals, final.events)
        v = ctx.replay_batch(np.full((1, 4), ~np.uint64(0), dtype=np.uint64), T.Limits(0, 0, P_MAX, 1, fp.code, 0))[0]
        assert int(v["flags"]) & T.V_VIOLATION and not int(v["flags"]) & T.V_DIVERGED
    finally:
        ctx.close()


def _k2w_lds(model, n_ext):
    """k2w_lds_bytes (csrc/k2_wildcard.hpp) restated: the tables, and four waves' lane memory with the array's words."""
    wide = bool(model.wide)
    arr_words = (model.array_len + (4 if wide else 8) - 1) // (4 if wide else 8)
    st_words = (2 if wide else 1) + arr_words
    ms = model.to_struct()
    tables = n_ext * 8 + 8 * 8 * st_words + int(ms.code_len) * 4 + int(ms.n_classes) * int(ms.n_msg_types) * 4 + 32 * 4 + 132 * 4 + 64 * 4
    tables = (tables + 15) & ~15
    hot, wb = (16, 8) if wide else (32, 4)
    wave = model.n_actors * 64 * 8 * st_words + hot * 64 * (wb + 4) + 8 * 64 * wb
    return tables + 4 * wave


def test_refusals_by_name(oracle):
    # an unspecialised context: these tables run only as compiled code
    model, trace, fp = Pc.get(oracle, Pc.WORKLOADS["real3"][0])
    n = len(trace.events)
    exact = (np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
    ctx = _ctx(model, specialise=False)
    try:
        ctx.replay_load(trace.original_externals, trace.events)
        ctx.replay_wildcard_load(*exact)
        with pytest.raises(_native.DemiError, match="compiled table"):
            ctx.replay_wildcard_batch(np.ones((1, n), dtype=bool), T.Limits(0, 0, 64, 1, fp.code, 0, 0, 0))
        with pytest.raises(_native.DemiError, match="compiled table"):
            ctx.replay_wildcard_candidates(np.full((1, 4), ~np.uint64(0), dtype=np.uint64), [], T.Limits(0, 0, 64, 1, fp.code, 0, 0, 0))
        ctx.model_specialize()
        ctx.replay_load(trace.original_externals, trace.events)
        ctx.replay_wildcard_load(*exact)
        with pytest.raises(_native.DemiError, match="filter_known_absents"):
            ctx.replay_wildcard_batch(np.ones((1, n), dtype=bool), T.Limits(0, 0, 64, 1, fp.code, 0, 0, T.FILTER_ABSENTS_CORRECTED))
    finally:
        ctx.close()
    # a BIG table (more than 8 actors) is still refused
    from demi_amd.fuzzer import events_to_array, send, start
    big = M.raft_model(11)
    ev = events_to_array([start(a) for a in range(11)] + [send(a, M.M_BOOTSTRAP) for a in range(11)])
    _, rec, _ = oracle.random_execute(big, ev, 1, T.Limits(40, 0, 128, 0, 0, 0))
    ctx = _ctx(big)
    try:
        ctx.replay_load(ev, rec)
        with pytest.raises(_native.DemiError, match="more than 8 actors"):
            ctx.replay_wildcard_load(np.zeros(len(rec), dtype=np.uint32), np.zeros(len(rec), dtype=np.uint8))
    finally:
        ctx.close()
    # a table whose lane memory exceeds the LDS budget: refused on the host, before anything is launched
    wide_log = M.replog_model(8, 64, True, False)             # eight actors with arrays of 64 elements: nine state words each
    ev = events_to_array([start(a) for a in range(8)] + [send(a % 3, M.RL_PUT, 30 + a, 0) for a in range(4)])
    assert _k2w_lds(wide_log, len(ev)) > 160 * 1024 >= _k2w_lds(model, len(trace.original_externals))
    _, rec, _ = oracle.random_execute(wide_log, ev, 1, T.Limits(30, 0, 128, 0, 0, 0))
    ctx = _ctx(wide_log, specialise=False)           # (the check precedes the compiled-table one: nothing needs compiling)
    try:
        ctx.replay_load(ev, rec)
        ctx.replay_wildcard_load(np.zeros(len(rec), dtype=np.uint32), np.zeros(len(rec), dtype=np.uint8))
        with pytest.raises(_native.DemiError, match="LDS budget exceeded"):
            ctx.replay_wildcard_batch(np.ones((1, len(rec)), dtype=bool), T.Limits(0, 0, 64, 1, 0x1000103, 0, 0, 0))
    finally:
        ctx.close()
