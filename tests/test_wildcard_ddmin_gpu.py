"""GPU suite: the candidates launch of the wildcard replay kernel (csrc/k2_wildcard_cand.hpp, demi_replay_wildcard_candidates)
and demi_wildcard_ddmin through the C ABI, bit for bit against the transliteration of tests/test_wildcard_ddmin_cpu.py and
tests/test_wildcard_transliteration_cpu.py: the verdict plane per proposal, the records reduced on the device, the same records
from demi_replay_wildcard_batch fed explicit presence rows, then the whole DDMin (MCS, consultations, first_hits,
total_replays, validated trace bytes) natively, through the Python mirror and sequentially.  No tolerance anywhere."""
import numpy as np
import pytest

from demi_amd import _native
from demi_amd import model as M
from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.apps import raft5_config2
from demi_amd.minification import events_to_masks
from demi_amd.runner_utils import run_the_gamut, wildcardDDMin
from demi_amd.schedulers import EventTrace, MinimizationStats, SchedulerConfig, ViolationFingerprint

from . import test_wildcard_ddmin_cpu as D
from . import test_wildcard_transliteration_cpu as X

pytestmark = pytest.mark.gpu

P_MAX = 128          # (the transliteration has no pending capacity: no replay of these tests may overflow, and that is asserted)
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
MIRROR = {"SrcDstFIFOOnly": W.SrcDstFIFOOnly, "BackTrackStrategy": W.BackTrackStrategy, "LastOnlyStrategy": W.LastOnlyStrategy}
_plane_memo = {}


def _ctx(model, specialised):
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if specialised or model.compiled_only:
        ctx.model_specialize()
    return ctx


def _shapes(trace, timers, rng):
    """[(masks, drops, base presence row or None)]: n_cand in {1, 3, 70} (below and above one wave), n_drop in {0, 1, T}, and
    5 x (1 + T) work items - more than a wave with candidates that straddle it (70 x (1 + T) replays of the transliteration would
    take minutes); random external masks (the first keeps everything), drops among the timers and, for n_drop = 1, any
    delivery; two cases over a base row with deliveries cleared in more than one presence word.  n_cand = 70 is covered only
    with n_drop = 1: the full 70 x (1 + T) point is not in the list."""
    n_ext = len(trace.original_externals)
    deliveries = np.nonzero(trace.events["kind"] == T.REC_MSG_EVENT)[0]

    def masks(n):
        keep = rng.random((n, n_ext)) < 0.85
        keep[0] = True
        return events_to_masks([tuple(np.nonzero(k)[0]) for k in keep])
    ev = trace.events
    internal = np.array([int(ev["kind"][i]) == T.REC_MSG_EVENT and int(ev["ext_idx"][i]) == 255 and i not in timers for i in range(len(ev))])
    base = ~(internal & (rng.random(len(ev)) < 0.1))          # a base row with about a tenth of the other deliveries cleared
    assert not base.all() and len(base) > 64                    # (more than one presence word)
    every = np.asarray(timers, dtype=np.uint32)
    return [(masks(1), np.zeros(0, dtype=np.uint32), None), (masks(3), every, None),
            (masks(70), np.array([rng.choice(deliveries)], dtype=np.uint32), None),
            (masks(3), np.array([timers[len(timers) // 2]], dtype=np.uint32), None),
            (masks(5), every, None),           # 5 x (1 + T) > 64 work items under the default launch shaping: candidates straddle waves
            (masks(3), every[:2], base), (masks(1), np.zeros(0, dtype=np.uint32), base)]


def _want_plane(oracle, key, model, trace, fp, wild, masks, drops, base=None):
    """The transliteration's verdict and executed length of every (candidate, proposal): run_candidate per proposal, once."""
    out = []
    for m in masks:
        sub = T.mask_to_events(m)
        row = []
        for j in range(len(drops) + 1):
            k = (key, tuple(sub), int(drops[j - 1]) if j else -1, None if base is None else base.tobytes())
            if k not in _plane_memo:
                present = np.ones(len(trace.events), dtype=bool) if base is None else base.copy()
                if j:
                    present[int(drops[j - 1])] = False
                v, _, executed, _, _ = X.run_candidate(oracle, model, trace, fp, wild, present, subseq=list(sub))
                _plane_memo[k] = (v, len(executed))
            row.append(_plane_memo[k])
        out.append(row)
    return out


def _reduce(rows, n_rec):
    """The sequential loop over a candidate's proposals -> (first_hit, executed_len, flags, first_ovf, hash) per candidate."""
    out = np.zeros(len(rows), dtype=T.WILDCARD_CANDIDATE_DTYPE)
    for c, row in enumerate(rows):
        out[c] = (T.NO_HIT, 0, 0, T.NO_HIT, 0)
        for j, ((flags, _, h), n) in enumerate(row):
            assert not flags & OVF
            if flags & T.V_VIOLATION:
                out[c] = (j, n, T.WC_REPRODUCES | (T.WC_LONGER if n > n_rec else 0), T.NO_HIT, h)
                break
    return out


def _compare_candidates(oracle, ctx, key, model, trace, fp, strategy, rng):
    lim = T.Limits(0, 0, P_MAX, 1, fp.code, 0, 0, 0)
    cl = W.ClockClusterizer(trace, model, MIRROR[strategy](), aggressiveness=W.Aggressiveness.STOP_IMMEDIATELY, skipClockClusters=True)
    ts, po = cl.selectors()
    timers = [cl.d.rec_of_id[i] for i in cl.timerIterator.toRemove]
    assert len(timers) >= 2
    ctx.replay_load(trace.original_externals, trace.events)
    ctx.replay_wildcard_load(ts, po)
    wild = X.wildcards_of(ts, po)
    hits = 0
    for masks, drops, base in _shapes(trace, timers, rng):
        got, plane = ctx.replay_wildcard_candidates(masks, drops, lim, base_present=base, want_all=True)
        want = _want_plane(oracle, (key, strategy), model, trace, fp, wild, masks, drops, base)
        for c in range(len(masks)):
            for j in range(len(drops) + 1):
                g = plane[c, j]
                assert (int(g["flags"]), int(g["fingerprint"]), int(g["hash"])) == want[c][j][0], (c, j)
        reduced = _reduce(want, len(trace.events))
        assert got.tobytes() == reduced.tobytes()
        hits += int((got["flags"] & T.WC_REPRODUCES).sum())
        # the same answers from demi_replay_wildcard_batch fed the presence rows built here
        presents = np.ones((len(masks), len(drops) + 1, len(trace.events)), dtype=bool)
        if base is not None:
            presents[:, :] = base
        for j, d in enumerate(drops):
            presents[:, j + 1, int(d)] = False
        flat = ctx.replay_wildcard_batch(presents.reshape(-1, len(trace.events)), lim, masks=np.repeat(masks, len(drops) + 1, axis=0))
        assert flat.tobytes() == plane.reshape(-1).tobytes()
    return hits


@pytest.mark.parametrize("lanes", [None, 1, 64])
@pytest.mark.parametrize("specialised", [False, True])
def test_candidates_launch_equals_the_transliteration(oracle, monkeypatch, specialised, lanes):
    if lanes is not None:
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_K2_LANES_PER_WAVE", str(lanes))
    hits = 0
    for skip, strategy in ((4, "BackTrackStrategy"), (6, "LastOnlyStrategy"), (4, "SrcDstFIFOOnly")):
        model, trace, fp = D.workload(oracle, skip)
        ctx = _ctx(model, specialised)
        try:
            hits += _compare_candidates(oracle, ctx, skip, model, trace, fp, strategy, np.random.default_rng(21 + skip))
        finally:
            ctx.close()
    assert hits > 0


def test_wide_table_candidates_launch_equals_the_transliteration(oracle):
    model = M.raft_model(5, term0=1000, loglen0=300, election_budget=2)
    assert model.wide
    _, events, lim = raft5_config2()
    trace, fp = X._verified_mcs(oracle, model, events, lim, 0)
    ctx = _ctx(model, True)
    try:
        _compare_candidates(oracle, ctx, "wide", model, trace, fp, "LastOnlyStrategy", np.random.default_rng(5))
    finally:
        ctx.close()


@pytest.mark.parametrize("skip,strategy", D.WORKLOADS)
def test_native_wildcard_ddmin_equals_the_mirror_and_the_transliteration(oracle, skip, strategy):
    model, trace, fp = D.workload(oracle, skip)
    want = D.scala_wildcard_ddmin(oracle, skip, strategy)
    cfg = SchedulerConfig(model=model)
    records = []
    for kw in (dict(native=True), dict(native=True, sequential=True), dict(native=False, speculative_depth=2)):
        stats = MinimizationStats()
        got = wildcardDDMin(cfg, trace, fp, resolutionStrategy=MIRROR[strategy](), stats=stats, p_max=P_MAX, **kw)
        D.assert_equals_the_transliteration(want, got, stats)
        records.append(got[4])
    st, seq = records[0].stats, records[1].stats
    for r in records[:2]:           # WildcardTestOracle.minTrace / externalsForMinTrace as the native call keeps them
        res = r.result
        if int(res.min_first_hit) == T.NO_HIT:
            assert want["min"] == ((), len(trace.events))
        else:
            assert (tuple(T.mask_to_events(np.array(list(res.min_externals), dtype=np.uint64))), int(res.min_executed_len)) == want["min"]
    assert records[0].result.retried == 0 and records[1].result.retried == 0
    assert st.consultations == seq.consultations == len(want["consulted"])
    assert all(b == 1 for b in records[1].batches) and seq.launches >= seq.consultations      # one consultation per launch
    assert st.launches < seq.launches or len(want["consulted"]) <= 2


def test_a_capacity_before_the_first_hit_is_unknown_and_evaluated_again(oracle):
    """p_max = 8: proposals of the frontier's candidates abort before any hit.  They are reported unknown, never 'does not
    reproduce', evaluated again with the largest pending set, and the DDMin is the one of the other tests."""
    skip, strategy = 4, "BackTrackStrategy"
    model, trace, fp = D.workload(oracle, skip)
    want = D.scala_wildcard_ddmin(oracle, skip, strategy)
    wo = W.WildcardTestOracle(SchedulerConfig(model=model), trace, resolutionStrategy=MIRROR[strategy](), p_max=8)
    try:
        first = [c for c, _ in want["consulted"]][:8]
        small = wo.oracle._ctx.replay_wildcard_candidates(events_to_masks(first), wo.drops, wo.oracle._limits(fp))
        full = wo.oracle._ctx.replay_wildcard_candidates(events_to_masks(first), wo.drops, wo.oracle._limits(fp, P_MAX))
        unknown = (small["flags"] & T.WC_UNKNOWN) != 0
        assert unknown.any() and not (full["flags"] & T.WC_UNKNOWN).any()
        assert (small["first_ovf"][unknown] < small["first_hit"][unknown]).all() and not (small["flags"][unknown] & T.WC_REPRODUCES).any()
        assert small[~unknown].tobytes() == full[~unknown].tobytes()
        assert wo.oracle.test_candidates(events_to_masks(first), wo.drops, fp).tobytes() == full.tobytes()
    finally:
        wo.shutdown()
    for native in (True, False):
        stats = MinimizationStats()
        got = wildcardDDMin(SchedulerConfig(model=model), trace, fp, resolutionStrategy=MIRROR[strategy](), stats=stats, p_max=8,
                            native=native, speculative_depth=0 if native else 2)
        D.assert_equals_the_transliteration(want, got, stats)
        if native:
            assert got[4].result.retried > 0


def test_native_wildcard_ddmin_with_a_base_presence_row(oracle):
    """base_present through demi_wildcard_ddmin: all ones is the NULL row, and with deliveries cleared every consultation's answer and
    first_hit are those demi_replay_wildcard_candidates gives for the same candidate and row (held against the transliteration above)."""
    skip, strategy = 6, "LastOnlyStrategy"
    model, trace, fp = D.workload(oracle, skip)
    wo = W.WildcardTestOracle(SchedulerConfig(model=model), trace, resolutionStrategy=MIRROR[strategy](), p_max=P_MAX)
    try:
        ctx, lim = wo.oracle._ctx, wo.oracle._limits(fp)
        par = T.DdminParams(check_unmodified=0)
        plain = ctx.wildcard_ddmin(lim, wo.drops, params=par)
        ones = ctx.wildcard_ddmin(lim, wo.drops, params=par, base_present=np.ones(len(trace.events), dtype=bool))
        assert plain[:3] == ones[:3] and int(plain[4].total_replays) == int(ones[4].total_replays)
        base = np.ones(len(trace.events), dtype=bool)
        base[[int(d) for d in wo.drops[::3]]] = False              # (a third of the timers is gone from every proposal)
        mcs, cons, _, st, res = ctx.wildcard_ddmin(lim, wo.drops, params=par, base_present=base)
        r = ctx.replay_wildcard_candidates(events_to_masks([c for c, _, _ in cons]), wo.drops, lim, base_present=base)
        assert not (r["flags"] & T.WC_UNKNOWN).any() and len(cons) == st.consultations
        for (c, passed, hit), x in zip(cons, r):
            reproduces = bool(int(x["flags"]) & T.WC_REPRODUCES)
            assert passed == (not reproduces or bool(int(x["flags"]) & T.WC_LONGER))
            assert hit == (int(x["first_hit"]) if reproduces else None)
        assert int(res.total_replays) == sum(h + 1 if h is not None else 1 + len(wo.drops) for _, _, h in cons)
        assert [c for c, _, _ in cons] != [c for c, _, _ in plain[1]] or [h for _, _, h in cons] != [h for _, _, h in plain[1]]
    finally:
        wo.shutdown()


def test_a_capacity_that_stays_is_an_error_by_name(oracle):
    """The candidate without the Arm runs a ninth effect row (tests/test_limits_gpu.py _k2_beyond_cases): no pending set is
    large enough, and demi_wildcard_ddmin says so instead of answering."""
    from .test_limits_gpu import _k2_beyond_cases
    name, model, ev, mm = _k2_beyond_cases()[0]
    ov, rec, _ = oracle.random_execute(model, ev, 5, T.Limits(mm, 0, 64, 0, 0, 0))
    ctx = _ctx(model, False)
    try:
        ctx.replay_load(ev, rec)
        ctx.replay_wildcard_load(np.zeros(len(rec), dtype=np.uint32), np.zeros(len(rec), dtype=np.uint8))
        lim = T.Limits(0, 0, 64, 1, 0x1000103, 0, 0, 0)
        r = ctx.replay_wildcard_candidates(events_to_masks([(0, 1, 3), (0, 3)]), [], lim)
        assert [int(f) for f in r["flags"]] == [0, T.WC_UNKNOWN] and int(r["first_ovf"][1]) == 0
        with pytest.raises(_native.DemiError, match="capacities") as e:
            ctx.wildcard_ddmin(lim, [])
        assert e.value.code == T.ERR_CAPACITY
    finally:
        ctx.close()


def test_refusals_by_name(oracle):
    model, trace, fp = D.workload(oracle, 4)
    ctx = _ctx(model, False)
    try:
        ctx.replay_load(trace.original_externals, trace.events)
        n = len(trace.events)
        ctx.replay_wildcard_load(np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
        masks = np.full((1, 4), ~np.uint64(0), dtype=np.uint64)
        lim = T.Limits(0, 0, 64, 1, fp.code, 0, 0, 0)
        not_a_delivery = int(np.nonzero(trace.events["kind"] != T.REC_MSG_EVENT)[0][0])
        for call in (lambda l, d: ctx.replay_wildcard_candidates(masks, d, l), lambda l, d: ctx.wildcard_ddmin(l, d)):
            with pytest.raises(_native.DemiError, match="filter_known_absents"):
                call(T.Limits(0, 0, 64, 1, fp.code, 0, 0, T.FILTER_ABSENTS_CORRECTED), [])
            with pytest.raises(_native.DemiError, match="not a MsgEvent of the loaded trace"):
                call(lim, [not_a_delivery])
            with pytest.raises(_native.DemiError, match="not a MsgEvent of the loaded trace"):
                call(lim, [n])
        with pytest.raises(_native.DemiError, match="at most 4096 candidates"):
            ctx.replay_wildcard_candidates(np.zeros((4097, 4), dtype=np.uint64), [], lim)
        gather = _native.ALLGATHER_FN(lambda user, send, recv, nbytes: 0)
        assert _native.lib().demi_comm_create_host(ctx._h, 0, 1, gather, None) == 0
        with pytest.raises(_native.DemiError, match="single rank"):
            ctx.wildcard_ddmin(lim, [])
        assert _native.lib().demi_comm_destroy(ctx._h) == 0
    finally:
        ctx.close()


def test_the_gamut_with_wildcard_ddmin_stages_ends_in_a_violating_trace(oracle):
    model, trace, fp = D.workload(oracle, 6)
    stages = ("DDMin", "IntMin", "WildCardDDMinNoBacktracks", "WildCardDDMinLastOnly", "WildcardsNoBackTracks", "WildcardsLastOnly")
    out = run_the_gamut(SchedulerConfig(model=model), trace, fp, stages=stages, p_max=P_MAX)
    assert set(out["wildcard_ddmin_replays"]) == {"WildCardDDMinNoBacktracks", "WildCardDDMinLastOnly"}
    final = out["wildcard_minimized"]
    ctx = _ctx(model, False)
    try:
        ctx.replay_load(final.original_externals, final.events)
        v = ctx.replay_batch(np.full((1, 4), ~np.uint64(0), dtype=np.uint64), T.Limits(0, 0, P_MAX, 1, fp.code, 0))[0]
        assert int(v["flags"]) & T.V_VIOLATION and not int(v["flags"]) & T.V_DIVERGED
    finally:
        ctx.close()
    # a rerun that shouldRerunDDMin declines leaves the later stages what they were without the new ones
    declined = run_the_gamut(SchedulerConfig(model=model), trace, fp, stages=stages, p_max=P_MAX, shouldRerunDDMin=lambda ext: False)
    without = run_the_gamut(SchedulerConfig(model=model), trace, fp, stages=("DDMin", "IntMin", "WildcardsNoBackTracks", "WildcardsLastOnly"), p_max=P_MAX)
    assert "wildcard_ddmin_replays" not in declined
    assert declined["wildcard_minimized"].events.tobytes() == without["wildcard_minimized"].events.tobytes()
    # the default stages are what they were
    plain = run_the_gamut(SchedulerConfig(model=model), trace, fp, p_max=P_MAX)
    assert "wildcard_ddmin_replays" not in plain and plain["mcs"] == out["mcs"] and plain["minimized_deliveries"] == out["minimized_deliveries"]
