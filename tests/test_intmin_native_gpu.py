"""demi_replay_removal_round and demi_minimize_internals through the C ABI: one round of STSSchedMinimizer.minimize reduced on
the device (k2_removal_round.hpp) against the existing pair demi_replay_removal_batch / demi_replay_get_kept, and the whole loop
(intmin_host.hpp) against the sequential reference loop over the CPU oracle and the Python mirror's round sizes."""
import os

import numpy as np
import pytest

from demi_amd import _native, types as T
from demi_amd import internal_minimization as IM
from demi_amd.apps import raft5_config2
from demi_amd.schedulers import EventTrace, SchedulerConfig, ViolationFingerprint

from .test_internal_min_cpu import OracleRemoval, _verified_mcs
from .test_minification_cpu import _violating_execution

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NO_SKIP = 0xFFFFFFFF
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
STRATEGIES = {"LeftToRight": (IM.LeftToRightOneAtATime, T.REMOVAL_LEFT_TO_RIGHT), "SrcDstFIFO": (IM.SrcDstFIFORemoval, T.REMOVAL_SRC_DST_FIFO)}
_cache = {}


def workload(oracle, skip):
    """(model, verified MCS execution, fingerprint) of tests/test_internal_min_cpu._verified_mcs, computed once per skip."""
    if ("w", skip) not in _cache:
        model, events, lim = raft5_config2()
        _cache["w", skip] = (model,) + _verified_mcs(oracle, model, events, lim, skip)
    return _cache["w", skip]


def sequential(oracle, key, model, trace, fp, strategy):
    """The reference: the one-replay-at-a-time loop over the CPU oracle, computed once per workload and strategy."""
    if ("s", key, strategy) not in _cache:
        m = IM.STSSchedMinimizer(trace.original_externals, trace, fp, STRATEGIES[strategy][0](trace, model), OracleRemoval(oracle, model), max_batch=1)
        stats, out = m.minimize()
        _cache["s", key, strategy] = (stats.total_replays, out, m.internal_sizes, STRATEGIES[strategy][0](trace, model).unignorable)
    return _cache["s", key, strategy]


def mirror_batches(oracle, key, model, trace, fp, strategy, max_batch):
    """The Python mirror's round sizes at this max_batch (the mirror over the CPU oracle: the rounds do not depend on who replays)."""
    if ("b", key, strategy, max_batch) not in _cache:
        m = IM.STSSchedMinimizer(trace.original_externals, trace, fp, STRATEGIES[strategy][0](trace, model), OracleRemoval(oracle, model),
                                 max_batch=max_batch or (1 << 14))
        m.minimize()
        _cache["b", key, strategy, max_batch] = m.batches
    return _cache["b", key, strategy, max_batch]


def fresh(model, specialise=False):
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if specialise:
        ctx.model_specialize()
        assert ctx.is_specialized()
    return ctx


def limits(fp, p_max=64):
    return T.Limits(0, 0, p_max, 1, fp.code, 0)


def check_native_loop(ctx, oracle, key, model, trace, fp, strategy, max_batch, lim=None):
    """demi_minimize_internals on `trace` = the sequential reference; returns its stats."""
    total, want, sizes, unignorable = sequential(oracle, key, model, trace, fp, strategy)
    ctx.replay_load(trace.original_externals, trace.events)
    events, got_sizes, batches, st = ctx.minimize_internals(lim or limits(fp), T.IntminParams(STRATEGIES[strategy][1], max_batch))
    assert events.tobytes() == T.rec_events(want.events).tobytes()
    assert int(st.total_replays) == total and got_sizes == sizes and int(st.unignorable) == unignorable
    assert batches == mirror_batches(oracle, key, model, trace, fp, strategy, max_batch) and int(st.rounds) == len(batches)
    assert int(st.deliveries_before) == IM.countMsgEvents(trace) and int(st.deliveries_after) == IM.countMsgEvents(want)
    # the context's loaded execution IS the minimized one (no reload): it replays strictly
    v = ctx.replay_removal_batch([NO_SKIP], limits(fp))[0]
    assert int(v["flags"]) & T.V_VIOLATION and not int(v["flags"]) & T.V_DIVERGED
    assert T.verdict_deliveries(int(v["flags"])) == int(st.deliveries_after)
    assert int(_native.lib().demi_replay_recorded_len(ctx._h)) == len(events)
    return st


# ------------------------------------------------------------------ 1. a round against the existing pair
def _round_lists(n, d_fail, d_ok):
    out = []
    for pos in sorted({p for p in (0, 63, 64, 255, 256, n - 1) if p < n}):
        sk = np.full(n, d_fail, dtype=np.uint32)
        sk[pos] = d_ok
        out.append(sk)
    if n >= 2:
        sk = np.full(n, d_fail, dtype=np.uint32)
        sk[[n // 3, n - 1]] = d_ok                     # two hits: the lower wins
        out.append(sk)
    out.append(np.full(n, d_fail, dtype=np.uint32))    # none
    return out


def _check_round(ctx, sk, lim, n_rec):
    v = ctx.replay_removal_batch(sk, lim)
    assert not (v["flags"] & OVF).any()
    hits = np.nonzero(v["flags"] & T.V_VIOLATION)[0]
    res, kept = ctx.replay_removal_round(sk, lim)
    if len(hits) == 0:
        assert res.first_hit == NONE and kept is None and res.verdict.flags == 0 and res.n_kept == 0
        return res
    assert res.first_hit == int(hits[0])
    gv, gk = ctx.replay_get_kept(n_rec, int(sk[res.first_hit]), lim)
    assert kept.tobytes() == gk.tobytes() and res.n_kept == int(gk.astype(bool).sum())
    assert (res.verdict.flags, res.verdict.fingerprint, res.verdict.hash) == (gv.flags, gv.fingerprint, gv.hash)
    assert bytes(res.verdict) == bytes(gv)
    return res


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
    yield
    for key in [k for k in _cache if k[0] == "ctx"]:
        _cache.pop(key)[0].close()


def _round_setup(oracle, specialised):
    """One context per table flavour for all round cases (the table is compiled once): skip 1's execution loaded, a delivery
    whose removal does not reproduce and one whose removal does, both taken from demi_replay_removal_batch over all deliveries."""
    if ("ctx", specialised) not in _cache:
        model, trace, fp = workload(oracle, 1)
        ctx = fresh(model, specialised)
        ctx.replay_load(trace.original_externals, trace.events)
        dl = np.array([i for i, _, _ in IM.deliveries(trace)], dtype=np.uint32)
        lim = limits(fp)
        v = ctx.replay_removal_batch(dl, lim)
        ok = dl[(v["flags"] & T.V_VIOLATION) != 0]
        bad = dl[(v["flags"] & (T.V_VIOLATION | OVF)) == 0]
        assert len(ok) and len(bad)
        _cache["ctx", specialised] = (ctx, lim, len(trace.events), int(bad[0]), int(ok[0]))
    return _cache["ctx", specialised]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000])
@pytest.mark.parametrize("specialised", [False, True])
def test_round_equals_removal_batch_and_get_kept(oracle, specialised, n):
    ctx, lim, n_rec, d_fail, d_ok = _round_setup(oracle, specialised)
    for sk in _round_lists(n, d_fail, d_ok):
        res = _check_round(ctx, sk, lim, n_rec)
        assert res.launches == 1 and res.retried == 0            # the default budget holds the whole round
    res, kept = ctx.replay_removal_round(np.zeros(0, dtype=np.uint32), lim)
    assert res.first_hit == NONE and kept is None and res.launches == 0


@pytest.mark.parametrize("n", [64, 65, 257])
@pytest.mark.parametrize("specialised", [False, True])
def test_a_round_wider_than_the_kept_budget_is_split(oracle, monkeypatch, specialised, n):
    ctx, lim, n_rec, d_fail, d_ok = _round_setup(oracle, specialised)
    whole = [ctx.replay_removal_round(sk, lim) for sk in _round_lists(n, d_fail, d_ok)]
    # a plane of 16 x (recorded events) bytes: the lowered events are fewer than the recorded ones, but more than a quarter of
    # them (every delivery is lowered), so a launch holds 16 .. 63 candidates
    monkeypatch.setenv("DEMI_INTMIN_KEPT_BYTES", str(16 * n_rec))
    for sk, (w, wk) in zip(_round_lists(n, d_fail, d_ok), whole):
        res = _check_round(ctx, sk, lim, n_rec)
        assert res.first_hit == w.first_hit and bytes(res.verdict) == bytes(w.verdict)
        last = n - 1 if res.first_hit == NONE else res.first_hit          # the launch that holds it is the last one
        assert last // 63 + 1 <= res.launches <= last // 16 + 1
        if last == n - 1:
            assert res.launches >= 2                                        # the round was split
    sk = np.full(n, d_fail, dtype=np.uint32)
    # one byte: a candidate per launch, and the round stops at the launch that holds the hit
    monkeypatch.setenv("DEMI_INTMIN_KEPT_BYTES", "1")
    sk[n // 2] = d_ok
    res = _check_round(ctx, sk, lim, n_rec)
    assert res.first_hit == n // 2 and res.launches == n // 2 + 1


# ------------------------------------------------------------------ 2. the loop against the sequential reference
@pytest.mark.parametrize("max_batch", [1, 7, 0])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
@pytest.mark.parametrize("skip", [0, 1])
def test_native_loop_equals_the_sequential_reference(oracle, skip, strategy, max_batch):
    model, trace, fp = workload(oracle, skip)
    ctx = fresh(model)
    try:
        st = check_native_loop(ctx, oracle, skip, model, trace, fp, strategy, max_batch)
        assert st.retried == 0 and st.launches == st.rounds            # one replay launch per round
        assert st.adoptions > 0 and st.deliveries_after < st.deliveries_before
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. capacity
def test_a_capacity_before_the_hit_is_evaluated_again(oracle):
    """A pending set so small that a proposal BEFORE the round's first hit aborts (found with the oracle, and asserted): the
    round answers what it answers with the largest pending set, and so does the loop, with retried > 0."""
    model, trace, fp = workload(oracle, 1)
    cands = np.array([i for i, k, _ in IM.deliveries(trace) if model.msg_class[k[2][0]] != T.MSG_EXTERNAL], dtype=np.uint32)
    full = oracle.sts_removal_batch(model, trace.original_externals, trace.events, cands, limits(fp, T.MAX_PENDING))
    assert not (full["flags"] & OVF).any()
    first = int(np.nonzero(full["flags"] & T.V_VIOLATION)[0][0])
    assert first > 0
    p_small = None
    for p in range(16, 0, -1):
        small = oracle.sts_removal_batch(model, trace.original_externals, trace.events, cands, limits(fp, p))
        if (small["flags"][:first] & OVF).any():
            p_small = p
            break
    assert p_small is not None, "no pending capacity makes a proposal before the first hit abort"
    ctx = fresh(model)
    try:
        ctx.replay_load(trace.original_externals, trace.events)
        g = ctx.replay_removal_batch(cands, limits(fp, p_small))
        assert (g["flags"][:first] & OVF).any()                         # the overflow really happens on the device
        big, big_kept = ctx.replay_removal_round(cands, limits(fp, T.MAX_PENDING))
        res, kept = ctx.replay_removal_round(cands, limits(fp, p_small))
        assert res.first_hit == big.first_hit == first and bytes(res.verdict) == bytes(big.verdict) and kept.tobytes() == big_kept.tobytes()
        assert res.retried > 0 and res.launches == 2 and big.retried == 0
        for strategy in sorted(STRATEGIES):
            st = check_native_loop(ctx, oracle, 1, model, trace, fp, strategy, 0, lim=limits(fp, p_small))
            assert st.retried > 0 and st.launches > st.rounds
    finally:
        ctx.close()


def _beyond_case(oracle):
    """tests/test_limits_gpu._k2_beyond_cases 'fx': the recorded execution [Start, Arm, WaitQuiescence, Kick] runs 8 effect rows in
    Kick; without the Arm's delivery a ninth runs - DEMI_V_QUEUE_OVF whatever the pending capacity."""
    from .test_limits_gpu import _k2_beyond_cases
    name, model, ev, mm = _k2_beyond_cases()[0]
    ov, rec, _ = oracle.random_execute(model, ev, 5, T.Limits(mm, 0, 64, 0, 0, 0))
    assert not int(ov.flags) & OVF
    return model, ev, rec


def test_a_capacity_that_stays_is_an_error_by_name(oracle):
    model, ev, rec = _beyond_case(oracle)
    lim = T.Limits(0, 0, 64, 1, 0x1000103, 0)
    ctx = fresh(model)
    try:
        # the round: the proposal that drops the Arm's delivery aborts with every pending set
        ctx.replay_load(ev, rec)
        arm_id = int(rec["id"][(rec["kind"] == T.REC_MSG_SEND) & (rec["ext_idx"] == 1)][0])
        arm = int(np.nonzero((rec["kind"] == T.REC_MSG_EVENT) & (rec["id"] == arm_id))[0][0])
        assert int(ctx.replay_removal_batch([arm], T.Limits(0, 0, T.MAX_PENDING, 1, 0x1000103, 0))[0]["flags"]) & T.V_QUEUE_OVF
        with pytest.raises(_native.DemiError, match="capacities") as e:
            ctx.replay_removal_round([arm], lim)
        assert e.value.code == T.ERR_CAPACITY
        # the loop: the execution re-based on [Start, WaitQuiescence, Kick] - every proposal of it runs the ninth row
        keep = ~(((rec["kind"] == T.REC_MSG_SEND) | (rec["kind"] == T.REC_MSG_EVENT)) & (rec["id"] == arm_id))
        sub = EventTrace(rec, ev)
        based = IM.executed_trace(sub, keep, subseq=[0, 2, 3])
        ctx.replay_load(based.original_externals, based.events)
        pings = np.array([i for i, k, _ in IM.deliveries(based) if model.msg_class[k[2][0]] == T.MSG_INTERNAL], dtype=np.uint32)
        assert len(pings) and (ctx.replay_removal_batch(pings, T.Limits(0, 0, T.MAX_PENDING, 1, 0x1000103, 0))["flags"] & T.V_QUEUE_OVF).all()
        with pytest.raises(_native.DemiError, match="capacities") as e:
            ctx.minimize_internals(lim)
        assert e.value.code == T.ERR_CAPACITY
        assert ctx.replay_removal_batch([NO_SKIP], lim) is not None      # the context still holds a loaded execution
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. other layouts
def _layout_case(oracle, model, events, lim, seed_index_of):
    """A violating execution of a compiled-only table as the loaded execution (all its externals kept), and its fingerprint."""
    l0 = T.Limits(lim.max_messages, lim.invariant_check_interval, lim.p_max, 0, 0, 0)
    v = oracle.random_explore(model, events, 4000, seed_base=0x5EED0000, limits=l0, n_threads=min(16, os.cpu_count() or 1))
    hits = np.nonzero((v["flags"] & T.V_VIOLATION) != 0)[0]
    assert len(hits)
    vv, rec, _ = oracle.random_execute(model, events, 0x5EED0000 + int(hits[seed_index_of]), l0)
    return EventTrace(rec, events), ViolationFingerprint(vv.fingerprint)


def _check_layout(oracle, name, model, trace, fp, p_max):
    cfg = SchedulerConfig(model=model)
    seq = IM.STSSchedMinimizer(trace.original_externals, trace, fp, IM.LeftToRightOneAtATime(trace, model), OracleRemoval(oracle, model), max_batch=1)
    seq_stats, seq_out = seq.minimize()
    if IM.countMsgEvents(seq_out) == IM.countMsgEvents(trace):
        pytest.skip("%s: the violating execution has no removable delivery" % name)
    orc = IM.StsRemovalOracle(cfg, p_max=p_max)
    try:
        mirror = IM.STSSchedMinimizer(trace.original_externals, trace, fp, IM.LeftToRightOneAtATime(trace, model), orc)
        m_stats, m_out = mirror.minimize()                              # the Python mirror on the GPU
        n_stats, n_out = IM.minimizeInternals(cfg, trace.original_externals, trace, fp, oracle=orc, native=True)
        assert n_out.events.tobytes() == m_out.events.tobytes() == seq_out.events.tobytes()
        assert n_stats.total_replays == m_stats.total_replays == seq_stats.total_replays
        assert orc.native_sizes == mirror.internal_sizes == seq.internal_sizes and orc.native_batches == mirror.batches
        # the oracle's cache is not trusted after the native call: the next replay of the ORIGINAL trace is the original's
        assert orc.test_removals(trace, [NO_SKIP], fp) == [True]
    finally:
        orc.shutdown()


def test_wide_table(oracle):
    """A DEMI_MODEL_WIDE table (tests/test_wide_gpu.py's raft with terms above 255: 16-bit payloads in the delivery key)."""
    from demi_amd import model as M
    _, events, lim = raft5_config2()
    model = M.raft_model(5, term0=1000, loglen0=300)
    trace, fp = _layout_case(oracle, model, events, lim, 0)
    assert int(trace.events["p0"].max()) >= 1000
    _check_layout(oracle, "wide", model, trace, fp, 64)


def test_table_of_more_than_eight_actors(oracle):
    """The BIG layout (tests/test_big_gpu.py's raft of 11 nodes): deadLetters is 31."""
    from demi_amd.apps import raft11_config2
    model, events, lim = raft11_config2()
    trace, fp = _layout_case(oracle, model, events, lim, 0)
    snd = trace.events["snd"][trace.events["kind"] == T.REC_MSG_EVENT]
    assert int(snd.max()) == T.DEADLETTERS_BIG
    _check_layout(oracle, "big", model, trace, fp, 64)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_by_name(oracle):
    model, trace, fp = workload(oracle, 0)
    ctx = fresh(model)
    try:
        lim = limits(fp)
        for call in (lambda l: ctx.minimize_internals(l), lambda l: ctx.replay_removal_round([NO_SKIP], l)):
            with pytest.raises(_native.DemiError, match="demi_replay_load must precede") as e:
                call(lim)
            assert e.value.code == T.ERR_NO_TRACE
        ctx.replay_load(trace.original_externals, trace.events)
        for call in (lambda l: ctx.minimize_internals(l), lambda l: ctx.replay_removal_round([NO_SKIP], l)):
            with pytest.raises(_native.DemiError, match="looking_for_valid") as e:
                call(T.Limits(0, 0, 64, 0, fp.code, 0))
            assert e.value.code == T.ERR_INVALID_ARG
        with pytest.raises(_native.DemiError, match="unknown removal strategy 7"):
            ctx.minimize_internals(lim, T.IntminParams(7, 0))
        not_a_delivery = int(np.nonzero(trace.events["kind"] != T.REC_MSG_EVENT)[0][0])
        with pytest.raises(_native.DemiError, match="not a delivery of the loaded trace"):
            ctx.replay_removal_round([not_a_delivery], lim)
        gather = _native.ALLGATHER_FN(lambda user, send, recv, nbytes: 0)
        assert _native.lib().demi_comm_create_host(ctx._h, 0, 1, gather, None) == 0
        with pytest.raises(_native.DemiError, match="single rank") as e:
            ctx.minimize_internals(lim)
        assert e.value.code == T.ERR_INVALID_ARG
        assert _native.lib().demi_comm_destroy(ctx._h) == 0
        # a buffer below the result's length: DEMI_ERR_CAPACITY with the length needed, and the minimized execution is loaded
        total, want, _, _ = sequential(oracle, 0, model, trace, fp, "LeftToRight")
        with pytest.raises(_native.DemiError, match="has %d events" % len(want.events)) as e:
            ctx.minimize_internals(lim, cap=len(want.events) - 1)
        assert e.value.code == T.ERR_CAPACITY
        v = ctx.replay_removal_batch([NO_SKIP], lim)[0]
        assert int(v["flags"]) & T.V_VIOLATION and T.verdict_deliveries(int(v["flags"])) == IM.countMsgEvents(want)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. the Python entry points
def test_python_entry_points_return_what_their_default_paths_return(oracle):
    from demi_amd.runner_utils import run_the_gamut
    model, events, lim = raft5_config2()
    _, trace, fp = workload(oracle, 0)
    cfg = SchedulerConfig(model=model)
    for strategy in sorted(STRATEGIES):
        ctor = lambda: STRATEGIES[strategy][0](trace, model)
        s0, t0 = IM.minimizeInternals(cfg, trace.original_externals, trace, fp, removalStrategyCtor=ctor)
        s1, t1 = IM.minimizeInternals(cfg, trace.original_externals, trace, fp, removalStrategyCtor=ctor, native=True)
        assert t0.events.tobytes() == t1.events.tobytes() and s0.total_replays == s1.total_replays > 0
        assert (t0.original_externals == t1.original_externals).all()
    vv, rec, used = _violating_execution(oracle, model, events, lim, 0)
    a = run_the_gamut(cfg, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint))
    b = run_the_gamut(cfg, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint), native_intmin=True)
    assert a["mcs"] == b["mcs"] and a["intmin_replays"] == b["intmin_replays"] and a["minimized_deliveries"] == b["minimized_deliveries"]
    assert a["minimized"].events.tobytes() == b["minimized"].events.tobytes()
