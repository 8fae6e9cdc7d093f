"""The capacity rule at the sites no other test reaches: a replay aborted on a capacity (DEMI_V_PENDING_OVF / DEMI_V_QUEUE_OVF) is
no verdict - it is run once more with the largest pending set, and what the caller gets is the answer at the largest pending set.
demi_ddmin, STSScheduler, StsRemovalOracle, StsWildcardOracle and demi_random_ddmin, each under a pending set so small that a
replay it consults aborts: the capacity is found with the CPU oracle (and asserted to exist), the abort is asserted on the device,
and the answers are held against the same call at DEMI_MAX_PENDING, where the CPU oracle shows that nothing aborts."""
import os

import numpy as np
import pytest

from demi_amd import _native, types as T
from demi_amd import internal_minimization as IM
from demi_amd import wildcard_minimization as W
from demi_amd.apps import SEED_BASE
from demi_amd.minification import DDMin, UnmodifiedEventDag, events_to_masks
from demi_amd.schedulers import STSScheduler, SchedulerConfig

from . import test_wildcard_transliteration_cpu as X
from . import wcmin_cases as Wc
from . import wildcard_payload_cases as Pc
from .test_intmin_native_gpu import workload
from .test_random_ddmin_gpu import _OracleRandomScheduler, _failing_execution

pytestmark = pytest.mark.gpu
EMU = os.environ.get("DEMI_EMU") == "1"
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
_cache = {}


def limits(fp, p_max):
    return T.Limits(0, 0, p_max, 1, fp.code, 0)


def _same_trace(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.events.tobytes() == b.events.tobytes()
                                         and a.original_externals.tobytes() == b.original_externals.tobytes())


# ------------------------------------------------------------------ demi_ddmin and STSScheduler: the candidates DDMin consults
def _ddmin_case(oracle):
    """(model, trace, fp, what oracle.ddmin answers at 128, its consulted masks, the largest p in 16..1 at which one of them aborts)"""
    if "ddmin" not in _cache:
        model, trace, fp = workload(oracle, 1)
        want = oracle.ddmin(model, trace.original_externals, trace.events, limits(fp, T.MAX_PENDING))
        masks = events_to_masks([c for c, _ in want[1]])
        assert not (oracle.sts_replay_batch(model, trace.original_externals, trace.events, masks, limits(fp, T.MAX_PENDING))["flags"] & OVF).any()
        p_small = None
        for p in range(16, 0, -1):
            if (oracle.sts_replay_batch(model, trace.original_externals, trace.events, masks, limits(fp, p))["flags"] & OVF).any():
                p_small = p
                break
        assert p_small is not None, "no pending capacity makes a consulted candidate abort"
        _cache["ddmin"] = (model, trace, fp, want, masks, p_small)
    return _cache["ddmin"]


def test_ddmin_under_a_small_pending_set(oracle):
    model, trace, fp, want, masks, p = _ddmin_case(oracle)
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        ctx.replay_load(trace.original_externals, trace.events)
        assert (ctx.replay_batch(masks, limits(fp, p))["flags"] & OVF).any()          # the abort really happens on the device
        big = ctx.ddmin(limits(fp, T.MAX_PENDING))
        small = ctx.ddmin(limits(fp, p))
        for got in (big, small):
            assert tuple(got[0]) == tuple(want[0])
            assert [(tuple(c), ps) for c, ps in got[1]] == [(tuple(c), ps) for c, ps in want[1]]
        assert small[2] == big[2] and small[3].consultations == big[3].consultations and small[3].verified == big[3].verified
    finally:
        ctx.close()


def test_sts_scheduler_under_a_small_pending_set(oracle):
    model, trace, fp, want, masks, p = _ddmin_case(oracle)
    subseqs = [tuple(c) for c, _ in want[1]]
    aborted = oracle.sts_replay_batch(model, trace.original_externals, trace.events, masks, limits(fp, p))["flags"] & OVF
    probes = [subseqs[int(np.nonzero(aborted)[0][0])], tuple(range(len(trace.original_externals)))]
    answers = []
    for p_max in (p, T.MAX_PENDING):
        sts = STSScheduler(SchedulerConfig(model=model), trace, p_max=p_max)
        try:
            if p_max == p:
                assert (sts._ctx.replay_batch(masks, limits(fp, p))["flags"] & OVF).any()
            answers.append((sts.test_batch(subseqs, fp), sts.verdicts(subseqs, fp).tobytes(), [sts.executed_trace(s, fp) for s in probes]))
        finally:
            sts.shutdown()
    (batch_s, v_s, ex_s), (batch_b, v_b, ex_b) = answers
    assert batch_s == batch_b == [not ps for _, ps in want[1]] and v_s == v_b
    assert all(_same_trace(a, b) for a, b in zip(ex_s, ex_b)) and ex_b[1] is not None


# ------------------------------------------------------------------ StsRemovalOracle
def test_removal_oracle_under_a_small_pending_set(oracle):
    """The candidates and the capacity of tests/test_intmin_native_gpu.py::test_a_capacity_before_the_hit_is_evaluated_again."""
    model, trace, fp = workload(oracle, 1)
    cands = np.array([i for i, k, _ in IM.deliveries(trace) if model.msg_class[k[2][0]] != T.MSG_EXTERNAL], dtype=np.uint32)
    full = oracle.sts_removal_batch(model, trace.original_externals, trace.events, cands, limits(fp, T.MAX_PENDING))
    assert not (full["flags"] & OVF).any()
    first = int(np.nonzero(full["flags"] & T.V_VIOLATION)[0][0])
    p_small, deep = None, None
    for p in range(16, 0, -1):
        small = oracle.sts_removal_batch(model, trace.original_externals, trace.events, cands, limits(fp, p))
        if (small["flags"][:first] & OVF).any():
            p_small, deep = p, int(np.nonzero(small["flags"] & OVF)[0][0])
            break
    assert p_small is not None, "no pending capacity makes a proposal before the first hit abort"
    answers = []
    for p_max in (p_small, T.MAX_PENDING):
        orc = IM.StsRemovalOracle(SchedulerConfig(model=model), p_max=p_max)
        try:
            if p_max == p_small:
                orc._load(trace)
                assert int(orc._ctx.replay_removal_batch(cands, limits(fp, p_small))["flags"][deep]) & OVF
            answers.append((orc.test_removals(trace, cands, fp), [orc.executed(trace, int(cands[k]), fp) for k in (deep, first)]))
        finally:
            orc._ctx.close()
    (rem_s, ex_s), (rem_b, ex_b) = answers
    assert rem_s == rem_b == [bool(f & T.V_VIOLATION) for f in full["flags"]]
    assert all(_same_trace(a, b) for a, b in zip(ex_s, ex_b)) and ex_b[0] is None and ex_b[1] is not None


# ------------------------------------------------------------------ StsWildcardOracle
def test_wildcard_oracle_under_a_small_pending_set(oracle):
    """The rows and the capacity of tests/test_wcmin_native_gpu.py::test_a_capacity_before_the_hit_is_evaluated_again."""
    from .test_wcmin_native_gpu import _pool
    name = "real3"
    model, trace, fp, _ = Wc.workload(oracle, name)
    (ts, po), rows = _pool(oracle, name)
    run = lambda row: Pc.run_candidate(oracle, model, trace, fp, X.wildcards_of(ts, po), row)
    outcome = [run(r) for r in rows[:72]]
    ok = [k for k, o in enumerate(outcome) if o[0][0] & T.V_VIOLATION]
    bad = [k for k, o in enumerate(outcome) if not o[0][0] & T.V_VIOLATION]
    assert ok and bad
    hit = min(ok, key=lambda k: outcome[k][4].max_pending)
    deep = max(bad, key=lambda k: outcome[k][4].max_pending)
    assert outcome[deep][4].max_pending > outcome[hit][4].max_pending, "no failing proposal holds more pending messages than a reproducing one"
    assert max(o[4].max_pending for o in outcome) <= T.MAX_PENDING                  # nothing aborts at the largest pending set
    p_small = outcome[deep][4].max_pending - 1
    r = np.array([rows[deep], rows[bad[0]], rows[hit], rows[deep]])
    answers = []
    for p_max in (p_small, T.MAX_PENDING):
        orc = W.StsWildcardOracle(SchedulerConfig(model=model), p_max=p_max)
        try:
            orc.load(trace, ts, po)
            if p_max == p_small:
                g = orc._ctx.replay_wildcard_batch(r, orc._limits(fp))
                assert int(g["flags"][0]) & OVF and not int(g["flags"][2]) & OVF    # the abort really happens on the device
            batch = orc.test_batch(r, fp)
            ex = [orc.executed(row, fp) for row in (r[0], r[2])]
            answers.append((batch, ex, orc.launches))
        finally:
            orc.shutdown()
    (batch_s, ex_s, launches_s), (batch_b, ex_b, launches_b) = answers
    assert batch_s == batch_b and batch_b[2] and not batch_b[0]
    assert ex_s[0] is None and ex_b[0] is None and ex_b[1] is not None
    assert _same_trace(ex_s[1][0], ex_b[1][0]) and ex_s[1][1] == ex_b[1][1]
    assert launches_b == 3 and launches_s == 5                                      # the batch and the first recorded replay ran twice


# ------------------------------------------------------------------ demi_random_ddmin
def test_random_ddmin_under_a_small_pending_set(oracle):
    """R = 16 executions per candidate; p is the largest capacity at which the CPU oracle shows a consulted candidate with an
    aborted execution and no violating one.  A verdict that does not overflow does not depend on p_max: the call at p answers
    what it answers at the largest pending set."""
    R = 16
    model, trace, fp, _ = _failing_execution(oracle, 200 if not EMU else 90)
    ext = trace.original_externals
    lim = lambda p: T.Limits(len(trace.events), 0, p, 1, fp.code, 0)
    ref = DDMin(_OracleRandomScheduler(oracle, model, ext, lim(T.MAX_PENDING), R, SEED_BASE), checkUnmodifed=False)
    want = ref.minimize(UnmodifiedEventDag(ext), fp).get_all_events()               # (asserts that nothing aborts at the largest pending set)
    consulted = [tuple(c) for c, _ in ref.consulted]

    def undecided(p):
        for c in consulted:
            f = oracle.random_explore(model, ext[list(c)], R, seed_base=SEED_BASE, limits=lim(p))["flags"]
            if (f & OVF).any() and not (f & T.V_VIOLATION).any():
                return True
        return False
    p_small = next((p for p in range(16, 0, -1) if undecided(p)), None)
    assert p_small is not None, "no pending capacity leaves a consulted candidate undecided"
    print("random ddmin: %d external events, p = %d" % (len(ext), p_small))
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        ctx.trace_load(ext)
        _, f = ctx.random_explore_candidates(events_to_masks(consulted), R, lim(p_small), seed_base=SEED_BASE)
        assert ((f & 3) == 2).any()                                                 # a candidate really is undecided on the device
        par = T.RandomDdminParams(R, 0, 256)
        big = ctx.random_ddmin(lim(T.MAX_PENDING), par, seed_base=SEED_BASE)
        small = ctx.random_ddmin(lim(p_small), par, seed_base=SEED_BASE)
        assert tuple(small[0]) == tuple(big[0]) == tuple(want)
        assert [(tuple(c), ps) for c, ps in small[1]] == [(tuple(c), ps) for c, ps in big[1]] == [(tuple(c), ps) for c, ps in ref.consulted]
        assert small[2] == big[2] and small[3].consultations == big[3].consultations and small[3].verified == big[3].verified
        assert small[3].replays > big[3].replays                                    # the undecided candidates ran again
    finally:
        ctx.close()
