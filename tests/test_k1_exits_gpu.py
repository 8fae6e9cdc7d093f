"""K1's rare events and the path of every delivery: one countdown stands for "this count is a checkpoint or the first one beyond
max_messages" in the kernels compiled for a table (the interpreter keeps its counters); the capacity exits and the per-delivery hit bit, which two other steps of that section would
have rewritten and which stay as they were, are held by the cases those steps were built against.  Bit for bit against the CPU
oracle: 256 .. 1 024 schedules per case on hand-built 3 - 5 actor tables, the table interpreter and the compiled kernel,
FullyRandom and SrcDstFIFO, the plain and the recording kernel.

  overflow  every site as the FIRST overflow of an execution, each capacity from both sides (exactly reached: no flag; one
            more: the flag): p_max in the middle of an injected batch of 16, 17 and 30 Sends; at the timer append of the step;
            at the 2nd and at the 4th of the 4 receivers of a BCAST; DEMI_TQ_CAP / DEMI_RESEND_CAP at enqueue_timer, the
            re-entry of timersToResend and DEMI_FX_CAP inside a handler (the tables of tests/test_k1_diet_gpu.py); a delivery
            whose timer slot hits the queue capacity and whose later BCAST would hit p_max - the verdict carries the first flag
            only, and no verdict of any case carries both.
  limits    max_messages in {0, 1, 29, 30, 31, the longest execution's delivery count, that + 1} x interval in {0, 1, 2, 30}; a
            violation first visible at a checkpoint, one visible only at the finish, a checkpoint that coincides with
            count == max_messages + 1 (MAXMSG, no violation); a carried instance of 3 executions; MULTI and TESTS launches;
            SPREAD with 1 and 5 lanes.
  hits      the path that recomputes the receiver's bit of the invariant's hit mask after every delivery, which stays as it
            was: the field written on a rarely taken branch, twice in one handler, with the value it had, by no row of a
            handler; initial states with one and two hits; a DEMI_INV_PEERS program; raft3 / raft5 at 1 024."""
import functools
import os

import numpy as np
import pytest

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.apps import raft3_config1, raft5_config2
from demi_amd.fuzzer import events_to_array, send, start, wait_quiescence
from demi_amd.model import Asm, build_model

from .test_k1_diet_gpu import GO, KICK, MSGS, NO_INV, PING, RT, T1, T2, _capacity_cases, _hits_model, _peers_program, _trace
from .test_k1_gpu import assert_same
from .test_limits_gpu import _fresh, _lim, _same_trace

pytestmark = pytest.mark.gpu

SEED = 4711
CPUS = min(16, os.cpu_count() or 1)
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF


# ---------------------------------------------------------------------------------------------------------------- overflow
def _kick_model(n_actors):
    """Kick(0) counts; Kick(1) sets T1; Kick(2) sets T1 and T2 (two timer appends in the next step); Kick(3) broadcasts a Ping to
    the other actors; Kick(4) sets the one-shot RT and then broadcasts.  Pings and timers count."""
    kick = (Asm().add(M.F[0], M.F[0], 1).if_eq(M.P0, 1, "a").tset(T1).label("a").if_eq(M.P0, 2, "b").tset(T1).tset(T2).label("b")
            .if_eq(M.P0, 3, "c").bcast(PING, M.P1, 0).label("c").if_eq(M.P0, 4, "d").tset(RT).bcast(PING, M.P1, 0).label("d"))
    h = {(0, "Kick"): kick, (0, "Ping"): Asm().add(M.F[1], M.F[1], 1), (0, "T1"): Asm().add(M.F[2], M.F[2], 1),
         (0, "T2"): Asm().add(M.F[3], M.F[3], 1), (0, "RT"): Asm().add(M.F[4], M.F[4], 1),
         (0, "Go"): Asm().trep(T1).trep(T2).skipz(M.P0, "x").trep(RT).label("x")}
    return build_model("exits_kick%d" % n_actors, n_actors, MSGS, h, [[0] * 8] * n_actors, NO_INV)


def _batch(n_actors, p0s):
    return events_to_array([start(a) for a in range(n_actors)] + [send(i % n_actors, KICK, p0, i) for i, p0 in enumerate(p0s)])


def _overflow_cases():
    """{name: (model, events, limits, schedules, expectation on the oracle's flags)}; the expectation is (flag every execution
    carries | None, flag some execution carries | None)"""
    c = {}
    m3, m5 = _kick_model(3), _kick_model(5)
    # p_max in the middle of an injected batch: n Sends fit p_max = n (a Kick(0) sends nothing), not p_max = n - 1
    for n in (16, 17, 30):
        for p_max, flag in ((n, None), (n - 1, T.V_PENDING_OVF)):
            c["batch%d-p%d" % (n, p_max)] = (m3, _batch(3, [0] * n), T.Limits(0, 0, p_max, 0, 0, 0), 256, (flag, flag) if flag else (0, None))
    # the timer append of the step: 12 Sends, p_max 12.  One Kick(1) first: 11 + 1 timer fit exactly; one Kick(2) first: 11 + 2 do not
    c["timer-append-fits"] = (m3, _batch(3, [1] + [0] * 11), T.Limits(0, 0, 12, 0, 0, 0), 256, (0, None))
    c["timer-append-over"] = (m3, _batch(3, [2] + [0] * 11), T.Limits(0, 0, 12, 0, 0, 0), 512, (None, T.V_PENDING_OVF))
    # the receivers of a BCAST: 10 Sends, one of them Kick(3) on a 5-actor table: 9 + 4 when it is delivered first
    for p_max, some in ((13, None), (12, T.V_PENDING_OVF), (10, T.V_PENDING_OVF)):      # fits exactly / the 4th / the 2nd receiver
        c["bcast-p%d" % p_max] = (m5, _batch(5, [3] + [0] * 9), T.Limits(0, 0, p_max, 0, 0, 0), 512, (0, None) if some is None else (None, some))
    # the timer queues and the effect queue (tests/test_k1_diet_gpu.py has the tables' stories)
    for name, model, ev, lim, ovf in _capacity_cases(3):
        c["queue-" + name] = (model, ev, lim, 256, (T.V_QUEUE_OVF, T.V_QUEUE_OVF) if ovf else (0, None))
    # QUEUE_OVF in an earlier slot, a BCAST that would overflow p_max in a later one.  Batch 1: three Go arm 3 + 3 + 2 repeating
    # timers, every one is delivered once and parked in timersToResend.  Batch 2: Kick(4) and 9 Kick(0), p_max 10.  When Kick(4)
    # is the batch's first delivery the 8 parked timers re-enter messagesToSend at its pick - exactly DEMI_TQ_CAP - its RT set
    # finds the queue full (DEMI_V_QUEUE_OVF) and its BCAST would append 2 to the 9 pending: the verdict is the queue flag alone.
    # When a Kick(0) is first, the next step appends 8 timers to 9 pending: DEMI_V_PENDING_OVF alone.
    arms = [start(a) for a in range(3)] + [send(0, GO, 1), send(1, GO, 1), send(2, GO, 0), wait_quiescence()]
    ev = events_to_array(arms + [send(2, KICK, 4, 0)] + [send(i % 3, KICK, 0, i) for i in range(9)])
    c["queue-then-send"] = (m3, ev, T.Limits(0, 0, 10, 0, 0, 0), 512, (None, T.V_QUEUE_OVF))
    return c


# ------------------------------------------------------------------------------------------------------------------ limits
def _limit_model():
    """Four actors, F0 == 1 is the hit, at most one may.  Go(1) makes the receiver a hit, Go(2) takes it back, Go(0) pings the next
    actor."""
    go = (Asm().if_eq(M.P0, 1, "a").mov(M.F[0], 1).label("a").if_eq(M.P0, 2, "b").mov(M.F[0], 0).label("b")
          .if_eq(M.P0, 0, "c").add(M.T0, M.ME, 1).and_(M.T0, M.T0, 3).send(PING, M.T0, M.T1, 0).label("c"))
    h = {(0, "Go"): go, (0, "Ping"): Asm().add(M.F[2], M.F[2], 1)}
    return build_model("exits_limit", 4, MSGS, h, [[0] * 8] * 4, (T.INV_AT_MOST_ONE, 0, 1, 1))


# (receiver, p0) of 20 Go's in three batches.  Actors 0 and 1 each get a Go(1) and a Go(2) in the first batch, actors 2 and 3 in the
# last: an actor ends a batch as a hit when its Go(1) came second, so two hits exist at the end of batch 1 in a quarter of the
# executions (a checkpoint sees them), and otherwise may arise in the last batch (counts 24 .. 32), for some executions only beyond
# the checkpoint at 30: visible at the finish alone.  12 Go(0) ping: 32 deliveries.
LIMIT_TRACE = ([(0, 1), (2, 0), (0, 2), (1, 1), (3, 0), (1, 2), (2, 0)], [(a % 4, 0) for a in range(7)],
               [(2, 1), (0, 0), (2, 2), (3, 1), (1, 0), (3, 2)])


def _limit_events():
    ev = [start(a) for a in range(4)]
    for b, batch in enumerate(LIMIT_TRACE):
        ev += [wait_quiescence()] * (b != 0) + [send(a, GO, p0, 0) for a, p0 in batch]
    return events_to_array(ev)


_GOS = [g for batch in LIMIT_TRACE for g in batch]
LONGEST = len(_GOS) + sum(1 for _, p0 in _GOS if p0 == 0)          # an execution that runs to the end delivers every Go and every Ping
# (0xFFFFFFFF: the largest limit the interface takes - max_messages + 1 does not fit 32 bits)
MAX_MESSAGES = (0, 1, 29, 30, 31, LONGEST, LONGEST + 1, 0xFFFFFFFF)
INTERVALS = (0, 1, 2, 30)


# -------------------------------------------------------------------------------------------------------------------- hits
def _field_writes_model(n_hit):
    """The invariant's field F0 written on a rarely taken branch (Go(1): only when F3 reached 2), twice in one handler (Go(2): 1,
    then back to what P1 says), with the value it already had (Go(3)), by no row (Go(0): a Ping to the next actor)."""
    go = (Asm().add(M.F[3], M.F[3], 1).if_eq(M.P0, 1, "a").if_ge(M.F[3], 2, "a").mov(M.F[0], 1).label("a")
          .if_eq(M.P0, 2, "b").mov(M.F[0], 1).mov(M.F[0], M.P1).label("b")
          .if_eq(M.P0, 3, "c").mov(M.F[0], M.F[0]).label("c")
          .if_eq(M.P0, 0, "d").add(M.T0, M.ME, 1).and_(M.T0, M.T0, 3).send(PING, M.T0, M.T1, 0).label("d"))
    h = {(0, "Go"): go, (0, "Ping"): Asm().add(M.F[2], M.F[2], 1)}
    init = [[1 if a < n_hit else 0] + [0] * 7 for a in range(4)]
    return build_model("exits_writes%d" % n_hit, 4, MSGS, h, init, (T.INV_AT_MOST_ONE, 0, 1, 1))


@functools.lru_cache(maxsize=None)
def _cases():
    """{name: (model, events, limits, schedules, (flag of every execution | None, flag of some execution | None) | None)}"""
    c = dict(_overflow_cases())
    lm, lev = _limit_model(), _limit_events()
    for mm in MAX_MESSAGES:
        for iv in INTERVALS:
            c["limit-m%d-i%d" % (mm, iv)] = (lm, lev, T.Limits(mm, iv, 64, 0, 0, 0), 256, None)
    c["limit-carry"] = (lm, lev, T.Limits(30, 2, 64, 0, 0, 0, 0, 0, 3), 510, None)
    for n_hit in (0, 1, 2):
        c["writes-%d" % n_hit] = (_field_writes_model(n_hit), _trace(41 + n_hit, 4, [0, 0, 1, 1, 2, 3], 18, 0.15), T.Limits(60, 3, 64, 0, 0, 0), 512, None)
    c["writes-peers"] = (_hits_model(1, (T.INV_NEVER, _peers_program())), _trace(45, 4, [0, 0, 1, 2], 18, 0.15), T.Limits(60, 3, 64, 0, 0, 0), 256, None)
    for name, (model, ev, lim) in (("raft3", raft3_config1()), ("raft5", raft5_config2())):
        c[name] = (model, ev, lim, 1024, None)
    return c


NAMES = (["batch%d-p%d" % (n, p) for n in (16, 17, 30) for p in (n, n - 1)] + ["timer-append-fits", "timer-append-over", "bcast-p13", "bcast-p12", "bcast-p10"] +
         ["queue-" + s for s in ("tset8", "tset9", "trep1+6+1", "trep1+7+1", "resend9", "resend8-reenter+0", "resend8-reenter+1")] + ["queue-then-send"] +
         ["limit-m%d-i%d" % (mm, iv) for mm in MAX_MESSAGES for iv in INTERVALS] + ["limit-carry"] +
         ["writes-0", "writes-1", "writes-2", "writes-peers", "raft3", "raft5"])
_WANT = {}


def _want(oracle, name, fifo):
    """The oracle's verdicts of a case, computed once and shared by the interpreted and the compiled run."""
    if (name, fifo) not in _WANT:
        model, ev, lim, n = _cases()[name][:4]
        l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
        w = oracle.random_explore(model, ev, n, seed_base=SEED, limits=l, n_threads=CPUS)
        w.setflags(write=False)
        _WANT[(name, fifo)] = w
    return _WANT[(name, fifo)]


def test_the_cases_are_the_ones_listed():
    assert sorted(_cases()) == sorted(NAMES)


@pytest.mark.parametrize("specialise", [False, True], ids=["interpreted", "compiled"])
@pytest.mark.parametrize("name", NAMES)
def test_exit_paths_equal_the_oracle(oracle, monkeypatch, name, specialise):
    model, ev, lim, n, expect = _cases()[name]
    ctx = _fresh(model, ev, specialise)
    try:
        for fifo in (False, True):
            l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
            want = _want(oracle, name, fifo)
            # an overflowed execution's verdict is its FIRST flag alone
            assert ((want["flags"] & OVF) != OVF).all(), (name, "oracle: both flags")
            if expect is not None:
                every, some = expect
                if every is not None:
                    assert ((want["flags"] & OVF) == every).all(), (name, "oracle", every)
                if some is not None:
                    assert ((want["flags"] & OVF) == some).any(), (name, "oracle", some)
            assert_same(ctx.random_explore(n, l, seed_base=SEED), want)                                # REC off
            if lim.executions_per_instance <= 1:
                for s in (SEED, SEED + 1):                                                               # REC on
                    _same_trace(ctx.random_get_trace(s, l), oracle.random_execute(model, ev, s, l))
        if name.startswith(("batch", "limit-m30-", "limit-m31-")):
            # SPREAD: the executions on the first 1 or 5 lanes of each wave
            for lanes in ("1", "5"):
                monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", lanes)
                assert_same(ctx.random_explore(70, lim, seed_base=SEED), _want(oracle, name, False)[:70])
            monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE")
    finally:
        ctx.close()


def test_the_limit_table_reaches_what_it_is_built_for(oracle):
    """On the oracle: with no limit an execution delivers LONGEST messages unless it violates before; interval 1 finds violations
    at checkpoints (count below LONGEST); interval 0 finds the ones that last to the finish and only those, so fewer; with
    max_messages 29 and interval 30 - the checkpoint coincides with count == max_messages + 1 - every execution that gets there
    carries MAXMSG and no violation, while interval 2 does find violations before it; the carried instance's second execution
    differs from a fresh run of that index and still checks at ITS count 2, 4, ..."""
    def flags(name):
        return _want(oracle, name, False)
    free, fin = flags("limit-m0-i1"), flags("limit-m0-i0")
    count = lambda w: (w["flags"] >> 16) & 0xFFFF
    viol = lambda w: (w["flags"] & T.V_VIOLATION) != 0
    assert count(fin).max() == LONGEST and (count(fin) == LONGEST).all()
    assert viol(free).any() and (count(free)[viol(free)] < LONGEST).any()
    assert viol(fin).sum() < viol(free).sum()
    # interval 30: some executions violate at the checkpoint of count 30, some only at the finish (count LONGEST, past the checkpoint)
    late = flags("limit-m0-i30")
    assert (viol(late) & (count(late) == 30)).any() and (viol(late) & (count(late) == LONGEST)).any()
    # the largest limit is no limit: the verdicts of max_messages 0 (which means 0x7FFFFFFF), checkpoints included
    for iv in INTERVALS:
        assert (flags("limit-m%d-i%d" % (0xFFFFFFFF, iv)) == flags("limit-m0-i%d" % iv)).all()
    assert viol(flags("limit-m%d-i2" % 0xFFFFFFFF)).any()
    co = flags("limit-m29-i30")
    assert ((co["flags"] & T.V_MAXMSG) != 0).all() and not viol(co).any() and (count(co) == 30).all()
    assert viol(flags("limit-m29-i2")).any()
    # one more message allowed: the checkpoint at 30 is a checkpoint
    assert (viol(flags("limit-m30-i30")) | ((flags("limit-m30-i30")["flags"] & T.V_MAXMSG) != 0)).all()
    carry = flags("limit-carry")
    model, ev, lim = _cases()["limit-carry"][:3]
    fresh = oracle.random_explore(model, ev, 510, seed_base=SEED, limits=_lim(lim, executions_per_instance=1), n_threads=CPUS)
    assert (carry[0::3] == fresh[:170]).all() and (carry[1::3] != fresh[1:171]).any()


@pytest.mark.parametrize("specialise", [False, True], ids=["interpreted", "compiled"])
def test_candidate_and_test_launches_count_down_per_execution(oracle, specialise):
    """MULTI (random_explore_candidates) and TESTS (random_explore_tests): every lane runs one execution of its workgroup's trace,
    with the limit and the checkpoints of the launch - max_messages 9 with interval 2 and 5, so that executions end at a
    checkpoint, at the limit, and at a checkpoint that coincides with the limit (count 10 with interval 5)."""
    model, full = _limit_model(), _limit_events()
    n_ev = len(full)
    keeps = [list(range(n_ev)), [i for i in range(n_ev) if i % 5 != 4], list(range(4)) + list(range(8, n_ev)), list(range(12))]
    execs = 64
    ctx = _fresh(model, full, specialise)
    try:
        for interval in (2, 5):
            lim = T.Limits(9, interval, 64, 0, 0, 1)
            masks = np.zeros((len(keeps), 4), dtype=np.uint64)
            for i, k in enumerate(keeps):
                masks[i, 0] = sum(1 << j for j in k)
            gv, _ = ctx.random_explore_candidates(masks, execs, lim, seed_base=SEED)
            tv, _ = ctx.random_explore_tests([full[k] for k in keeps], execs, lim, seed_base=SEED)
            for i, k in enumerate(keeps):
                c = oracle.random_explore(model, full[k], execs, seed_base=SEED, limits=lim, n_threads=CPUS)
                assert_same(gv[i], c)
                assert_same(tv[i], c)
    finally:
        ctx.close()
