"""K1 with commuting classes in the effect-slot schedule (jit.hpp fx_schedule): a timer-set row may be applied
before a send that precedes it in the program.  Bit for bit against the CPU oracle: 256 - 1 024 schedules per case, the table
interpreter and the compiled kernel, FullyRandom and SrcDstFIFO, the plain and the recording kernel (which keeps the effect queue).

  hand      the table of tests/test_fx_commute_cpu.py: [SEND, TSET X], [TSET X, SEND], [TSET X, SEND, TSET X], [SEND, TCANCEL X, TSET X]
  matrix    the capacity verdict of a delivery whose rows were re-ordered.  Kick(5) is [BCAST, TSET RT] - the TSET is moved below the
            send - and Kick(4) is [TSET RT, BCAST].  Three Go arm 7 / 8 / 9 repeating timers, every one is delivered once and parked
            in timersToResend; the next batch is the Kick and nine Kick(0).  When the Kick is the batch's first delivery the parked
            timers re-enter messagesToSend - DEMI_TQ_CAP - 1, exactly DEMI_TQ_CAP, or one more (which is the queue flag at the pick) -
            9 messages are pending and the BCAST appends 3: p_max 12 is exactly reached at the 3rd receiver; 11 at the 2nd and
            exceeded at the 3rd; 10 at the 1st and exceeded at the 2nd.  (Exceeded at the 1st cannot be built: the delivered Kick itself
            left the pending set.)  With the queue at its capacity Kick(5) reports DEMI_V_PENDING_OVF alone when its BCAST
            overflows - the program sends first - and DEMI_V_QUEUE_OVF alone when it fits; Kick(4) reports the queue flag alone
            whatever its BCAST would do.  No verdict of any case carries both flags.
  resend    a repeating timer whose handler is [TCANCEL RT, BCAST, TREP RT]: the TREP is moved below the BCAST and, the timer
            being in justScheduledTimers, goes to timersToResend.  (DEMI_RESEND_CAP and p_max cannot both be met by one such
            delivery: the parked timers only pile up while nothing else is delivered, which drains the pending set.)
  raft      raft3 / raft5 at 1 024 with the switch DEMI_JIT_NO_FX_COMMUTE off and on."""
import functools
import os

import numpy as np
import pytest

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.apps import raft3_config1, raft5_config2
from demi_amd.fuzzer import events_to_array, send, start, wait_quiescence
from demi_amd.model import Asm, build_model

from .test_fx_commute_cpu import KA, KB, KC, KD, _hand_model
from .test_k1_diet_gpu import GO, KICK, MSGS, NO_INV, PING, RT, T1, T2
from .test_k1_gpu import assert_same
from .test_limits_gpu import _fresh, _lim, _same_trace

pytestmark = pytest.mark.gpu

SEED = 2020
CPUS = min(16, os.cpu_count() or 1)
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF


def _hand_events(seed, n=24, quiesce=0.2):
    rng = np.random.default_rng(seed)
    ev = [start(a) for a in range(3)]
    for _ in range(n):
        ev.append(send(int(rng.integers(3)), int(rng.choice([KA, KB, KC, KD])), 0, int(rng.integers(4))))
        if rng.random() < quiesce:
            ev.append(wait_quiescence())
    return events_to_array(ev)


def _matrix_model():
    """Four actors.  Go arms the repeating T1 and T2 (and RT when p0 is set); Kick(5): [BCAST, TSET RT]; Kick(4): [TSET RT, BCAST]; any
    other Kick counts.  Pings and timers count."""
    kick = (Asm().add(M.F[0], M.F[0], 1).if_eq(M.P0, 5, "n5").bcast(PING, M.P1, 0).tset(RT).halt().label("n5")
            .if_eq(M.P0, 4, "n4").tset(RT).bcast(PING, M.P1, 0).label("n4"))
    h = {(0, "Kick"): kick, (0, "Ping"): Asm().add(M.F[1], M.F[1], 1), (0, "T1"): Asm().add(M.F[2], M.F[2], 1),
         (0, "T2"): Asm().add(M.F[3], M.F[3], 1), (0, "RT"): Asm().add(M.F[4], M.F[4], 1),
         (0, "Go"): Asm().trep(T1).trep(T2).skipz(M.P0, "x").trep(RT).label("x")}
    return build_model("fxc_matrix", 4, MSGS, h, [[0] * 8] * 4, NO_INV)


def _matrix_events(parked, kick):
    """`parked` repeating timers armed on actors 0 .. 2 (and T1, T2 of actor 3 for the 9th: its RT stays free), then the Kick to
    actor 3 among nine Kick(0)"""
    gos = {7: [(0, 1), (1, 0), (2, 0)], 8: [(0, 1), (1, 1), (2, 0)], 9: [(0, 1), (1, 0), (2, 0), (3, 0)]}[parked]
    ev = [start(a) for a in range(4)] + [send(a, GO, p0) for a, p0 in gos] + [wait_quiescence()]
    return events_to_array(ev + [send(3, KICK, kick, 0)] + [send(i % 3, KICK, 0, i) for i in range(9)])


def _resend_model():
    """Three actors.  Go arms the repeating RT (and T1 when p0 is set); RT's handler cancels it, pings everybody and arms it again."""
    h = {(0, "Go"): Asm().trep(RT).skipz(M.P0, "x").trep(T1).label("x"),
         (0, "RT"): Asm().add(M.F[0], M.F[0], 1).tcancel(RT).bcast(PING, M.F[0], 0).trep(RT),
         (0, "T1"): Asm().add(M.F[2], M.F[2], 1), (0, "Ping"): Asm().add(M.F[1], M.F[1], 1), (0, "Kick"): Asm().add(M.F[3], M.F[3], 1)}
    return build_model("fxc_resend", 3, MSGS, h, [[0] * 8] * 3, NO_INV)


@functools.lru_cache(maxsize=None)
def _cases():
    """{name: (model, events, limits, schedules, (flag of every execution | None, flag of some execution | None) | None)}"""
    c = {}
    hand = _hand_model()
    c["hand"] = (hand, _hand_events(5), T.Limits(80, 0, 64, 0, 0, 0), 512, (0, None))
    c["hand-p6"] = (hand, _hand_events(6, quiesce=0.0), T.Limits(80, 0, 6, 0, 0, 0), 256, None)       # (p_max met by injections and sends alike)
    mm = _matrix_model()
    P, Q = T.V_PENDING_OVF, T.V_QUEUE_OVF
    for kick in (5, 4):
        for p_max in (12, 11, 10):
            # DEMI_TQ_CAP - 1: the TSET fits, and the pending set overflows: at the BCAST, or at the next step's 8 timers
            c["matrix-k%d-q7-p%d" % (kick, p_max)] = (mm, _matrix_events(7, kick), T.Limits(0, 0, p_max, 0, 0, 0), 512, (P, P))
            # DEMI_TQ_CAP: the TSET overflows.  [BCAST, TSET]: the BCAST comes first - the queue flag only where it fits; [TSET, BCAST]: always
            some_q = kick == 4 or p_max == 12
            c["matrix-k%d-q8-p%d" % (kick, p_max)] = (mm, _matrix_events(8, kick), T.Limits(0, 0, p_max, 0, 0, 0), 512, (None, Q) if some_q else (P, P))
        # one more than DEMI_TQ_CAP: the queue flag before anything of the batch is delivered
        c["matrix-k%d-q9-p12" % kick] = (mm, _matrix_events(9, kick), T.Limits(0, 0, 12, 0, 0, 0), 256, (Q, Q))
        # no capacity in the way
        c["matrix-k%d-q7-p64" % kick] = (mm, _matrix_events(7, kick), T.Limits(60, 0, 64, 0, 0, 0), 256, (0, None))
    rm = _resend_model()
    ev = events_to_array([start(a) for a in range(3)] + [send(0, GO, 1), send(1, GO, 0), send(2, GO, 1)] + [send(i % 3, KICK, 0, i) for i in range(3)])
    c["resend"] = (rm, ev, T.Limits(60, 0, 64, 0, 0, 0), 512, (0, None))
    c["resend-p8"] = (rm, ev, T.Limits(60, 0, 8, 0, 0, 0), 512, (None, P))
    return c


NAMES = (["hand", "hand-p6"] +
         ["matrix-k%d-q%d-p%d" % (k, q, p) for k in (5, 4) for q, ps in ((7, (12, 11, 10, 64)), (8, (12, 11, 10)), (9, (12,))) for p in ps] +
         ["resend", "resend-p8"])
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
def test_reordered_deliveries_equal_the_oracle(oracle, name, specialise):
    model, ev, lim, n, expect = _cases()[name]
    ctx = _fresh(model, ev, specialise)
    try:
        for fifo in (False, True):
            l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
            want = _want(oracle, name, fifo)
            flags = want["flags"] & OVF
            print(name, "fifo" if fifo else "random", "none / pending / queue / both:",
                  int((flags == 0).sum()), int((flags == T.V_PENDING_OVF).sum()), int((flags == T.V_QUEUE_OVF).sum()), int((flags == OVF).sum()))
            # an overflowed execution's verdict is its FIRST flag alone
            assert (flags != OVF).all(), (name, "oracle: both flags")
            if expect is not None:
                every, some = expect
                if every is not None:
                    assert (flags == every).all(), (name, "oracle", every)
                if some is not None:
                    assert (flags == some).any(), (name, "oracle", some)
            got = ctx.random_explore(n, l, seed_base=SEED)
            assert ((got["flags"] & OVF) != OVF).all(), (name, "both flags")
            assert_same(got, want)                                                                       # REC off
            for s in (SEED, SEED + 1):                                                                   # REC on: the effect queue
                _same_trace(ctx.random_get_trace(s, l), oracle.random_execute(model, ev, s, l))
    finally:
        ctx.close()


def test_the_matrix_meets_both_capacities_in_one_delivery(oracle):
    """On the oracle: with the queue at its capacity and p_max 11, the executions that deliver Kick(5) = [BCAST, TSET RT] first
    report the pending flag and the ones that deliver Kick(4) = [TSET RT, BCAST] first the queue flag - same trace otherwise, so
    the two cases differ in exactly the executions whose first delivery of the batch is the Kick."""
    a, b = _want(oracle, "matrix-k5-q8-p11", False), _want(oracle, "matrix-k4-q8-p11", False)
    differ = a["flags"] != b["flags"]
    assert 10 < differ.sum() < 150                     # (one of ten messages is the Kick: about 51 of 512)
    assert ((a["flags"][differ] & OVF) == T.V_PENDING_OVF).all() and ((b["flags"][differ] & OVF) == T.V_QUEUE_OVF).all()


@pytest.mark.parametrize("specialise", [False, True], ids=["interpreted", "compiled"])
def test_candidate_and_test_launches_of_the_hand_made_table(oracle, specialise):
    """MULTI (random_explore_candidates) and TESTS (random_explore_tests): a workgroup per subsequence of the hand-made table's trace."""
    model, full = _hand_model(), _hand_events(5)
    n_ev = len(full)
    keeps = [list(range(n_ev)), [i for i in range(n_ev) if i % 5 != 4], list(range(3)) + list(range(9, n_ev)), list(range(14))]
    execs = 64
    ctx = _fresh(model, full, specialise)
    try:
        for p_max in (64, 5):
            lim = T.Limits(80, 0, p_max, 0, 0, 1)
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


@pytest.mark.parametrize("name,cfg", [("raft3", raft3_config1), ("raft5", raft5_config2)])
def test_raft_with_the_switch_on_and_off(oracle, monkeypatch, name, cfg):
    """The election timeout's TSET after its BCAST is the moved row of these tables.  DEMI_JIT_NO_FX_COMMUTE compiles the schedule
    without commutation: another kernel, the same verdicts."""
    model, ev, lim = cfg()
    want = oracle.random_explore(model, ev, 1024, seed_base=SEED, limits=lim, n_threads=CPUS)
    ids = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("DEMI_EXPERIMENT", "1")
            monkeypatch.setenv("DEMI_JIT_NO_FX_COMMUTE", "1")
        ctx = _fresh(model, ev, True)
        try:
            ids.append(ctx.code_id())
            assert_same(ctx.random_explore(1024, lim, seed_base=SEED), want)
            assert_same(ctx.random_explore(1024, _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO), seed_base=SEED),
                        oracle.random_explore(model, ev, 1024, seed_base=SEED, limits=_lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO), n_threads=CPUS))
        finally:
            ctx.close()
    assert ids[0] != ids[1] and 0 not in ids
