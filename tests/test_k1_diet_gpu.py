"""The per-iteration code K1 was relieved of - a cancel that removes through the directory entry it already holds, the constant
hit mask of a fresh execution with the batched copy and hash of the actor states - and the code around it that was looked at and
kept: the timer enqueues with their capacity checks and the cooperative batch flush.  Bit for bit against the CPU oracle: 256 .. 1 024 schedules per case on hand-built 3 - 6 actor tables,
the table interpreter and the compiled kernel, FullyRandom and SrcDstFIFO, the plain and the recording kernel.

  cancel    every timer is armed once, twice or three times per actor and cancelled while the pending set holds other actors'
            timers and plain messages: over a few hundred random schedules the cancelled copy sits in slot 0, in the last slot
            (no move) and in between with another single-copy timer in the last slot (its entry must follow the move); the
            directory entry is exact (one copy) or TD_MANY with two copies (repaired to the survivor, which may be the moved
            last word) and with three (stays TD_MANY); a cancel that finds the timer still in messagesToSend (set and
            cancelled in one delivery) and one parked in timersToResend (a repeating timer cancelled by its own delivery).
  capacity  DEMI_TQ_CAP and DEMI_RESEND_CAP reached exactly and exceeded by one at every enqueue site: TSET (8 one-shot sets in
            one delivery fit; a ninth is a ninth effect row and overflows DEMI_FX_CAP first, so the TSET that finds the queue
            full is the one behind the re-entered list below), TREP (a repeating timer armed behind n one-shot sets, messagesToSend holding one entry already),
            the re-enqueue of a delivered repeating timer (8 or 9 of them delivered in a row), and timersToResend re-entering
            messagesToSend (8 entries: exactly the capacity - messagesToSend is always empty at that point, so it cannot be
            exceeded there - followed by one more TSET that does exceed it).  Each on a 3-actor table (9 directory entries: the
            4-bit queues) and a 6-actor one (18: the byte form); the flag is asserted on the oracle, the verdicts are compared.
  hits      initial states that already hit the invariant for one actor (a second hit violates later) and for two (the first
            check violates); a DEMI_INV_PEERS program; candidate (MULTI) and test (TESTS) launches whose traces Start
            different actor sets with populate_all = 0; a carried instance of 3 executions (the states start over).
  flush     batches of exactly 16 and of 17 Sends, 30 Sends (across the 28 LDS-resident slots of the generic kernel), p_max
            reached in the middle of a batch, every lane of the first waves flushing in the same iteration, and SPREAD launches
            with 1 and 5 lanes per wave."""
import functools
import os

import numpy as np
import pytest

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.fuzzer import events_to_array, send, start, wait_quiescence
from demi_amd.model import Asm, build_model

from .test_k1_gpu import assert_same
from .test_limits_gpu import _fresh, _lim, _same_trace

pytestmark = pytest.mark.gpu

SEED = 9090
CPUS = min(16, os.cpu_count() or 1)
NO_INV = (T.INV_NONE, 0, 0, 0)
MSGS = [("Go", T.MSG_EXTERNAL), ("Kick", T.MSG_EXTERNAL), ("Ping", T.MSG_INTERNAL), ("T1", T.MSG_TIMER), ("T2", T.MSG_TIMER), ("RT", T.MSG_TIMER)]
GO, KICK, PING, T1, T2, RT = range(6)
CAP = 8                 # DEMI_TQ_CAP = DEMI_RESEND_CAP of include/demi_gpu.h


def _trace(seed, n_actors, p0s, n, quiesce):
    rng = np.random.default_rng(seed)
    ev = [start(a) for a in range(n_actors)]
    for _ in range(n):
        ev.append(send(int(rng.integers(n_actors)), GO, int(rng.choice(p0s)), int(rng.integers(2))))
        if rng.random() < quiesce:
            ev.append(wait_quiescence())
    return events_to_array(ev)


# ---------------------------------------------------------------------------------------------------------------- cancel
def _cancel_model(n_actors):
    """Go(0) / Go(1) arm T1 / T2 (again and again: a second and third copy), Go(2) / Go(3) cancel them, Go(4) pings the next
    actor (a plain message between the timers), Go(5) sets and cancels T1 in one delivery, Go(6) arms the repeating RT, which
    cancels itself in its second delivery - while it is parked in timersToResend."""
    go = (Asm().if_eq(M.P0, 0, "a").tset(T1).label("a").if_eq(M.P0, 1, "b").tset(T2).label("b")
          .if_eq(M.P0, 2, "c").tcancel(T1).label("c").if_eq(M.P0, 3, "d").tcancel(T2).label("d")
          .if_eq(M.P0, 5, "f").tset(T1).tcancel(T1).label("f").if_eq(M.P0, 6, "g").trep(RT).label("g")
          .if_eq(M.P0, 4, "e").add(M.T0, M.ME, 1).if_eq(M.T0, n_actors, "w").mov(M.T0, 0).label("w").send(PING, M.T0, M.T1, 0).label("e"))
    h = {(0, "Go"): go, (0, "Ping"): Asm().add(M.F[1], M.F[1], 1), (0, "T1"): Asm().add(M.F[2], M.F[2], 1),
         (0, "T2"): Asm().add(M.F[3], M.F[3], 1), (0, "RT"): Asm().add(M.F[0], M.F[0], 1).if_eq(M.F[0], 2, "x").tcancel(RT).label("x")}
    return build_model("diet_cancel%d" % n_actors, n_actors, MSGS, h, [[0] * 8] * n_actors, NO_INV)


# -------------------------------------------------------------------------------------------------------------- capacity
def _capacity_cases(n_actors):
    """[(name, model, events, limits, every execution overflows a timer queue)]"""
    out = []

    def sets(n):
        a = Asm()
        for _ in range(n):
            a.tset(T1)
        return a
    # TSET: 8 one-shot sets in one delivery fit; 9 are 9 effect rows: DEMI_FX_CAP overflows (the same flag)
    for n in (CAP, CAP + 1):
        m = build_model("diet_tset%d_%d" % (n, n_actors), n_actors, MSGS, {(0, "Kick"): sets(n)}, [[0] * 8] * n_actors, NO_INV)
        out.append(("tset%d" % n, m, events_to_array([start(0), send(0, KICK)]), T.Limits(40, 0, 64, 0, 0, 0), n > CAP))
    # TREP: Go arms the repeating RT; its delivery parks it, the Kick's scheduling step moves it to messagesToSend (1 entry),
    # Kick then sets T1 n times and arms the repeating T2: 1 + 6 + 1 fit with 7 effect rows, 1 + 7 + 1 do not, with 8
    for n in (CAP - 2, CAP - 1):
        m = build_model("diet_trep%d_%d" % (n, n_actors), n_actors, MSGS, {(0, "Kick"): sets(n).trep(T2), (0, "Go"): Asm().trep(RT)},
                        [[0] * 8] * n_actors, NO_INV)
        ev = events_to_array([start(0), send(0, GO), wait_quiescence(), send(0, KICK)])
        out.append(("trep1+%d+1" % n, m, ev, T.Limits(40, 0, 64, 0, 0, 0), n > CAP - 2))
    # the re-enqueue of a delivered repeating timer: three actors arm 3 + 3 + 2 (or 3) repeating timers, every one is delivered
    # once before anything else and parked in timersToResend; then (8 only) the Kick of the next batch is the first delivery that
    # is no repeating timer: all 8 re-enter messagesToSend - exactly its capacity - and Kick(1) sets actor 2's RT, the one
    # timer that is not registered as repeating (a set of a registered one is ignored)
    arm = Asm().trep(T1).trep(T2).skipz(M.P0, "x").trep(RT).label("x")
    kick = Asm().skipz(M.P0, "k").tset(RT).label("k")
    m = build_model("diet_resend_%d" % n_actors, n_actors, MSGS, {(0, "Go"): arm, (0, "Kick"): kick}, [[0] * 8] * n_actors, NO_INV)
    arms = [start(a) for a in range(3)] + [send(0, GO, 1), send(1, GO, 1)]
    out.append(("resend9", m, events_to_array(arms + [send(2, GO, 1)]), T.Limits(60, 0, 64, 0, 0, 0), True))
    for p0 in (0, 1):
        ev = events_to_array(arms + [send(2, GO, 0), wait_quiescence(), send(2, KICK, p0)])
        out.append(("resend8-reenter+%d" % p0, m, ev, T.Limits(60, 0, 64, 0, 0, 0), p0 == 1))
    return out


# ------------------------------------------------------------------------------------------------------------------ hits
def _hits_model(n_hit, program=None):
    """F0 == 1 is the hit, F1 the key (0 everywhere); the first n_hit of four actors start as hits.  Go(1) makes the receiver one,
    Go(2) takes it back, everything else pings the next actor."""
    go = (Asm().if_eq(M.P0, 1, "a").mov(M.F[0], 1).label("a").if_eq(M.P0, 2, "b").mov(M.F[0], 0).label("b")
          .if_eq(M.P0, 0, "c").add(M.T0, M.ME, 1).and_(M.T0, M.T0, 3).send(PING, M.T0, M.T1, 0).label("c"))
    h = {(0, "Go"): go, (0, "Ping"): Asm().add(M.F[2], M.F[2], 1)}
    init = [[1 if a < n_hit else 0] + [0] * 7 for a in range(4)]
    return build_model("diet_hits%d%s" % (n_hit, "p" if program else ""), 4, MSGS, h, init, program or (T.INV_AT_MOST_ONE, 0, 1, 1))


def _peers_program():
    """NEVER "F0 == 1 here and at some created actor with a higher id" - a program that reads the other actors (DEMI_INV_PEERS)"""
    p = Asm().if_eq(M.F[0], 1, "no")
    for j in range(4):
        p.mov(M.T2, j).if_gt(M.T2, M.ME, "n%d" % j).peer(M.T1, M.T2, M.PEER_CREATED).if_ne(M.T1, 0, "n%d" % j)
        p.peer(M.T1, M.T2, 0).if_eq(M.T1, 1, "n%d" % j).mov(M.T0, 1).label("n%d" % j)
    return p.label("no").mov(M.T1, 0).halt()


# ----------------------------------------------------------------------------------------------------------------- flush
def _flush_case(n_sends, p_max):
    """n external Kicks to three actors injected in one batch, a second batch behind a WaitQuiescence"""
    h = {(0, "Kick"): Asm().add(M.F[0], M.F[0], 1).skipz(M.P0, "x").send(PING, M.ME, M.P0, 0).label("x"), (0, "Ping"): Asm().add(M.F[1], M.F[1], 1)}
    m = build_model("diet_flush", 3, MSGS, h, [[0] * 8] * 3, NO_INV)
    ev = [start(a) for a in range(3)] + [send(i % 3, KICK, i % 4, i) for i in range(n_sends)] + [wait_quiescence()] + [send(i % 3, KICK, 1, i) for i in range(5)]
    return m, events_to_array(ev), T.Limits(0, 0, p_max, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def _cases():
    """{name: (model, events, limits, schedules, None or whether every execution carries V_QUEUE_OVF, 4-bit queues or None)}"""
    c = {}
    for na in (3, 6):
        m = _cancel_model(na)
        c["cancel-%d" % na] = (m, _trace(11 + na, na, [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 5, 6], 40, 0.08), T.Limits(90, 0, 64, 0, 0, 0), 512, None, na == 3)
        c["cancel-%d-quiet" % na] = (m, _trace(21 + na, na, [0, 0, 1, 2, 3, 4, 6], 24, 0.3), T.Limits(90, 0, 64, 0, 0, 0), 256, None, na == 3)
        for name, model, ev, lim, ovf in _capacity_cases(na):
            c["cap-%s-%d" % (name, na)] = (model, ev, lim, 256, ovf, na == 3)
    c["hits-1"] = (_hits_model(1), _trace(31, 4, [0, 0, 1, 2], 20, 0.15), T.Limits(60, 3, 64, 0, 0, 0), 512, None, None)
    c["hits-2"] = (_hits_model(2), _trace(32, 4, [0, 0, 1, 2], 12, 0.15), T.Limits(60, 3, 64, 0, 0, 0), 256, None, None)
    c["hits-peers"] = (_hits_model(1, (T.INV_NEVER, _peers_program())), _trace(33, 4, [0, 0, 1, 2], 20, 0.15), T.Limits(60, 3, 64, 0, 0, 0), 512, None, None)
    c["hits-carry"] = (_hits_model(1), _trace(34, 4, [0, 0, 1, 2], 16, 0.15), T.Limits(60, 3, 64, 0, 0, 0, 0, 0, 3), 510, None, None)
    for n, p_max in ((16, 64), (17, 64), (30, 64), (30, 20)):
        c["flush-%d-p%d" % (n, p_max)] = _flush_case(n, p_max) + (256, None, None)
    return c


NAMES = (["cancel-3", "cancel-3-quiet", "cancel-6", "cancel-6-quiet"] +
         ["cap-%s-%d" % (s, na) for na in (3, 6) for s in ("tset8", "tset9", "trep1+6+1", "trep1+7+1", "resend9", "resend8-reenter+0", "resend8-reenter+1")] +
         ["hits-1", "hits-2", "hits-peers", "hits-carry", "flush-16-p64", "flush-17-p64", "flush-30-p64", "flush-30-p20"])
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
def test_diet_paths_equal_the_oracle(oracle, monkeypatch, tmp_path, name, specialise):
    model, ev, lim, n, ovf, narrow = _cases()[name]
    if specialise:
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_JIT_DUMP_SRC", str(tmp_path / "tu"))
    ctx = _fresh(model, ev, specialise)
    try:
        if specialise:
            tu = open(str(tmp_path / "tu") + ".0").read()
            if narrow is not None:
                assert ("#define DEMI_JIT_TQ4_TYPES" in tu) == narrow, name
            # the constant hit mask: bit a = actor a's initial F0 is 1 - by hand, per table; a program invariant gets no constant
            if name.startswith("hits-"):
                want_def = {"hits-1": "0x1u", "hits-2": "0x3u", "hits-carry": "0x1u", "hits-peers": None}[name]
                assert ("#define DEMI_JIT_INIT_HITS" in tu) == (want_def is not None), name
                assert want_def is None or "#define DEMI_JIT_INIT_HITS %s\n" % want_def in tu, name
        for fifo in (False, True):
            l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
            want = _want(oracle, name, fifo)
            if ovf is not None:
                assert (((want["flags"] & T.V_QUEUE_OVF) != 0) == ovf).all(), (name, "oracle")
            assert_same(ctx.random_explore(n, l, seed_base=SEED), want)                                # REC off
            if lim.executions_per_instance <= 1:
                for s in (SEED, SEED + 1, SEED + 2):                                                     # REC on
                    _same_trace(ctx.random_get_trace(s, l), oracle.random_execute(model, ev, s, l))
        if name.startswith("flush-"):
            # SPREAD: the flushing lanes are the first 1 or 5 of each wave
            for lanes in ("1", "5"):
                monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", lanes)
                assert_same(ctx.random_explore(70, lim, seed_base=SEED), _want(oracle, name, False)[:70])
            monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE")
    finally:
        ctx.close()


@pytest.mark.parametrize("specialise", [False, True], ids=["interpreted", "compiled"])
def test_candidates_and_tests_that_start_different_actor_sets(oracle, specialise):
    """MULTI (random_explore_candidates) and TESTS (random_explore_tests) with populate_all = 0: `exists` is each workgroup's own -
    the actors its trace Starts - and masks the hit mask every execution starts from.  Actors 0 and 1 hit initially: a trace that
    Starts both violates at once, one that Starts one of them only when a Go(1) makes a second hit, one that Starts neither never
    through them."""
    model = _hits_model(2)
    lim = T.Limits(60, 3, 64, 0, 0, 0)
    gos = [send(a, GO, p0, 0) for a, p0 in ((2, 0), (3, 1), (2, 1), (0, 0), (1, 2), (3, 0), (2, 2), (1, 1))]
    full = events_to_array([start(a) for a in range(4)] + gos)
    keeps = [[0, 1, 2, 3], [0, 2, 3], [1, 2, 3], [2, 3], [0, 1]]
    kept = [np.array([i in k for i in range(4)] + [True] * len(gos)) for k in keeps]
    execs = 64
    ctx = _fresh(model, full, specialise)
    try:
        masks = np.zeros((len(kept), 4), dtype=np.uint64)
        for i, kp in enumerate(kept):
            masks[i, 0] = sum(1 << j for j in np.nonzero(kp)[0])
        gv, gf = ctx.random_explore_candidates(masks, execs, lim, seed_base=SEED)
        tv, tf = ctx.random_explore_tests([full[kp] for kp in kept], execs, lim, seed_base=SEED)
        viol = []
        for i, kp in enumerate(kept):
            c = oracle.random_explore(model, full[kp], execs, seed_base=SEED, limits=lim, n_threads=CPUS)
            assert_same(gv[i], c)
            assert_same(tv[i], c)
            viol.append(bool((c["flags"] & T.V_VIOLATION).any()))
            assert bool(gf[i] & 1) == viol[-1] and bool(tf[i] & 1) == viol[-1]
        assert viol[0] and viol[4]
    finally:
        ctx.close()


def test_hand_built_tables_reach_what_they_are_built_for(oracle):
    """The oracle's recorded traces say that the paths exist: in the cancel tables timers are sent, delivered and some sent ones are
    never delivered (cancelled); two initial hits violate in every execution, one only in some; the carried instance's second and
    third executions differ from a fresh run of the same index (the generator goes on) while each starts from the initial states."""
    for name in ("cancel-3", "cancel-6"):
        model, ev, lim = _cases()[name][:3]
        sent = delivered = 0
        for s in range(SEED, SEED + 16):
            _, rec, _ = oracle.random_execute(model, ev, s, lim)
            is_t = np.isin(rec["msg_type"], [T1, T2, RT]) & (rec["snd"] == T.DEADLETTERS)
            sent += int((is_t & (rec["kind"] == T.REC_MSG_SEND)).sum())
            delivered += int((is_t & (rec["kind"] == T.REC_MSG_EVENT)).sum())
        assert delivered > 32 and sent >= delivered + 8, (name, sent, delivered)
    v1, v2 = (_want(oracle, n, False)["flags"] & T.V_VIOLATION for n in ("hits-1", "hits-2"))
    assert (v2 != 0).all() and (v1 != 0).any() and (v1 == 0).any()
    assert (_want(oracle, "flush-30-p20", False)["flags"] & T.V_PENDING_OVF).all()
    assert not (_want(oracle, "flush-30-p64", False)["flags"] & T.V_PENDING_OVF).any()
