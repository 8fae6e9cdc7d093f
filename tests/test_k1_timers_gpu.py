"""K1's timer bookkeeping in the apply phase - the queued-timer filter of the cancel path and the two forms of the timer queues
(demi_device.hpp TimerQ: one byte per entry, or four bits in a kernel compiled for a table with n_actors * n_timer_types <= 16) -
bit for bit against the CPU oracle (oracle/demi_oracle.c): the table interpreter and the compiled kernel, FullyRandom and
SrcDstFIFO, the plain kernel (256 .. 1 024 verdicts) and the recording one (a few whole traces).

Hand-built 3-actor tables whose handlers reach
  tq      a cancel of a timer that sits in messagesToSend: set and cancelled by neighbouring rows of one delivery; set, a send,
          then the cancel in a later effect slot; a cancel with no copy anywhere (T2 is never set); two and more pending copies
          of T1, then a cancel (the directory entry is TD_MANY: the scan);
  rep     a repeating timer: cancelled by its own delivery while it is parked in timersToResend; cancelled by the NEXT delivery,
          when timersToResend has just re-entered messagesToSend (the entry the filter knows through justScheduledTimers);
          cancelled while pending, and when it was never set;
  rearm   tcancel(t).tset(t) (from an external's handler and from the timer's own), tcancel(t).tset(u), and a set behind a branch
          that may skip the cancel;
  the capacity cases of test_limits_gpu.py for DEMI_TQ_CAP and DEMI_RESEND_CAP - exactly the capacity and one more, the
  expected flag written down there by hand - whose tables (2 x 4 and 3 x 4 directory entries) compile to the 4-bit form;
  pmax    p_max = 2: a cancel frees a pending slot and the sends behind it fill the set again - two fit, the third aborts.
Tables at the edge of the 4-bit form: 4 actors x 4 timer types and 8 x 2 (16 directory entries, the last that takes it; the
highest entry, 15, is used) and 6 x 3 (18: the first product of a legal actor count and timer-type count above 16 - 17 is
none - which must keep the byte form); which form the compiled kernel got is read from the translation unit it was compiled from.
raft3_config1 and raft5_config2 at 1 024 schedules."""
import functools
import os

import numpy as np
import pytest

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.apps import raft3_config1, raft5_config2
from demi_amd.fuzzer import events_to_array, send, start, wait_quiescence
from demi_amd.model import Asm, build_model

from .test_k1_gpu import assert_same
from .test_limits_gpu import _capacity_cases, _fresh, _lim, _same_trace

pytestmark = pytest.mark.gpu

MSGS = [("Go", T.MSG_EXTERNAL), ("Ping", T.MSG_INTERNAL), ("T1", T.MSG_TIMER), ("T2", T.MSG_TIMER), ("RT", T.MSG_TIMER)]
GO, PING, T1, T2, RT = range(5)
NO_INV = (T.INV_NONE, 0, 0, 0)
SEED = 4242


def _trace(seed, n_actors, p0s, n, quiesce=0.2):
    """Start() of every actor, then n external Go(p0, p1) to random actors, p0 from p0s, with WaitQuiescence sprinkled in."""
    rng = np.random.default_rng(seed)
    ev = [start(a) for a in range(n_actors)]
    for _ in range(n):
        ev.append(send(int(rng.integers(n_actors)), GO, int(rng.choice(p0s)), int(rng.integers(2))))
        if rng.random() < quiesce:
            ev.append(wait_quiescence())
    return events_to_array(ev)


def _next_actor(a, n_actors):
    """T0 = (ME + 1) % n_actors"""
    return a.add(M.T0, M.ME, 1).if_eq(M.T0, n_actors, "wrap").mov(M.T0, 0).label("wrap")


def _tq_model():
    go = (Asm().if_eq(M.P0, 0, "a").tset(T1).tcancel(T1).label("a")
          .if_eq(M.P0, 1, "b").tset(T1).send(PING, M.ME, M.T1, 0).tcancel(T1).label("b")
          .if_eq(M.P0, 4, "c").tcancel(T2).label("c")
          .if_eq(M.P0, 5, "d").tset(T1).label("d")
          .if_eq(M.P0, 9, "e").tcancel(T1).label("e"))
    h = {(0, "Go"): go, (0, "Ping"): Asm().add(M.F[1], M.F[1], 1), (0, "T1"): Asm().add(M.F[2], M.F[2], 1)}
    return build_model("timers_tq", 3, MSGS, h, [[0] * 8] * 3, NO_INV), _trace(1, 3, [0, 1, 4, 5, 5, 5, 9, 9], 28), T.Limits(80, 0, 64, 0, 0, 0)


def _rep_model():
    go = Asm().if_eq(M.P0, 2, "a").trep(RT).label("a").if_eq(M.P0, 3, "b").tcancel(RT).label("b").if_eq(M.P0, 10, "c")
    go = _next_actor(go, 3).send(PING, M.T0, M.T1, 0).label("c")
    ping = Asm().add(M.F[1], M.F[1], 1).and_(M.T0, M.F[1], 1).skipz(M.T0, "e").tcancel(RT).label("e")
    rt = Asm().add(M.F[0], M.F[0], 1).if_eq(M.F[0], 3, "x").tcancel(RT).label("x")
    h = {(0, "Go"): go, (0, "Ping"): ping, (0, "RT"): rt}
    return build_model("timers_rep", 3, MSGS, h, [[0] * 8] * 3, NO_INV), _trace(2, 3, [2, 2, 3, 10, 10], 24), T.Limits(60, 0, 64, 0, 0, 0)


def _rearm_model():
    go = (Asm().if_eq(M.P0, 5, "a").tset(T1).label("a")
          .if_eq(M.P0, 6, "b").tcancel(T1).tset(T2).label("b")
          .if_eq(M.P0, 7, "c").tcancel(T1).tset(T1).label("c")
          .if_eq(M.P0, 8, "d").skipz(M.P1, "s").tcancel(T2).label("s").tset(T2).label("d"))
    t1 = Asm().add(M.F[2], M.F[2], 1).if_lt(M.F[2], 3, "x").tcancel(T1).tset(T1).label("x")
    h = {(0, "Go"): go, (0, "T1"): t1, (0, "T2"): Asm().add(M.F[3], M.F[3], 1)}
    return build_model("timers_rearm", 3, MSGS, h, [[0] * 8] * 3, NO_INV), _trace(3, 3, [5, 5, 6, 7, 7, 8, 8], 28), T.Limits(80, 0, 64, 0, 0, 0)


def _pmax_case(n):
    """Go(0) arms T1, Go(1) cancels it and sends n Pings to itself; both are injected at once and p_max is 2."""
    go = Asm().if_eq(M.P0, 0, "a").tset(T1).label("a").if_eq(M.P0, 1, "b").tcancel(T1)
    for _ in range(n):
        go.send(PING, M.ME, M.T1, 0)
    go.label("b")
    m = build_model("timers_pmax%d" % n, 3, MSGS, {(0, "Go"): go, (0, "Ping"): Asm().add(M.F[1], M.F[1], 1)}, [[0] * 8] * 3, NO_INV)
    return m, events_to_array([start(0), send(0, GO, 0), send(0, GO, 1)]), T.Limits(40, 0, 2, 0, 0, 0)


def _grid_model(n_actors, ntt):
    """n_actors x ntt directory entries: every one-shot timer type k is re-armed by Go(k); the last type is the repeating one,
    armed by Go(ntt - 1) and cancelled by Go(ntt) or by its own third delivery."""
    msgs = [("Go", T.MSG_EXTERNAL), ("Ping", T.MSG_INTERNAL)] + [("Tm%d" % k, T.MSG_TIMER) for k in range(ntt)]
    last = 2 + ntt - 1
    go = Asm()
    for k in range(ntt - 1):
        go.if_eq(M.P0, k, "k%d" % k).tcancel(2 + k).tset(2 + k).label("k%d" % k)
    go.if_eq(M.P0, ntt - 1, "r").trep(last).label("r").if_eq(M.P0, ntt, "c").tcancel(last).label("c")
    rt = Asm().add(M.F[0], M.F[0], 1).if_eq(M.F[0], 3, "x").tcancel(last).label("x")
    h = {(0, "Go"): go, (0, "Tm%d" % (ntt - 1)): rt}
    model = build_model("timers_%dx%d" % (n_actors, ntt), n_actors, msgs, h, [[0] * 8] * n_actors, NO_INV)
    ev = _trace(10 * n_actors + ntt, n_actors, list(range(ntt + 1)) + [ntt - 1], 5 * n_actors)
    # (the last actor arms the repeating timer for certain: directory entry n_actors * ntt - 1)
    ev = np.concatenate([ev, events_to_array([send(n_actors - 1, GO, ntt - 1), send(n_actors - 1, GO, 0), wait_quiescence(),
                                              send(n_actors - 1, GO, ntt)])])
    return model, ev, T.Limits(70, 0, 64, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def _cases():
    """{name: (model, events, limits, schedules, low flag byte every execution must carry or None, 4-bit form or None)}"""
    c = {"tq": _tq_model() + (512, None, True), "rep": _rep_model() + (512, None, True), "rearm": _rearm_model() + (512, None, True),
         "pmax2": _pmax_case(2) + (256, None, True), "pmax3": _pmax_case(3) + (256, None, True),
         "4x4": _grid_model(4, 4) + (512, None, True), "8x2": _grid_model(8, 2) + (512, None, True), "6x3": _grid_model(6, 3) + (512, None, False),
         "raft3_config1": raft3_config1() + (1024, None, True), "raft5_config2": raft5_config2() + (1024, None, True)}
    for name, model, ev, lim, want in _capacity_cases():
        if name.startswith(("tq", "resend")):
            c["cap-" + name] = (model, ev, lim, 256, want, True)
    return c


NAMES = ["tq", "rep", "rearm", "pmax2", "pmax3", "4x4", "8x2", "6x3", "raft3_config1", "raft5_config2",
         "cap-tq1+7", "cap-tq1+8", "cap-tq-plain8", "cap-tq-plain9", "cap-resend8", "cap-resend9"]
_WANT = {}


def _want(oracle, name, fifo):
    """The oracle's verdicts of a case, computed once and shared by the interpreted and the compiled run."""
    if (name, fifo) not in _WANT:
        model, ev, lim, n, _, _ = _cases()[name]
        l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
        w = oracle.random_explore(model, ev, n, seed_base=SEED, limits=l, n_threads=min(16, os.cpu_count() or 1))
        w.setflags(write=False)
        _WANT[(name, fifo)] = w
    return _WANT[(name, fifo)]


def test_the_cases_are_the_ones_listed():
    assert sorted(_cases()) == sorted(NAMES)


@pytest.mark.parametrize("specialise", [False, True], ids=["interpreted", "compiled"])
@pytest.mark.parametrize("name", NAMES)
def test_timer_paths_equal_the_oracle(oracle, monkeypatch, tmp_path, name, specialise):
    model, ev, lim, n, flag, narrow = _cases()[name]
    if specialise:
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_JIT_DUMP_SRC", str(tmp_path / "tu"))
    ctx = _fresh(model, ev, specialise)
    try:
        if specialise:
            # which form of the timer queues the compiled K1 got: the line jit.hpp tq_defines puts in front of its translation unit
            tu = open(str(tmp_path / "tu") + ".0").read()
            assert ("#define DEMI_JIT_TQ4_TYPES" in tu) == narrow, name
            assert model.n_actors * sum(c == T.MSG_TIMER for c in model.msg_class) <= 16 if narrow else True
        for fifo in (False, True):
            l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
            want = _want(oracle, name, fifo)
            if flag is not None:
                assert ((want["flags"] & 0xFF) == flag).all(), (name, "oracle")
            assert_same(ctx.random_explore(n, l, seed_base=SEED), want)                                # REC off
            for s in (SEED, SEED + 1, SEED + 2):                                                         # REC on
                _same_trace(ctx.random_get_trace(s, l), oracle.random_execute(model, ev, s, l))
    finally:
        ctx.close()


def test_hand_built_tables_reach_what_they_are_built_for(oracle):
    """The oracle's own recorded traces say that the paths exist: timers are sent and delivered in every hand-built table, the
    rep table delivers its repeating timer more than once in some execution, with p_max = 2 three sends behind the cancel always abort and two do not."""
    for name in ("tq", "rep", "rearm", "4x4", "8x2", "6x3"):
        model, ev, lim, n, _, _ = _cases()[name]
        timers = [t for t, c in enumerate(model.msg_class) if c == T.MSG_TIMER]
        sent = delivered = most = 0
        for s in range(SEED, SEED + 24):
            _, rec, _ = oracle.random_execute(model, ev, s, lim)
            is_t = np.isin(rec["msg_type"], timers) & (rec["snd"] == T.DEADLETTERS)
            sent += int((is_t & (rec["kind"] == T.REC_MSG_SEND)).sum())
            d = is_t & (rec["kind"] == T.REC_MSG_EVENT)
            delivered += int(d.sum())
            most = max(most, int((d & (rec["msg_type"] == timers[-1])).sum()))
        assert sent > 24 and delivered > 12, (name, sent, delivered)
        assert most >= 2 or name in ("tq", "rearm"), (name, most)
    f2, f3 = (_want(oracle, "pmax%d" % k, False)["flags"] & T.V_PENDING_OVF for k in (2, 3))
    assert (f3 != 0).all() and (f2 == 0).any()       # (n = 2 fits whenever the cancel found the timer pending or queued)
