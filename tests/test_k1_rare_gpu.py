"""K1 with its never-taken paths hinted out of the delivery loop's straight line (k1_random_explore.hpp K1_RARE):
the rejected draw of nextInt, the capacity arms of every append and enqueue, the re-entry of timersToResend over DEMI_TQ_CAP and
the TD_MANY scan of a cancel are reached through a branch of their own in the kernel compiled for a table.  The hint moves code,
it computes nothing else: every case here ENTERS one of those paths and is held bit for bit against the CPU oracle - 256 to
1 024 schedules, the table interpreter and the compiled kernel, the compiled kernel once more with DEMI_K1_NO_RARE (the plain
conditions: another code object, the same verdicts), FullyRandom and SrcDstFIFO, the plain and the recording kernel.

  raft      raft3_config1 and raft5_config2 at 1 024;
  retry     the seeds of tests/limit_tables.py whose k-th scheduler draw nextInt rejects, on raft5: the loop that now sits out of line;
  overflow  the tables of tests/test_k1_exits_gpu.py that reach p_max inside an injected batch, at the step's timer append and at
            a BCAST's receivers, DEMI_TQ_CAP / DEMI_RESEND_CAP at a set, at a parked timer and at the re-entry - each exactly
            reached and exceeded by one - and the capacity tables of tests/test_k1_timers_gpu.py;
  scan      the `tq` table of tests/test_k1_timers_gpu.py: two and more pending copies of one timer, then its cancel (TD_MANY)."""
import os

import numpy as np
import pytest

from demi_amd import types as T
from demi_amd.apps import raft5_config2

from . import limit_tables as LT
from . import test_k1_exits_gpu as EX
from . import test_k1_timers_gpu as TM
from .test_k1_gpu import assert_same
from .test_limits_gpu import _fresh, _lim, _same_trace

pytestmark = pytest.mark.gpu

CPUS = min(16, os.cpu_count() or 1)
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
EXITS = [n for n in EX.NAMES if n.startswith(("batch16", "batch30-p29", "timer-append", "bcast", "queue-"))] + ["raft3", "raft5"]
TIMERS = ["tq", "pmax2", "pmax3", "cap-tq1+7", "cap-tq1+8", "cap-tq-plain8", "cap-tq-plain9", "cap-resend8", "cap-resend9"]
CASES = [("exits", n) for n in EXITS] + [("timers", n) for n in TIMERS]
KERNELS = ["interpreted", "compiled", "compiled-no-rare"]


def _case(src, name):
    mod = EX if src == "exits" else TM
    model, ev, lim, n = mod._cases()[name][:4]
    return mod, model, ev, lim, n


def _context(monkeypatch, model, ev, kernel):
    """the table interpreter, the compiled kernel, or the compiled kernel with plain conditions"""
    if kernel == "compiled-no-rare":
        monkeypatch.setenv("DEMI_EXPERIMENT", "1")
        monkeypatch.setenv("DEMI_JIT_DEFINES", "DEMI_K1_NO_RARE=1")
    return _fresh(model, ev, kernel != "interpreted")


def test_the_borrowed_cases_exist():
    assert all(n in EX._cases() for n in EXITS) and all(n in TM._cases() for n in TIMERS)
    assert len(EXITS) == 18


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("src,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_hinted_paths_equal_the_oracle(oracle, monkeypatch, src, name, kernel):
    mod, model, ev, lim, n = _case(src, name)
    ctx = _context(monkeypatch, model, ev, kernel)
    try:
        for fifo in (False, True):
            l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
            want = mod._want(oracle, name, fifo)
            assert ((want["flags"] & OVF) != OVF).all(), (name, "oracle: both flags")
            assert_same(ctx.random_explore(n, l, seed_base=mod.SEED), want)                               # REC off
            _same_trace(ctx.random_get_trace(mod.SEED, l), oracle.random_execute(model, ev, mod.SEED, l))  # REC on
    finally:
        ctx.close()


def test_the_cases_enter_the_hinted_paths(oracle):
    """On the oracle: the overflow cases carry their flag in some execution, each flag alone, and both sides of every capacity
    are there - a case that fits and its neighbour that does not; the `tq` table has executions with two copies of T1 pending."""
    flagged = {}
    for src, name in CASES:
        mod = _case(src, name)[0]
        flagged[name] = int((mod._want(oracle, name, False)["flags"] & OVF != 0).sum())
    for over, fits in (("batch16-p15", "batch16-p16"), ("timer-append-over", "timer-append-fits"), ("queue-tset9", "queue-tset8"),
                       ("queue-trep1+7+1", "queue-trep1+6+1"), ("queue-resend8-reenter+1", "queue-resend8-reenter+0"),
                       ("cap-tq1+8", "cap-tq1+7"), ("cap-resend9", "cap-resend8"), ("pmax3", "pmax2")):
        assert flagged[over] > 0 and flagged[fits] < flagged[over], (over, flagged[over], fits, flagged[fits])
    model, ev, lim = TM._cases()["tq"][:3]
    word_t1 = 0
    for s in range(TM.SEED, TM.SEED + 48):
        _, rec, _ = oracle.random_execute(model, ev, s, lim)
        pending = {}
        for r in rec:
            if r["msg_type"] == TM.T1 and r["snd"] == T.DEADLETTERS:
                if r["kind"] == T.REC_MSG_SEND and not (r["flags"] & 4):
                    pending[int(r["rcv"])] = pending.get(int(r["rcv"]), 0) + 1
                    word_t1 = max(word_t1, pending[int(r["rcv"])])
                elif r["kind"] == T.REC_MSG_EVENT:
                    pending[int(r["rcv"])] = pending.get(int(r["rcv"]), 1) - 1
    assert word_t1 >= 2


@pytest.mark.parametrize("kernel", KERNELS)
def test_seeds_whose_draw_is_rejected(oracle, monkeypatch, kernel):
    """nextInt's retry: seeds built so that the k-th draw of the scheduler's generator is rejected (tests/limit_tables.py; the CPU
    suite counts in the transliteration that they really retry at every call site), as explicit seeds, both strategies."""
    model, ev, lim = raft5_config2()
    seeds = np.array(LT.candidate_seeds(), dtype=np.uint64)
    ctx = _context(monkeypatch, model, ev, kernel)
    try:
        for fifo in (False, True):
            l = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO) if fifo else lim
            want = oracle.random_explore(model, ev, len(seeds), seed_base=0, seeds=seeds, limits=l, n_threads=CPUS)
            assert_same(ctx.random_explore(len(seeds), l, seed_base=0, seeds=seeds), want)
            for s in seeds[:4]:
                _same_trace(ctx.random_get_trace(int(s), l), oracle.random_execute(model, ev, int(s), l))
    finally:
        ctx.close()


def test_the_switch_compiles_another_kernel(monkeypatch):
    """DEMI_K1_NO_RARE is a real switch: the two compiled kernels of raft5 differ, and the default one is the hinted one."""
    model, ev, _ = raft5_config2()
    ids = []
    for kernel in ("compiled", "compiled-no-rare"):
        ctx = _context(monkeypatch, model, ev, kernel)
        try:
            ids.append(ctx.code_id())
        finally:
            ctx.close()
    assert ids[0] != ids[1] and 0 not in ids
