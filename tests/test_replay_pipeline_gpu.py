"""GPU parity suite for demi_replay_batch_submit / _wait (K2 in pieces, up to three calls outstanding in one context): every
answer bit for bit what demi_replay_batch returns and what the oracle computes, the flagged list exactly the candidates whose
flags intersect the mask, with the neighbours of a context (synchronous replays, removal batches, K1 tickets, reloads) in
between.  tests/test_replay_pipeline_emu_cpu.py runs part of this file on the wave64 emulator."""
import os

import numpy as np
import pytest

from demi_amd import _native, types as T
from demi_amd import model as M
from demi_amd.apps import SEED_BASE, raft5_config2, raft5_config4, raft11_config2

from .test_k2_gpu import random_masks, record

pytestmark = pytest.mark.gpu

OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
ALL = T.V_VIOLATION | OVF
NONE = 2**64 - 1
ONES = 0xFFFFFFFFFFFFFFFF
WAVE_EDGES = (1, 63, 64, 65, 257, 1000)


class Workload:
    def __init__(self, name, model, used, rec, fingerprint, events=None, lim=None, specialize=False):
        self.name, self.model, self.used, self.rec, self.fingerprint = name, model, used, rec, int(fingerprint)
        self.events, self.lim, self.specialize = events, lim, specialize
        self.max_messages, self.p_max = 0, 64
        self._want = {}

    def limits(self, p_max=64, fk=0, looking_for=None):
        return T.Limits(self.max_messages, 0, p_max, 1, self.fingerprint if looking_for is None else looking_for, 0, 0, fk)

    def load(self, ctx, specialize=None):
        ctx.model_load(self.model.to_struct())
        if self.specialize if specialize is None else specialize:
            ctx.model_specialize()
        ctx.replay_load(self.used, self.rec)

    def masks(self, n, seed=1):
        m = random_masks(np.random.default_rng(seed), len(self.used), n)
        m[0] = ONES
        return m

    def want(self, oracle, masks, lim):
        """the oracle's verdicts, computed once per (candidates, limits)"""
        key = (masks.tobytes(), lim.p_max, lim.looking_for, lim.filter_known_absents)
        if key not in self._want:
            self._want[key] = oracle.sts_replay_batch(self.model, self.used, self.rec, masks, lim, n_threads=os.cpu_count())
        return self._want[key]


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def narrow(ctx):
    """the violating executions of raft5_config2 (50 externals; a second one for the reload) and raft5_config4 (200 externals)"""
    out = {}
    for name, cfg, skip in (("config2", raft5_config2, 0), ("config2b", raft5_config2, 3), ("config4", raft5_config4, 0)):
        model, events, lim = cfg()
        vv, rec, used = record(ctx, model, events, lim, skip=skip)
        out[name] = Workload(name, model, used, rec, vv.fingerprint, events, lim)
    return out


@pytest.fixture(scope="module")
def wide(ctx):
    """the wide raft table of tests/test_wide_gpu.py: terms from 1000, logs from 300 entries (compiled code only)"""
    _, events, lim = raft5_config2()
    model = M.raft_model(5, term0=1000, loglen0=300)
    assert model.wide
    ctx.model_load(model.to_struct())
    ctx.trace_load(events)
    ctx.model_specialize()
    v = ctx.random_explore(4000, lim, seed_base=SEED_BASE)
    k = int(np.nonzero(v["flags"] & T.V_VIOLATION)[0][0])
    vv, rec = ctx.random_get_trace(SEED_BASE + k, lim)
    return Workload("wide", model, events[:T.verdict_trace_idx(vv.flags)], rec, vv.fingerprint, specialize=True)


@pytest.fixture(scope="module")
def big(ctx, oracle):
    """raft11_config2 as tests/test_big_gpu.py::test_replay_and_ddmin sets it up (BIG layout, the scanning kernel)"""
    model, ev, lim = raft11_config2()
    l0 = T.Limits(lim.max_messages, 0, lim.p_max, 0, 0, 0)
    ctx.model_load(model.to_struct())
    ctx.trace_load(ev)
    ctx.model_specialize()
    v = oracle.random_explore(model, ev, 4000, seed_base=SEED_BASE, limits=l0, n_threads=os.cpu_count())
    idx = int(np.nonzero((v["flags"] & T.V_VIOLATION) != 0)[0][0])
    vd, rec = ctx.random_get_trace(SEED_BASE + idx, l0)
    assert vd.flags & T.V_VIOLATION
    w = Workload("raft11", model, ev, rec, vd.fingerprint, specialize=True)
    w.max_messages, w.p_max = lim.max_messages, lim.p_max
    return w


def check_flagged(v, answer, flag_mask, cap=1 << 16):
    """the flagged list of `answer` is exactly the sorted candidates of verdicts v whose flags intersect flag_mask"""
    flagged, n_flagged, first = answer
    sel = np.nonzero(v["flags"] & (flag_mask or T.V_VIOLATION))[0]
    assert n_flagged == len(sel)
    assert first == (int(sel[0]) if len(sel) else NONE)
    assert len(flagged) == min(len(sel), cap)
    if len(sel) <= cap:
        assert (flagged["index"] == sel).all()
        assert (flagged["flags"] == v["flags"][sel]).all() and (flagged["fingerprint"] == v["fingerprint"][sel]).all()


def run(ctx, masks, lim, flag_mask=0, want_verdicts=False, fetch=True):
    """one submit and its wait -> (all verdicts or None, the wait's answer)"""
    t = ctx.replay_batch_submit(masks, lim, flag_mask=flag_mask, want_verdicts=want_verdicts)
    out = np.zeros(len(masks), dtype=T.VERDICT_DTYPE) if fetch else None
    return out, ctx.replay_batch_wait(t, out=out)


def same(got, want):
    assert len(got) == len(want) and (got == want).all(), "first difference at %d" % int(np.nonzero(got != want)[0][0])


# ---------------------------------------------------------------------------------------------- 1. parity at the wave edges
@pytest.mark.parametrize("specialize", [False, True])
@pytest.mark.parametrize("fk", [0, 1, 2])
def test_parity_at_the_wave_edges(ctx, oracle, narrow, fk, specialize):
    for name in ("config2", "config4"):
        w = narrow[name]
        w.load(ctx, specialize)
        assert ctx.is_specialized() == specialize
        lim = w.limits(fk=fk)
        masks = w.masks(max(WAVE_EDGES))
        want = w.want(oracle, masks, lim)
        assert want[0]["flags"] & T.V_VIOLATION and (want["flags"] & T.V_VIOLATION).sum() < len(want)
        for n in WAVE_EDGES:
            same(ctx.replay_batch(masks[:n], lim), want[:n])
            for flag_mask, want_verdicts, fetch in ((0, True, True), (T.V_DIVERGED | T.V_VIOLATION, False, True), (ALL, False, False)):
                out, answer = run(ctx, masks[:n], lim, flag_mask, want_verdicts, fetch)
                if fetch:
                    same(out, want[:n])
                check_flagged(want[:n], answer, flag_mask)


# ---------------------------------------------------------------------------------------------- 2. wide and BIG tables
def test_wide_and_big_tables(ctx, oracle, wide, big):
    for w in (wide, big):
        p_max = w.p_max
        w.load(ctx)
        masks = w.masks(200)
        if w is big:           # (candidates as test_replay_and_ddmin draws them: random words, a denser first quarter)
            rng = np.random.default_rng(7)
            masks = rng.integers(0, 2**63, size=(200, 4), dtype=np.uint64) | (rng.integers(0, 2, size=(200, 4), dtype=np.uint64) << np.uint64(63))
            masks[1:50] |= rng.integers(0, 2**63, size=(49, 4), dtype=np.uint64)
            masks[0] = ONES
        for fk in (0, 1):
            lim = w.limits(p_max=p_max, fk=fk)
            want = w.want(oracle, masks, lim)
            assert want[0]["flags"] & T.V_VIOLATION
            same(ctx.replay_batch(masks, lim), want)
            for flag_mask, want_verdicts, fetch in ((0, True, True), (ALL, False, True), (ALL, False, False)):
                out, answer = run(ctx, masks, lim, flag_mask, want_verdicts, fetch)
                if fetch:
                    same(out, want)
                check_flagged(want, answer, flag_mask)


# ---------------------------------------------------------------------------------------------- 3. three in flight
def test_three_in_flight(ctx, oracle, narrow):
    w = narrow["config2"]
    w.load(ctx)
    big_masks = w.masks(2008, seed=3)
    calls = [(big_masks[:1000], w.limits(p_max=64)), (big_masks[1000:1001], w.limits(p_max=16)),
             (big_masks[1001:1301], w.limits(p_max=128, looking_for=w.fingerprint ^ 0x100))]
    tickets = [ctx.replay_batch_submit(m, lim, flag_mask=ALL, want_verdicts=(j == 1)) for j, (m, lim) in enumerate(calls)]
    assert len(set(tickets)) == 3 and all(t > 0 for t in tickets)
    with pytest.raises(_native.DemiError, match="three replay calls are outstanding"):
        ctx.replay_batch_submit(big_masks[:5], w.limits(), flag_mask=ALL)
    for j in (2, 0, 1):
        m, lim = calls[j]
        out = np.zeros(len(m), dtype=T.VERDICT_DTYPE)
        answer = ctx.replay_batch_wait(tickets[j], out=out)
        want = w.want(oracle, m, lim)
        same(out, want)
        check_flagged(want, answer, ALL)
        if j == 2:               # the freed slot is reused, with a fourth call outstanding beside two
            extra = ctx.replay_batch_submit(big_masks[:70], w.limits(), flag_mask=ALL)
            with pytest.raises(_native.DemiError, match="three replay calls are outstanding"):
                ctx.replay_batch_submit(big_masks[:5], w.limits(), flag_mask=ALL)
    check_flagged(w.want(oracle, big_masks[:1000], w.limits())[:70], ctx.replay_batch_wait(extra), ALL)
    assert (w.want(oracle, calls[2][0], calls[2][1])["flags"] & T.V_VIOLATION).sum() == 0      # (another fingerprint: nothing reproduces)
    # submit(k + 2); wait(k) over calls whose buffers grow and are reused
    sizes = (500, 2000, 50, 2000, 1, 700, 64, 500)
    lim = w.limits()
    want_all = w.want(oracle, big_masks, lim)
    part = lambda k: slice(k, k + sizes[k])
    tickets = [ctx.replay_batch_submit(big_masks[part(k)], lim, flag_mask=ALL, want_verdicts=(k % 2 == 0)) for k in range(2)]
    for k in range(len(sizes)):
        if k + 2 < len(sizes):
            tickets.append(ctx.replay_batch_submit(big_masks[part(k + 2)], lim, flag_mask=ALL, want_verdicts=(k % 2 == 0)))
        out = np.zeros(sizes[k], dtype=T.VERDICT_DTYPE)
        answer = ctx.replay_batch_wait(tickets[k], out=out)
        same(out, want_all[part(k)])
        check_flagged(want_all[part(k)], answer, ALL)


# ---------------------------------------------------------------------------------------------- 4. truncation
def test_truncated_list_keeps_the_exact_count_and_first_index(ctx, narrow):
    w = narrow["config2"]
    w.load(ctx)
    masks = np.full((300, 4), ONES, dtype=np.uint64)
    t = ctx.replay_batch_submit(masks, w.limits())
    flagged, n_flagged, first = ctx.replay_batch_wait(t, cap=7)
    assert n_flagged == 300 and first == 0 and len(flagged) == 7
    idx = [int(i) for i in flagged["index"]]
    assert idx == sorted(set(idx)) and all(0 <= i < 300 for i in idx)
    assert (flagged["flags"] & T.V_VIOLATION).all() and (flagged["fingerprint"] == w.fingerprint).all()


# ---------------------------------------------------------------------------------------------- 5. capacities
def test_aborted_replays_are_named_beside_the_reproducing_ones(ctx, oracle, narrow):
    w = narrow["config4"]
    w.load(ctx)
    masks = w.masks(300, seed=5)
    # a pending capacity at which some candidates abort and others still reproduce: the oracle decides which
    for p_max in (8, 10, 12, 14, 16, 20, 24, 32):
        lim = w.limits(p_max=p_max)
        want = w.want(oracle, masks, lim)
        aborted = (want["flags"] & T.V_PENDING_OVF) != 0
        hit = ((want["flags"] & T.V_VIOLATION) != 0) & ~aborted
        if aborted.any() and not aborted.all() and hit.any():
            break
    assert aborted.any() and not aborted.all() and hit.any()
    out, answer = run(ctx, masks, lim, ALL)
    same(out, want)
    check_flagged(want, answer, ALL)
    flagged = answer[0]
    assert (flagged["flags"] & T.V_PENDING_OVF).any() and ((flagged["flags"] & ALL) == T.V_VIOLATION).any()


# ---------------------------------------------------------------------------------------------- 6. the caller's buffer
def test_masks_are_the_callers_again_when_submit_returns(ctx, oracle, narrow):
    w = narrow["config4"]
    w.load(ctx)
    lim = w.limits()
    masks = w.masks(1000)
    want = w.want(oracle, masks, lim)
    mine = masks.copy()
    t = ctx.replay_batch_submit(mine, lim, flag_mask=ALL)
    mine[:] = 0
    out = np.zeros(len(masks), dtype=T.VERDICT_DTYPE)
    answer = ctx.replay_batch_wait(t, out=out)
    same(out, want)
    check_flagged(want, answer, ALL)
    assert (want["flags"] & T.V_VIOLATION).sum() > 1          # (the empty candidate, which `mine` now holds 1000 times, reproduces nothing)


# ---------------------------------------------------------------------------------------------- 7. neighbours
def test_neighbours_of_outstanding_tickets(ctx, oracle, narrow):
    from demi_amd.internal_minimization import deliveries
    from demi_amd.schedulers import EventTrace
    w = narrow["config2"]
    w.load(ctx)
    ctx.trace_load(w.events)
    lim = w.limits()
    masks = w.masks(1500, seed=9)
    want = w.want(oracle, masks, lim)
    skips = np.array([i for i, _, _ in deliveries(EventTrace(w.rec, w.used))][:60] + [0xFFFFFFFF], dtype=np.uint32)
    k1_n = 600
    tickets = [ctx.replay_batch_submit(masks[:1000], lim, flag_mask=ALL), ctx.replay_batch_submit(masks[1000:], lim, flag_mask=ALL, want_verdicts=True)]
    same(ctx.replay_batch(masks[200:500], lim), want[200:500])
    same(ctx.replay_removal_batch(skips, lim), oracle.sts_removal_batch(w.model, w.used, w.rec, skips, lim, n_threads=os.cpu_count()))
    k1 = ctx.random_explore_submit(k1_n, w.lim, seed_base=SEED_BASE, flag_mask=ALL, want_verdicts=True)
    gv, gk = ctx.replay_get_kept(len(w.rec), int(skips[3]), lim, mask=masks[7])
    cv, ck = oracle.sts_removal_kept(w.model, w.used, w.rec, int(skips[3]), lim, mask=masks[7])
    assert gv.flags == cv.flags and gv.hash == cv.hash and gv.fingerprint == cv.fingerprint and (gk == ck).all()
    tickets.append(ctx.replay_batch_submit(masks[300:900], lim, flag_mask=0))
    same(ctx.replay_batch(masks[:64], lim), want[:64])
    k1_out = np.zeros(k1_n, dtype=T.VERDICT_DTYPE)
    k1_answer = ctx.random_explore_wait(k1, out=k1_out)
    k1_want = oracle.random_explore(w.model, w.events, k1_n, seed_base=SEED_BASE, limits=w.lim, n_threads=os.cpu_count())
    same(k1_out, k1_want)
    check_flagged(k1_want, k1_answer, ALL)
    for t, part, flag_mask in zip(tickets, (slice(0, 1000), slice(1000, 1500), slice(300, 900)), (ALL, ALL, 0)):
        out = np.zeros(part.stop - part.start, dtype=T.VERDICT_DTYPE)
        answer = ctx.replay_batch_wait(t, out=out)
        same(out, want[part])
        check_flagged(want[part], answer, flag_mask)


# ---------------------------------------------------------------------------------------------- 8. reload
def test_a_ticket_answers_for_the_execution_loaded_at_its_submit(ctx, oracle, narrow):
    a, b = narrow["config2"], narrow["config2b"]
    assert len(a.rec) != len(b.rec) or (a.rec != b.rec).any()
    a.load(ctx)
    masks = a.masks(1000, seed=4)
    t = ctx.replay_batch_submit(masks, a.limits(), flag_mask=ALL)
    ctx.replay_load(b.used, b.rec)
    t2 = ctx.replay_batch_submit(masks, b.limits(), flag_mask=ALL, want_verdicts=True)
    for ticket, w in ((t, a), (t2, b)):
        out = np.zeros(len(masks), dtype=T.VERDICT_DTYPE)
        answer = ctx.replay_batch_wait(ticket, out=out)
        want = w.want(oracle, masks, w.limits())
        same(out, want)
        check_flagged(want, answer, ALL)
    assert (a.want(oracle, masks, a.limits()) != b.want(oracle, masks, b.limits())).any()


# ---------------------------------------------------------------------------------------------- 9. tickets
def test_tickets_name_their_kind_and_are_single_use(ctx, oracle, narrow):
    w = narrow["config2"]
    w.load(ctx)
    ctx.trace_load(w.events)
    lim = w.limits()
    masks = w.masks(100)
    want = w.want(oracle, masks, lim)
    for wait in (ctx.replay_batch_wait, ctx.random_explore_wait):
        with pytest.raises(_native.DemiError, match="no call in flight with ticket 0"):
            wait(0)
        with pytest.raises(_native.DemiError, match="no call in flight with ticket 123456"):
            wait(123456)
    r = ctx.replay_batch_submit(masks, lim)
    k = ctx.random_explore_submit(100, w.lim, seed_base=SEED_BASE)
    assert r != k and r > 0 and k > 0
    with pytest.raises(_native.DemiError, match="ticket %d is a random-explore ticket" % k) as e:
        ctx.replay_batch_wait(k)
    assert e.value.code == T.ERR_INVALID_ARG
    with pytest.raises(_native.DemiError, match="ticket %d is a replay ticket" % r) as e:
        ctx.random_explore_wait(r)
    assert e.value.code == T.ERR_INVALID_ARG
    check_flagged(want, ctx.replay_batch_wait(r), 0)        # (the refusals consumed neither ticket)
    ctx.random_explore_wait(k)
    for wait, t in ((ctx.replay_batch_wait, r), (ctx.random_explore_wait, k)):
        with pytest.raises(_native.DemiError, match="no call in flight with ticket %d" % t):
            wait(t)
    # a failed submit leaves no slot busy: three more fit afterwards, and the context works
    for _ in range(4):
        with pytest.raises(_native.DemiError):
            ctx.replay_batch_submit(masks, T.Limits(0, 0, 64, 0, 0, 0))         # (no target fingerprint)
    tickets = [ctx.replay_batch_submit(masks, lim) for _ in range(3)]
    for t in tickets:
        out = np.zeros(len(masks), dtype=T.VERDICT_DTYPE)
        check_flagged(want, ctx.replay_batch_wait(t, out=out), 0)
        same(out, want)


# ---------------------------------------------------------------------------------------------- 10. STSScheduler
def test_sts_scheduler_in_chunks_returns_what_one_call_returns(oracle, narrow):
    from demi_amd.schedulers import EventTrace, STSScheduler, SchedulerConfig, ViolationFingerprint
    w = narrow["config2"]
    rng = np.random.default_rng(12)
    subseqs = [tuple(range(len(w.used)))] + [tuple(int(i) for i in np.nonzero(rng.random(len(w.used)) < rng.choice([0.5, 0.8, 0.95]))[0])
                                             for _ in range(999)]
    sts = STSScheduler(SchedulerConfig(model=w.model), EventTrace(w.rec, w.used))
    try:
        fp = ViolationFingerprint(w.fingerprint)
        assert sts.chunk == 1 << 20
        one = sts.test_batch(subseqs, fp)
        v_one = sts.verdicts(subseqs, fp)
        sts.chunk = 300
        assert sts.test_batch(subseqs, fp) == one
        same(sts.verdicts(subseqs, fp), v_one)
        assert one[0] and not all(one)
        masks = sts._masks(subseqs)
        same(v_one, w.want(oracle, masks, sts._limits(fp)))
    finally:
        sts.shutdown()
