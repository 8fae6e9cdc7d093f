"""GPU parity suite at the limits include/demi_gpu.h declares and on the paths random inputs never reach - everything bit for
bit against the CPU oracle (which tests/test_limits_cpu.py holds against the literal Scala transliterations on the same inputs):
  * the limits tables of tests/limit_tables.py (32 message types, 4 classes, 4 timer types with ids up to 31, 900 .. 1024 rows;
    8 actors narrow and wide, 16 actors in the BIG layout) through K1 in every variant, K2 in every DEMI_K2_MODE with demi_ddmin,
    the wildcard replay with type sets that hold bit 31, K3 in both orders and k_provenance;
  * crafted seeds whose k-th scheduler draw takes the retry branch of java.util.Random.nextInt(bound) (jr_next_int), through
    every K1 variant;
  * every capacity from both sides: a tiny model that reaches exactly DEMI_FX_CAP / DEMI_TQ_CAP / DEMI_RESEND_CAP / p_max /
    DEMI_DPOR_MAX_TRACE carries no overflow flag, one more does - the expected flag written down by hand and asserted on the
    oracle as well;
  * the two launchable K1 variants without a parity test so far: the re-binned kernel (DEMI_K1_REBIN=1) and the compiled kernels
    with LDS-resident pending slots (DEMI_JIT_K1_HOT / DEMI_JIT_K1S_HOT above 0).
Out of reach: DEMI_OP_RND's retry path (the application's generator restarts at seed 0 in every execution, so no rejection can
be placed in it)."""
import os

import numpy as np
import pytest

from demi_amd import _native, types as T
from demi_amd import model as M
from demi_amd.apps import raft5_config2
from demi_amd.fuzzer import events_to_array, send, start, wait_quiescence
from demi_amd.model import Asm, build_model

from . import limit_tables as LT
from .test_k1_gpu import assert_same

pytestmark = pytest.mark.gpu

EMU = os.environ.get("DEMI_EMU") == "1"
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF
CPUS = min(16, os.cpu_count() or 1)


def _workload(layout, n_events=64):
    model = LT.limits_model(LT.SEEDS[layout], layout)
    return model, LT.limits_trace(LT.SEEDS[layout], model, n_events), LT.limits_of(layout, n_events)


def _lim(lim, **kw):
    l = T.Limits(lim.max_messages, lim.invariant_check_interval, lim.p_max, lim.looking_for_valid, lim.looking_for, lim.populate_all,
                 lim.strategy, lim.filter_known_absents, lim.executions_per_instance)
    for k, v in kw.items():
        setattr(l, k, v)
    return l


def _same_trace(got, want):
    (gv, grec), (ov, orec) = got, want[:2]
    assert (int(gv.flags), int(gv.fingerprint), int(gv.hash)) == (int(ov.flags), int(ov.fingerprint), int(ov.hash))
    assert len(grec) == len(orec) and (grec == orec).all()


def _every_k1_variant(ctx, oracle, model, events, lim, sizes, monkeypatch, seeds=None, traced=4, with_fifo=True):
    """The loaded (interpreted or specialised) table through K1 plain, SrcDstFIFO, SPREAD forced to 1 and 3 lanes (both
    strategies), the carried-generator mode, the recording kernel, the candidate-frontier kernel and submit / wait - each against
    the oracle.  seeds: explicit seeds (one per schedule; the first ones per instance, trace, candidate batch and ticket)."""
    def explore(n, l):
        k = max(1, int(l.executions_per_instance))
        sd = None if seeds is None else np.asarray(seeds[:(n + k - 1) // k], dtype=np.uint64)
        g = ctx.random_explore(n, l, seed_base=777, seeds=sd)
        assert_same(g, oracle.random_explore(model, events, n, seed_base=777, seeds=sd, limits=l, n_threads=CPUS))
        return g
    fifo = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO)
    for n in sizes:
        n = n if seeds is None else min(n, len(seeds))
        monkeypatch.setenv("DEMI_K1_NO_SPREAD", "1")
        monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE", raising=False)
        plain = explore(n, lim)
        plain_fifo = explore(n, fifo) if with_fifo else None
        monkeypatch.delenv("DEMI_K1_NO_SPREAD")
        for lanes in (1, 3):
            monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", str(lanes))
            assert_same(explore(n, lim), plain)
            if with_fifo:
                assert_same(explore(n, fifo), plain_fifo)
        monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE")
        for l in (lim, fifo) if with_fifo else (lim,):
            explore(n, _lim(l, executions_per_instance=4))
    # the recording kernel, both strategies, independent and carried
    for s in ([777 + i for i in range(traced)] if seeds is None else [int(x) for x in seeds[:traced]]):
        for l in (lim, fifo) if with_fifo else (lim,):
            _same_trace(ctx.random_get_trace(s, l), oracle.random_execute(model, events, s, l))
        lc = _lim(lim, executions_per_instance=4)
        v, rec, ran = ctx.random_get_trace_carried(s, 2, lc)
        ov, orec, oran = oracle.random_execute_carried(model, events, s, 2, lc)
        assert ran == oran
        _same_trace((v, rec), (ov, orec))
    # the candidate-frontier kernel (what demi_random_ddmin launches): a workgroup per subsequence of the externals
    n_ev, execs = len(events), 24 if EMU else 96
    rng = np.random.default_rng(5)
    masks = np.zeros((4, 4), dtype=np.uint64)
    keep = [np.ones(n_ev, dtype=bool)] + [(rng.random(n_ev) < 0.8) | (events["kind"] == T.EV_START) for _ in range(3)]
    for i, kp in enumerate(keep):
        for j in np.nonzero(kp)[0]:
            masks[i, j // 64] |= np.uint64(1) << np.uint64(j % 64)
    base = 777 if seeds is None else int(seeds[0])
    gv, gf = ctx.random_explore_candidates(masks, execs, lim, seed_base=base)
    for i, kp in enumerate(keep):
        c = oracle.random_explore(model, events[kp], execs, seed_base=base, limits=lim, n_threads=CPUS)
        assert_same(gv[i], c)
        assert bool(gf[i] & 1) == bool((c["flags"] & T.V_VIOLATION).any()) and bool(gf[i] & 2) == bool((c["flags"] & OVF).any())
    # submit / wait: three tickets in flight
    n = 65
    bases = [777 + 1000 * k for k in range(3)] if seeds is None else [int(x) for x in seeds[:3]]
    tickets = [ctx.random_explore_submit(n, lim, seed_base=b, flag_mask=T.V_VIOLATION, want_verdicts=True) for b in bases]
    for b, t in zip(bases, tickets):
        out = np.zeros(n, dtype=T.VERDICT_DTYPE)
        fl, cnt, _first = ctx.random_explore_wait(t, out=out)
        c = oracle.random_explore(model, events, n, seed_base=b, limits=lim, n_threads=CPUS)
        assert_same(out, c)
        assert cnt == int(((c["flags"] & T.V_VIOLATION) != 0).sum())


def _fresh(model, events=None, specialise=True):
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if events is not None:
        ctx.trace_load(events)
    if specialise:
        ctx.model_specialize()
        assert ctx.is_specialized()
    return ctx


# ======================================================================================================== limits tables
def test_model_load_refuses_one_step_beyond_each_limit(gpu_ctx, oracle):
    """33 message types, 5 classes, 1025 rows, 5 timer types: demi_model_load names the limit, as the oracle does."""
    for what, match in LT.beyond_the_limits():
        model = what(LT.limits_model(LT.SEEDS["narrow"], "narrow"))
        assert oracle.model_validate(model)[0] == T.ERR_INVALID_MODEL
        with pytest.raises(_native.DemiError, match=match):
            gpu_ctx.model_load(model.to_struct())


@pytest.mark.parametrize("layout,specialise", [("narrow", False), ("narrow", True), ("wide", True), ("big", True)])
def test_limits_tables_through_every_k1_variant(oracle, monkeypatch, layout, specialise):
    """K1 on a table at the limits: 64-bit `tix_packed` (timer ids 18, 27, 31), the timer directory with NTT = 4, timer bit 31
    (narrow, wide: actor 7, timer index 3) / 63 (big: actor 15), type ids up to 31 in the message word, 128 handler starts,
    LDS sized for ~970 rows - and the 255-event trace.  (SrcDstFIFO on the BIG table: the test below.)"""
    model, events, lim = _workload(layout)
    big = layout == "big"
    ctx = _fresh(model, events, specialise)
    try:
        _every_k1_variant(ctx, oracle, model, events, lim, (1, 65, 300) if EMU else (1, 65, 4000), monkeypatch, with_fifo=not big)
        long_events, long_lim = LT.limits_trace(LT.SEEDS[layout], model, T.MAX_EXT_EVENTS), LT.limits_of(layout, T.MAX_EXT_EVENTS)
        ctx.trace_load(long_events)
        n = 64 if EMU else 2000
        for l in (long_lim,) if big else (long_lim, _lim(long_lim, strategy=T.STRATEGY_SRC_DST_FIFO)):
            assert_same(ctx.random_explore(n, l, seed_base=1000), oracle.random_explore(model, long_events, n, seed_base=1000, limits=l, n_threads=CPUS))
        _same_trace(ctx.random_get_trace(1003, long_lim), oracle.random_execute(model, long_events, 1003, long_lim))
    finally:
        ctx.close()


@pytest.mark.parametrize("specialise", [False, True])
def test_three_timer_types_at_ids_up_to_31(oracle, monkeypatch, specialise):
    """The limits table with THREE timer types (ids 5, 18, 31; id 27 internal): the timer directory entry rcv * NTT + index and
    the timer bit rcv * DEMI_MAX_TIMER_TYPES + index differ only when NTT < 4, so a confusion of the two is invisible on the
    four-timer tables - here NTT = 3, through every K1 variant, one K2 batch and a short K3 exploration."""
    # a small table first, one that has an effect-slot schedule (the compiled K1 then forms timer bits in the slots as well)
    msgs = [("Kick", T.MSG_EXTERNAL), ("Ping", T.MSG_INTERNAL), ("Ta", T.MSG_TIMER), ("Tb", T.MSG_TIMER), ("Rc", T.MSG_TIMER)]
    kick = Asm().and_(M.T0, M.P0, 3).if_eq(M.T0, 0, "a").tset(2).trep(4).label("a").if_eq(M.T0, 1, "b").tset(3).tcancel(4).label("b")
    kick.if_eq(M.T0, 2, "c").tcancel(2).trep(4).bcast(1, M.P0, 1).label("c").if_eq(M.T0, 3, "d").tcancel(3).tset(2).label("d")
    h = {(0, "Kick"): kick, (0, "Ping"): Asm().add(M.F[0], M.F[0], 1).skipz(M.P1, "x").tset(3).label("x"),
         (0, "Ta"): Asm().add(M.F[1], M.F[1], 1).tcancel(4), (0, "Tb"): Asm().add(M.F[2], M.F[2], 1),
         (0, "Rc"): Asm().add(M.F[3], M.F[3], 1).ge(M.T0, M.F[3], 9).skipz(M.T0, "z").tcancel(4).label("z")}
    small = build_model("three_timers", 8, msgs, h, [[0] * 8] * 8, (T.INV_NEVER, 3, 7, 0))
    rng = np.random.default_rng(23)
    sev = [start(a) for a in range(8)]
    for _ in range(90):
        sev.append(wait_quiescence() if rng.integers(6) == 0 and sev[-1][0] != T.EV_WAIT_QUIESCENCE else send(int(rng.integers(8)), 0, int(rng.integers(8))))
    sev, slim = events_to_array(sev), T.Limits(400, 7, 128, 0, 0, 0)
    ctx = _fresh(small, sev, specialise)
    try:
        _every_k1_variant(ctx, oracle, small, sev, slim, (300,) if EMU else (4000,), monkeypatch)
        c = oracle.random_explore(small, sev, 300, seed_base=777, limits=slim)
        assert len(np.unique(c["hash"])) > 250 and not (c["flags"] & OVF).any()
    finally:
        ctx.close()
    model = LT.limits_model(LT.SEEDS["narrow"], "narrow", n_timer_types=3)
    assert sum(c == T.MSG_TIMER for c in model.msg_class) == 3 and oracle.model_validate(model) == (0, "")
    events, lim = LT.limits_trace(LT.SEEDS["narrow"], model), LT.limits_of("narrow")
    ctx = _fresh(model, events, specialise)
    try:
        _every_k1_variant(ctx, oracle, model, events, lim, (65, 300) if EMU else (65, 4000), monkeypatch)
        ov, rec, _ = oracle.random_execute(model, events, 1001, lim)
        used = events[:T.verdict_trace_idx(int(ov.flags))]
        lr = T.Limits(0, 0, T.MAX_PENDING, 1, 0x1000103, 0)
        masks = _random_masks(np.random.default_rng(4), 96 if EMU else 1000, len(used))
        ctx.replay_load(used, rec)
        assert_same(ctx.replay_batch(masks, lr), oracle.sts_replay_batch(model, used, rec, masks, lr, n_threads=CPUS))
        dev = LT.limits_trace(LT.SEEDS["narrow"], model, model.n_actors + 6, dpor=True)
        par, srch = T.DporParams(40, 200, 0, 0, 64, 4096, 0), T.DporSearch(64, 200 if EMU else 2000, 0, 1, T.DPOR_ORDER_ROUNDS)
        ctx.dpor_load(dev)
        g, c = ctx.dpor_explore(par, srch), oracle.dpor_explore(model, dev, par, srch, CPUS)
        assert len(g[0]) == len(c[0]) and (g[0] == c[0]).all() and (g[1] == c[1]).all()
    finally:
        ctx.close()


def test_srcdst_fifo_on_big_limits_tables_up_to_the_lds_budget(oracle, monkeypatch):
    """FINDING: a BIG table of ~970 rows without an effect-slot schedule does not fit the 160 KB of LDS under SrcDstFIFO (256
    (src, dst) queues per schedule next to 16 wide actor states): the launch is refused BY NAME - DEMI_ERR_INVALID_ARG, "LDS
    budget exceeded" - never run short.  Largest accepted shapes of the limits table, SrcDstFIFO without recording: 14 actors
    under a 64-event trace (15: 166 112 bytes, 16: 171 200), 13 actors under the 255-event trace (14: 166 832); the recording
    SrcDstFIFO kernel is refused from 12 actors on (167 392 bytes).  FullyRandom runs all of them at 16 actors (the test above).
    So: the refusal is asserted at 16 actors, and the largest accepted shapes run every SrcDstFIFO variant against the oracle."""
    model, events, lim = _workload("big")
    fifo = _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO)
    ctx = _fresh(model, events)
    try:
        with pytest.raises(_native.DemiError, match="LDS budget exceeded"):
            ctx.random_explore(65, fifo, seed_base=777)
        with pytest.raises(_native.DemiError, match="LDS budget exceeded"):
            ctx.random_get_trace(777, fifo)
        assert_same(ctx.random_explore(65, lim, seed_base=777), oracle.random_explore(model, events, 65, seed_base=777, limits=lim))   # (the context is intact)
    finally:
        ctx.close()
    for n_actors, n_events in ((14, 64), (13, T.MAX_EXT_EVENTS)):
        model = LT.limits_model(LT.SEEDS["big"], "big", n_actors=n_actors)
        events = LT.limits_trace(LT.SEEDS["big"], model, n_events)
        fifo = _lim(LT.limits_of("big", n_events), strategy=T.STRATEGY_SRC_DST_FIFO)
        assert oracle.model_validate(model) == (0, "") and len(model.code) >= 900
        ctx = _fresh(model, events)
        try:
            monkeypatch.setenv("DEMI_K1_NO_SPREAD", "1")
            n = 300 if EMU else 4000
            c = oracle.random_explore(model, events, n, seed_base=777, limits=fifo, n_threads=CPUS)
            assert_same(ctx.random_explore(n, fifo, seed_base=777), c)
            assert len(np.unique(c["hash"])) >= 10
            monkeypatch.delenv("DEMI_K1_NO_SPREAD")
            monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", "3")
            assert_same(ctx.random_explore(n, fifo, seed_base=777), c)
            monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE")
            lc = _lim(fifo, executions_per_instance=4)
            assert_same(ctx.random_explore(n, lc, seed_base=777), oracle.random_explore(model, events, n, seed_base=777, limits=lc, n_threads=CPUS))
            with pytest.raises(_native.DemiError, match="LDS budget exceeded"):
                ctx.random_get_trace(777, fifo)
        finally:
            ctx.close()


def _violating_execution(oracle, model, events, lim):
    """-> (the limits it ran under, its seed, verdict, recorded trace): the first execution that stops at a violated check."""
    l0 = _lim(lim)
    v = oracle.random_explore(model, events, 2000, seed_base=1000, limits=l0, n_threads=CPUS)
    idx = int(np.nonzero(((v["flags"] & T.V_VIOLATION) != 0) & ((v["flags"] & OVF) == 0))[0][0])
    vd, rec, _ = oracle.random_execute(model, events, 1000 + idx, l0)
    return l0, 1000 + idx, vd, rec


def _random_masks(rng, n, n_ev):
    masks = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) | (rng.integers(0, 2, size=(n, 4), dtype=np.uint64) << np.uint64(63))
    masks[1:n // 3] |= rng.integers(0, 2**63, size=(n // 3 - 1, 4), dtype=np.uint64)
    masks[0] = 0xFFFFFFFFFFFFFFFF
    return masks


@pytest.mark.parametrize("k2_mode", ["auto", "wave", "lds", "hbm", "scan"])
@pytest.mark.parametrize("layout,specialise", [("narrow", False), ("narrow", True), ("wide", True), ("big", True)])
def test_limits_tables_replay_in_every_k2_mode(oracle, monkeypatch, layout, specialise, k2_mode):
    """K2 over a violating recorded execution of a limits table: replay_batch under the three filterKnownAbsents settings and
    replay_removal_batch, in every DEMI_K2_MODE (a compiled-only table replays with the scanning kernel whatever the mode)."""
    if k2_mode == "scan":
        monkeypatch.setenv("DEMI_K2_SCAN", "1")
    elif k2_mode != "auto":
        monkeypatch.setenv("DEMI_K2_MODE", k2_mode)
    model, events, lim = _workload(layout)
    l0, seed, vd, orec = _violating_execution(oracle, model, events, lim)
    ctx = _fresh(model, events, specialise)
    try:
        gv, rec = ctx.random_get_trace(seed, l0)
        _same_trace((gv, rec), (vd, orec))
        used = events[:T.verdict_trace_idx(int(vd.flags))]
        lr = T.Limits(0, 0, l0.p_max, 1, int(vd.fingerprint), 0)
        n = 96 if EMU else 1500
        masks = _random_masks(np.random.default_rng(3), n, len(used))
        ctx.replay_load(used, rec)
        for fk in (0, 1, 2):
            lr.filter_known_absents = fk
            g = ctx.replay_batch(masks, lr)
            assert_same(g, oracle.sts_replay_batch(model, used, rec, masks, lr, n_threads=CPUS))
            assert g[0]["flags"] & T.V_VIOLATION and not g[0]["flags"] & T.V_DIVERGED
        lr.filter_known_absents = 0
        skips = np.nonzero(rec["kind"] == T.REC_MSG_EVENT)[0].astype(np.uint32)
        skips = np.concatenate([skips[:: max(1, len(skips) // (40 if EMU else 400))], np.array([0xFFFFFFFF], dtype=np.uint32)])
        assert_same(ctx.replay_removal_batch(skips, lr), oracle.sts_removal_batch(model, used, rec, skips, lr))
        for sk in (int(skips[1]), 0xFFFFFFFF):
            gk, ok = ctx.replay_get_kept(len(rec), sk, lr), oracle.sts_removal_kept(model, used, rec, sk, lr)
            assert (gk[0].flags, gk[0].hash) == (ok[0].flags, ok[0].hash) and (gk[1] == ok[1]).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", LT.LAYOUTS)
def test_limits_tables_ddmin_end_to_end(oracle, layout):
    """demi_ddmin over a violating execution of a limits table = the same loop around the oracle's replay: MCS, consultations."""
    model, events, lim = _workload(layout)
    l0, seed, vd, rec = _violating_execution(oracle, model, events, lim)
    used = events[:T.verdict_trace_idx(int(vd.flags))]
    lr = T.Limits(0, 0, T.MAX_PENDING, 1, int(vd.fingerprint), 0)
    ctx = _fresh(model, events)
    try:
        ctx.replay_load(used, rec)
        mcs, consulted, _batches, st = ctx.ddmin(lr)
        omcs, oconsulted, _ob, ost = oracle.ddmin(model, used, rec, lr, n_threads=CPUS)
        assert mcs == omcs and consulted == oconsulted and 0 < len(mcs) < len(used) and st.verified == ost.verified
    finally:
        ctx.close()


@pytest.mark.parametrize("layout,specialise", [("narrow", False), ("narrow", True), ("wide", True)])
def test_wildcards_whose_type_set_holds_bit_31(oracle, layout, specialise):
    """k2_replay_wildcard with selectors that name message type 31 (the top bit of the uint32 type set): every timer delivery
    is a wildcard over all four timer types, every internal one over its own type, type 29 and - never pending between actors,
    but part of the mask - type 31; held against the transliterated STSScheduler as tests/test_wildcard_gpu.py does."""
    from demi_amd.schedulers import EventTrace, ViolationFingerprint
    from . import test_wildcard_transliteration_cpu as X
    model, events, lim = _workload(layout)
    l0, seed, vd, rec = _violating_execution(oracle, model, events, lim)
    used = events[:T.verdict_trace_idx(int(vd.flags))]
    trace, fp = EventTrace(rec, used), ViolationFingerprint(int(vd.fingerprint))
    is_ev = rec["kind"] == T.REC_MSG_EVENT
    cls = np.array([model.msg_class[int(t)] for t in rec["msg_type"]])
    timer_set = sum(1 << t for t in LT.TIMER_TYPES)
    ts = np.where(is_ev & (cls == T.MSG_TIMER), timer_set,
                  np.where(is_ev & (cls == T.MSG_INTERNAL), (np.uint64(1) << rec["msg_type"].astype(np.uint64)) | (1 << 29) | (1 << 31), 0)).astype(np.uint32)
    assert (ts >> 31).any() and ((ts & (1 << 29)) != 0).any()
    rng = np.random.default_rng(9)
    wild_ev = is_ev & (cls != T.MSG_EXTERNAL)
    presents = [np.ones(len(rec), dtype=bool)] + [~wild_ev | (rng.random(len(rec)) < p) for p in (0.97, 0.9, 0.8) for _ in range(2 if EMU else 6)]
    rl = T.Limits(0, 0, T.MAX_PENDING, 1, fp.code, 0, 0, 0)
    ctx = _fresh(model, None, specialise)
    try:
        ctx.replay_load(used, rec)
        for policy in (T.WILDCARD_HEAD, T.WILDCARD_FIRST, T.WILDCARD_LAST):
            po = np.full(len(rec), policy, dtype=np.uint8)
            ctx.replay_wildcard_load(ts, po)
            got = ctx.replay_wildcard_batch(np.array(presents), rl)
            assert not (got["flags"] & OVF).any()
            wild = X.wildcards_of(ts, po)
            for k, present in enumerate(presents):
                v, kept, executed, _ignored, _s = X.run_candidate(oracle, model, trace, fp, wild, present)
                assert (int(got["flags"][k]), int(got["fingerprint"][k]), int(got["hash"][k])) == v, (policy, k)
                if k % 5 == 0:
                    v1, kept1, rec1 = ctx.replay_wildcard_get_trace(present, rl)
                    assert (int(v1.flags), int(v1.fingerprint), int(v1.hash)) == v and (kept1 == kept).all()
                    assert len(rec1) == len(executed) and rec1.tobytes() == executed.tobytes()
    finally:
        ctx.close()


def _dpor_workload(layout):
    model = LT.limits_model(LT.SEEDS[layout], layout)
    return model, LT.limits_trace(LT.SEEDS[layout], model, model.n_actors + 6, dpor=True)


@pytest.mark.parametrize("layout,specialise", [("narrow", False), ("narrow", True), ("wide", True), ("big", True)])
def test_limits_tables_dpor_in_both_orders(oracle, layout, specialise):
    """K3 on a limits table under a DPOR-valid trace (Start / Send / WaitQuiescence): per-interleaving verdicts, traces and racing
    pairs of the prefixes an oracle-backed exploration launches, then a short native exploration in ROUNDS order against the
    oracle's and in the reference's order against the oracle one backtrack point at a time."""
    from .test_k3_gpu import collect_prefixes, same_batch
    model, ev = _dpor_workload(layout)
    prefixes, _res, _d = collect_prefixes(oracle, model, ev, 40, 32, 96 if EMU else 400)
    assert len(prefixes) >= 16
    par = T.DporParams(40, 200, 0, 0, 128 if layout == "big" else 64, 4096, 0)
    ctx = _fresh(model, None, specialise)
    try:
        ctx.dpor_load(ev)
        same_batch(ctx.dpor_batch(prefixes, par), oracle.dpor_batch(model, ev, prefixes, par))
        for order, budget, batch in ((T.DPOR_ORDER_ROUNDS, 300 if EMU else 3000, 64), (T.DPOR_ORDER_REFERENCE, 100 if EMU else 600, 32)):
            g = ctx.dpor_explore(par, T.DporSearch(batch, budget, 0, 1, order))
            if order == T.DPOR_ORDER_ROUNDS:
                c = oracle.dpor_explore(model, ev, par, T.DporSearch(batch, budget, 0, 1, T.DPOR_ORDER_ROUNDS), CPUS)
            else:
                c = oracle.dpor_explore(model, ev, par, T.DporSearch(1, budget, 0, 1, T.DPOR_ORDER_ROUNDS), 1)
            assert len(g[0]) == len(c[0]) and (g[0] == c[0]).all() and (g[1] == c[1]).all(), order
            assert len(g[0]) >= 16
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", LT.LAYOUTS)
def test_limits_tables_provenance(oracle, layout):
    """k_provenance over recorded executions of a limits table (type ids up to 31 in the words the node keys hash) against the
    host class."""
    from demi_amd.incremental_ddmin import dpor_initial_trace
    from demi_amd.provenance import ProvenanceTracker, pruneConcurrentEventsBatch
    from demi_amd.schedulers import EventTrace
    model, events, lim = _workload(layout)
    big = layout == "big"
    ctx = _fresh(model, events)
    try:
        traces, affected = [], []
        for s in range(1000, 1040):
            vv, rec = ctx.random_get_trace(s, _lim(lim, max_messages=120))
            it = dpor_initial_trace(EventTrace(rec, events[:T.verdict_trace_idx(vv.flags)]), model)
            if len(it) <= T.DPOR_MAX_TRACE:
                traces.append(it)
                affected.append([model.n_actors - 1, s % model.n_actors])
            if len(traces) >= (6 if EMU else 30):
                break
        assert len(traces) >= 4
        got = pruneConcurrentEventsBatch(ctx, traces, affected)
        kept_some = 0
        for tr, aff, k in zip(traces, affected, got):
            w = tr[ProvenanceTracker(tr, big=big).pruneConcurrentEvents(aff)]
            assert len(k) == len(w) and (k == w).all()
            kept_some += int(0 < len(k) < len(tr))
        assert kept_some >= 1
    finally:
        ctx.close()


# ======================================================================================================== crafted seeds
@pytest.mark.parametrize("workload,specialise", [("raft5", False), ("raft5", True), ("limits", False), ("limits", True)])
def test_crafted_seeds_through_every_k1_variant(oracle, monkeypatch, workload, specialise):
    """Seeds whose k-th scheduler draw is rejected by nextInt(bound) (tests/test_limits_cpu.py counts, in the transliteration,
    that at least 64 of these candidates per strategy really retry, at every call site: FullyRandom's draw, SrcDstFIFO's draw
    over all messages, its pair draw and timersAndExternals' generator) as explicit `seeds=` through every K1 variant: a kernel
    that returned r - q * bound without drawing again passes everything else in the suite and fails here."""
    if workload == "raft5":
        model, events, lim = raft5_config2()
    else:
        model, events, lim = _workload("narrow")
    seeds = np.array(LT.candidate_seeds(), dtype=np.uint64)
    ctx = _fresh(model, events, specialise)
    try:
        _every_k1_variant(ctx, oracle, model, events, lim, (len(seeds),), monkeypatch, seeds=seeds, traced=12 if EMU else 48)
    finally:
        ctx.close()


# ======================================================================================================== capacity edges
CAP_MSGS = [("Kick", T.MSG_EXTERNAL), ("Arm", T.MSG_EXTERNAL), ("Ping", T.MSG_INTERNAL), ("T1", T.MSG_TIMER), ("T2", T.MSG_TIMER),
            ("T3", T.MSG_TIMER), ("RT", T.MSG_TIMER)]
C_KICK, C_ARM, C_PING, C_T1, C_T2, C_T3, C_RT = range(7)
NO_INV = (T.INV_NONE, 0, 0, 0)


def _capacity_cases():
    """[(name, model, events, limits, expected low flag byte of EVERY execution)] - the expectations are reasoned here, by hand:
    fx        n SEND rows in one delivery: DEMI_FX_CAP = 8 effect rows fit, the ninth aborts (V_QUEUE_OVF);
    tq        Arm arms the repeating timer RT; its delivery retriggers it into timersToResend (it was just scheduled), the
              pending set is empty, the trace goes on to Kick, whose scheduling step hands RT to messagesToSend (1 entry) before
              the handler adds n one-shot T1: 1 + 7 = DEMI_TQ_CAP fit, 1 + 8 abort - with 8 effect rows, so it is not FX_CAP;
    tq-plain  n one-shot sets in one delivery: 8 fit both capacities, 9 abort;
    resend    three actors arm 3 + 3 + 2 (or 3) repeating timers; after the last Arm every timer is delivered once, each
              retriggered into timersToResend (nothing else is delivered in between): 8 = DEMI_RESEND_CAP fit, 9 abort;
    pmax      n external Sends injected at once with p_max = 16: 16 pending fit, 17 abort (V_PENDING_OVF)."""
    cases = []
    for n, want in ((T_FX_CAP, 0), (T_FX_CAP + 1, T.V_QUEUE_OVF)):
        a = Asm()
        for _ in range(n):
            a.send(C_PING, M.ME, M.T0, 0)
        m = build_model("cap_fx%d" % n, 2, CAP_MSGS, {(0, "Kick"): a}, [[0] * 8] * 2, NO_INV)
        cases.append(("fx%d" % n, m, events_to_array([start(0), send(0, C_KICK)]), T.Limits(0, 0, 64, 0, 0, 0), want))
    for n, want in ((T_TQ_CAP - 1, 0), (T_TQ_CAP, T.V_QUEUE_OVF)):
        a = Asm()
        for _ in range(n):
            a.tset(C_T1)
        m = build_model("cap_tq%d" % n, 2, CAP_MSGS, {(0, "Kick"): a, (0, "Arm"): Asm().trep(C_RT)}, [[0] * 8] * 2, NO_INV)
        ev = events_to_array([start(0), send(0, C_ARM), wait_quiescence(), send(0, C_KICK)])
        cases.append(("tq1+%d" % n, m, ev, T.Limits(40, 0, 64, 0, 0, 0), want))
    for n, want in ((T_TQ_CAP, 0), (T_TQ_CAP + 1, T.V_QUEUE_OVF)):
        a = Asm()
        for _ in range(n):
            a.tset(C_T1)
        m = build_model("cap_tqp%d" % n, 2, CAP_MSGS, {(0, "Kick"): a}, [[0] * 8] * 2, NO_INV)
        cases.append(("tq-plain%d" % n, m, events_to_array([start(0), send(0, C_KICK)]), T.Limits(40, 0, 64, 0, 0, 0), want))
    arm = Asm().trep(C_T1).trep(C_T2).skipz(M.P0, "x").trep(C_T3).label("x")
    m = build_model("cap_resend", 3, CAP_MSGS, {(0, "Arm"): arm}, [[0] * 8] * 3, NO_INV)
    for third, want in ((0, 0), (1, T.V_QUEUE_OVF)):
        ev = events_to_array([start(a) for a in range(3)] + [send(0, C_ARM, 1), send(1, C_ARM, 1), send(2, C_ARM, third)])
        cases.append(("resend%d" % (T_RESEND_CAP + third), m, ev, T.Limits(60, 0, 64, 0, 0, 0), want))
    m = build_model("cap_pmax", 1, CAP_MSGS, {(0, "Kick"): Asm().add(M.F[0], M.F[0], 1)}, [[0] * 8], NO_INV)
    for n, want in ((16, 0), (17, T.V_PENDING_OVF)):
        cases.append(("pmax%d" % n, m, events_to_array([start(0)] + [send(0, C_KICK, i) for i in range(n)]), T.Limits(0, 0, 16, 0, 0, 0), want))
    return cases


T_FX_CAP = T_TQ_CAP = T_RESEND_CAP = 8          # DEMI_FX_CAP, DEMI_TQ_CAP, DEMI_RESEND_CAP of include/demi_gpu.h


@pytest.mark.parametrize("specialise", [False, True])
def test_every_k1_capacity_from_both_sides(oracle, monkeypatch, specialise):
    """Exactly the capacity: no overflow flag; one more: the flag - on the oracle and on K1 plain, SrcDstFIFO, SPREAD, carried
    and recording, interpreted and compiled.  An off-by-one would turn valid executions into 'verdict invalid' silently."""
    for name, model, ev, lim, want in _capacity_cases():
        ctx = _fresh(model, ev, specialise)
        try:
            variants = [lim, _lim(lim, strategy=T.STRATEGY_SRC_DST_FIFO), _lim(lim, executions_per_instance=3)]
            for l in variants:
                for lanes in (None, 1):
                    if lanes:
                        monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", "1")
                    else:
                        monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE", raising=False)
                    g = ctx.random_explore(66, l, seed_base=5)
                    c = oracle.random_explore(model, ev, 66, seed_base=5, limits=l)
                    assert ((c["flags"] & 0xFF) == want).all(), (name, "oracle")
                    assert_same(g, c)
            monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE", raising=False)
            whole = np.zeros((1, 4), dtype=np.uint64)
            whole[0, 0] = (1 << len(ev)) - 1
            gv, gf = ctx.random_explore_candidates(whole, 8, lim, seed_base=5)          # the candidate-frontier kernel
            assert ((gv[0]["flags"] & 0xFF) == want).all() and bool(gf[0] & 2) == bool(want), name
            out = np.zeros(9, dtype=T.VERDICT_DTYPE)
            ctx.random_explore_wait(ctx.random_explore_submit(9, lim, seed_base=5, want_verdicts=True), out=out)      # submit / wait
            assert_same(out, oracle.random_explore(model, ev, 9, seed_base=5, limits=lim))
            v, rec = ctx.random_get_trace(5, lim)
            ov, orec, _ = oracle.random_execute(model, ev, 5, lim)
            assert int(v.flags) & 0xFF == want and (int(v.flags), int(v.hash)) == (int(ov.flags), int(ov.hash)), name
            assert len(rec) == len(orec) and (rec == orec).all()
        finally:
            ctx.close()


def _k2_beyond_cases():
    """[(name, model, events, max_messages of the recording)]: F0 starts at 1 and the external Arm clears it; the recorded
    execution [Start, Arm, WaitQuiescence, Kick] stays at the capacity, the candidate WITHOUT the Arm goes one beyond:
    fx   Kick runs 8 SEND rows and a ninth under `F0 != 0`: 8 = DEMI_FX_CAP recorded, 9 replayed -> V_QUEUE_OVF;
    tq   Kick arms the repeating timer RT, whose delivery retriggers it (1 entry of messagesToSend) and runs 7 one-shot sets and
         an eighth under `F0 != 0`: 1 + 7 = DEMI_TQ_CAP recorded, 1 + 8 replayed -> V_QUEUE_OVF with 8 effect rows (not FX_CAP)."""
    ev = events_to_array([start(0), send(0, C_ARM), wait_quiescence(), send(0, C_KICK)])
    init = [[1] + [0] * 7] * 2
    a = Asm()
    for _ in range(T_FX_CAP):
        a.send(C_PING, M.ME, M.T0, 0)
    a.skipz(M.F[0], "e").send(C_PING, M.ME, M.T0, 0).label("e")
    fx = build_model("k2_fx", 2, CAP_MSGS, {(0, "Arm"): Asm().mov(M.F[0], 0), (0, "Kick"): a}, init, NO_INV)
    r = Asm()
    for _ in range(T_TQ_CAP - 1):
        r.tset(C_T1)
    r.skipz(M.F[0], "e").tset(C_T1).label("e")
    tq = build_model("k2_tq", 2, CAP_MSGS, {(0, "Arm"): Asm().mov(M.F[0], 0), (0, "Kick"): Asm().trep(C_RT), (0, "RT"): r}, init, NO_INV)
    return [("fx", fx, ev, 0), ("tq", tq, ev, 6)]


@pytest.mark.parametrize("specialise", [False, True])
def test_k2_capacities_at_the_edge(oracle, specialise):
    """K2 replays the executions that reach exactly a capacity without an overflow flag; the pending capacity from both sides
    (the 17 Sends replay with p_max = 17 and abort with p_max = 16); and DEMI_FX_CAP / DEMI_TQ_CAP one step beyond, which a
    replayed SUBSEQUENCE reaches where the recorded execution did not (_k2_beyond_cases).  The same candidates through the
    wildcard replay kernel with no wildcard loaded (its own copy of the checks)."""
    for name, model, ev, mm in _k2_beyond_cases():
        ov, rec, _ = oracle.random_execute(model, ev, 5, T.Limits(mm, 0, 64, 0, 0, 0))
        assert not int(ov.flags) & OVF
        masks = np.full((2, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        masks[1, 0] &= ~np.uint64(2)                       # candidate 1: without the Arm (external event 1)
        l = T.Limits(0, 0, 64, 1, 0x1000103, 0)
        ctx = _fresh(model, ev, specialise)
        try:
            ctx.replay_load(ev, rec)
            g, c = ctx.replay_batch(masks, l), oracle.sts_replay_batch(model, ev, rec, masks, l)
            assert [int(f) & 0xFF for f in c["flags"]] == [0, T.V_QUEUE_OVF], (name, "oracle")      # written by hand
            assert_same(g, c)
            ctx.replay_wildcard_load(np.zeros(len(rec), dtype=np.uint32), np.zeros(len(rec), dtype=np.uint8))
            w = ctx.replay_wildcard_batch(np.ones((2, len(rec)), dtype=bool), l, masks=masks)
            assert [int(f) & 0xFF for f in w["flags"]] == [0, T.V_QUEUE_OVF], (name, "wildcard kernel")
            assert int(w[0]["hash"]) == int(c[0]["hash"])
        finally:
            ctx.close()
    for name, model, ev, lim, want in _capacity_cases():
        if want and not name.startswith("pmax"):
            continue
        rlim = T.Limits(lim.max_messages, 0, 64, 0, 0, 0)
        ov, rec, _ = oracle.random_execute(model, ev, 5, rlim)
        assert not int(ov.flags) & 0xFF
        n_kick = int((ev["kind"] == T.EV_SEND).sum())
        ctx = _fresh(model, ev, specialise)
        try:
            ctx.replay_load(ev, rec)
            masks = np.full((3, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            for p_max, flag in ((64, 0),) + (((n_kick, 0), (n_kick - 1, T.V_PENDING_OVF)) if name == "pmax17" else ()):
                l = T.Limits(0, 0, p_max, 1, 0x1000103, 0)      # (a replay needs a target fingerprint; these models have no invariant)
                g = ctx.replay_batch(masks, l)
                c = oracle.sts_replay_batch(model, ev, rec, masks, l)
                assert ((c["flags"] & 0xFF) == flag).all(), (name, p_max, "oracle")
                assert_same(g, c)
                if not flag:
                    assert int(g[0]["hash"]) == int(ov.hash)
        finally:
            ctx.close()


@pytest.mark.parametrize("specialise", [False, True])
def test_k3_capacities_from_both_sides(oracle, specialise):
    """K3: DEMI_FX_CAP and p_max as in K1, and DEMI_DPOR_MAX_TRACE = 256 entries: a chain Kick(p0) -> Ping(p0) -> ... -> Ping(0)
    records the Start, the Kick and p0 + 1 Pings - 256 entries for p0 = 253 (no flag, 256 entries back), 257 for p0 = 254
    (V_TRACE_OVF)."""
    chain = build_model("cap_chain", 2, CAP_MSGS, {(0, "Kick"): Asm().send(C_PING, M.ME, M.P0, 0),
                                                   (0, "Ping"): Asm().skipz(M.P0, "e").sub(M.T0, M.P0, 1).send(C_PING, M.ME, M.T0, 0).label("e")},
                        [[0] * 8] * 2, NO_INV)
    cases = [("trace%d" % (p0 + 3), chain, events_to_array([start(0), send(0, C_KICK, p0)]), T.DporParams(0, 0, 0, 0, 64, 4096, 0), want, n)
             for p0, want, n in ((253, 0, T.DPOR_MAX_TRACE), (254, T.V_TRACE_OVF, 0))]
    for name, model, ev, lim, want in _capacity_cases():
        if name.startswith("fx") or name.startswith("pmax"):
            cases.append((name, model, ev, T.DporParams(0, 0, 0, 0, lim.p_max, 4096, 0), want, None))
    root = [np.zeros(0, dtype=np.uint64)]
    for name, model, ev, par, want, n_trace in cases:
        ctx = _fresh(model, None, specialise)
        try:
            ctx.dpor_load(ev)
            g, c = ctx.dpor_batch(root, par), oracle.dpor_batch(model, ev, root, par)
            assert int(c[0]["flags"][0]) & 0xFF == want, (name, "oracle", hex(int(c[0]["flags"][0])))
            assert n_trace is None or len(c[1][0]) == n_trace
            assert (g[0] == c[0]).all() and len(g[1][0]) == len(c[1][0]) and (g[1][0] == c[1][0]).all(), name
            assert len(g[2][0]) == len(c[2][0]) and (g[2][0] == c[2][0]).all()
        finally:
            ctx.close()


# ======================================================================================================== K1 variants without a test
def _k1_launch_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("[k1 launch]")]


@pytest.mark.parametrize("workload", ["raft5", "limits"])
def test_rebinned_kernel_against_the_plain_launch_and_the_oracle(oracle, monkeypatch, capfd, workload):
    """DEMI_K1_REBIN=1 (JK_K1B: the compiled FullyRandom exploration that re-bins its lanes by handler class): the same
    verdicts as the plain launch and the oracle; the launch line says which kernel ran."""
    if workload == "raft5":
        model, events, lim = raft5_config2()
    else:
        model, events, lim = _workload("narrow")
    monkeypatch.setenv("DEMI_K1_VERBOSE", "1")
    monkeypatch.setenv("DEMI_K1_NO_SPREAD", "1")
    # (the host launches the re-binned kernel only when its LDS leaves DEMI_K1_REBIN_MIN_WG workgroups per CU, 4 by default: the
    # ~970 rows of a limits table need 39 KB before the kernel's own lists, so the test asks for one workgroup per CU)
    monkeypatch.setenv("DEMI_K1_REBIN_MIN_WG", "1")
    ctx = _fresh(model, events)
    try:
        for n in (65, 700) if EMU else (1, 65, 20000):
            for p_max in (32, 64, 128):
                l = _lim(lim, p_max=p_max)
                monkeypatch.setenv("DEMI_K1_REBIN", "0")
                plain = ctx.random_explore(n, l, seed_base=777)
                assert "re-binned" not in " ".join(_k1_launch_lines(capfd))
                monkeypatch.setenv("DEMI_K1_REBIN", "1")
                g = ctx.random_explore(n, l, seed_base=777)
                lines = _k1_launch_lines(capfd)
                assert lines and "specialised, re-binned" in lines[0], lines
                assert_same(g, plain)
                assert_same(g, oracle.random_explore(model, events, n, seed_base=777, limits=l, n_threads=CPUS))
        seeds = np.array(LT.candidate_seeds(), dtype=np.uint64)
        g = ctx.random_explore(len(seeds), lim, seeds=seeds)
        assert "specialised, re-binned" in " ".join(_k1_launch_lines(capfd))
        assert_same(g, oracle.random_explore(model, events, len(seeds), seeds=seeds, limits=lim, n_threads=CPUS))
    finally:
        ctx.close()


@pytest.mark.parametrize("hot", [3, 11, 64])
@pytest.mark.parametrize("workload", ["raft5", "limits"])
def test_compiled_k1_with_lds_resident_pending_slots(oracle, monkeypatch, capfd, workload, hot):
    """DEMI_JIT_K1_HOT / DEMI_JIT_K1S_HOT above 0: the compiled K1 kernels keep the first `hot` pending slots of a schedule in
    LDS and the rest in scratch memory (default 0: every `slot < hot` branch is otherwise dead in the suite).  3 and 11 lie
    strictly between 0 and the largest pending set these workloads reach (asserted on the oracle's recorded executions), so
    the slots straddle both; 64 keeps a whole default pending set in LDS.  The knobs are read when the table is specialised
    AND when a launch is sized, so they stay set from model_specialize to the last launch of the context."""
    if workload == "raft5":
        model, events, lim = raft5_config2()
    else:
        model, events, lim = _workload("narrow")
    # the largest pending set of an execution: messages sent and not dropped, minus deliveries, along the recorded trace
    peak = 0
    for s in range(777, 783):
        _v, rec, _ = oracle.random_execute(model, events, s, _lim(lim, p_max=128))
        cur = 0
        for e in rec:
            if e["kind"] == T.REC_MSG_SEND and not int(e["flags"]) & 4:
                cur += 1
                peak = max(peak, cur)
            elif e["kind"] == T.REC_MSG_EVENT:
                cur -= 1
    assert peak > 11
    monkeypatch.setenv("DEMI_K1_VERBOSE", "1")
    monkeypatch.setenv("DEMI_JIT_K1_HOT", str(hot))
    monkeypatch.setenv("DEMI_JIT_K1S_HOT", str(hot))
    ctx = _fresh(model, events)
    try:
        ids = set()
        for p_max in (32, 64, 128):
            for strategy in (T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO):
                l = _lim(lim, p_max=p_max, strategy=strategy)
                for n, spread in ((65, "3"), (600 if EMU else 20000, None)):
                    if spread:
                        monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", spread)
                        monkeypatch.delenv("DEMI_K1_NO_SPREAD", raising=False)
                    else:
                        monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE", raising=False)
                        monkeypatch.setenv("DEMI_K1_NO_SPREAD", "1")
                    g = ctx.random_explore(n, l, seed_base=777)
                    lines = _k1_launch_lines(capfd)
                    assert lines and "specialised" in lines[0] and "hot=%d " % hot in lines[0], lines
                    assert (len(lines) == 2 and "spread: 3 lanes" in lines[1]) if spread else len(lines) == 1, lines
                    assert_same(g, oracle.random_explore(model, events, n, seed_base=777, limits=l, n_threads=CPUS))
        ids.add(ctx.code_id())
        seeds = np.array(LT.candidate_seeds(), dtype=np.uint64)
        assert_same(ctx.random_explore(len(seeds), lim, seeds=seeds), oracle.random_explore(model, events, len(seeds), seeds=seeds, limits=lim, n_threads=CPUS))
    finally:
        ctx.close()
    # another kernel than the default one: the code id of the table compiled without the knobs differs
    monkeypatch.delenv("DEMI_JIT_K1_HOT")
    monkeypatch.delenv("DEMI_JIT_K1S_HOT")
    ctx = _fresh(model, events)
    try:
        assert ctx.code_id() not in ids and ctx.code_id() != 0
    finally:
        ctx.close()
