"""CPU suite: the checker side of the limits tables (tests/limit_tables.py) - tables with DEMI_MAX_MSG_TYPES message types,
DEMI_MAX_CLASSES classes, DEMI_MAX_TIMER_TYPES timer types and 900 .. DEMI_MAX_CODE rows, and seeds that force the retry loop of
java.util.Random.nextInt(bound).  Pinned here, on the oracle and the literal Scala transliterations alone, so that the GPU
comparison of tests/test_limits_gpu.py means something:
  * the tables are valid, one step beyond each limit is refused by name;
  * the oracle's executions of them have the properties the tables were built for (few capacity aborts, distinct schedules,
    violations, all four timer types delivered, the timer with the top bit of the timer mask set and cancelled);
  * the oracle equals the transliterated RandomScheduler on them, FullyRandom and SrcDstFIFO;
  * the generated handlers equal the row interpreter on them, delivery by delivery, and the kernels compile for gfx950;
  * the crafted seeds really take nextInt's retry branch - counted in the transliteration - at every call site.
Out of reach: DEMI_OP_RND's retry path (the application's generator is seeded 0 in every execution: no rejection can be placed)."""
import ctypes as C

import numpy as np
import pytest

from demi_amd import _native, types as T
from demi_amd import model as M
from oracle.oracle_py import Effect

from . import limit_tables as LT
from .test_jit_cpu import FX_CAP, _host_vm
from .test_random_scheduler_transliteration_cpu import DEAD, ScalaRandomScheduler, _compare

OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF


def _workload(layout, n_events=64):
    model = LT.limits_model(LT.SEEDS[layout], layout)
    return model, LT.limits_trace(LT.SEEDS[layout], model, n_events), LT.limits_of(layout, n_events)


@pytest.mark.parametrize("layout", LT.LAYOUTS)
def test_limits_tables_are_valid_and_sit_at_the_declared_limits(oracle, layout):
    model, events, _ = _workload(layout)
    assert oracle.model_validate(model) == (0, "")
    assert model.n_actors == (T.MAX_ACTORS_BIG if layout == "big" else T.MAX_ACTORS) and model.wide == (layout != "narrow")
    assert model.n_msg_types == T.MAX_MSG_TYPES and model.n_classes == T.MAX_CLASSES and set(model.actor_class) == set(range(T.MAX_CLASSES))
    assert 900 <= len(model.code) <= T.MAX_CODE
    timers = [t for t, c in enumerate(model.msg_class) if c == T.MSG_TIMER]
    assert len(timers) == T.MAX_TIMER_TYPES and sum(t >= 16 for t in timers) >= 2 and 31 in timers
    assert any(t > 16 and c == T.MSG_INTERNAL for t, c in enumerate(model.msg_class))
    assert any(t >= 20 and c == T.MSG_EXTERNAL for t, c in enumerate(model.msg_class))
    assert sum(s != 0xFFFF for s in model.handler_start) >= T.MAX_CLASSES * T.MAX_MSG_TYPES - 3
    # SEND / BCAST rows name many internal types (ids above 16 among them), the timer rows all four timer types
    sent = {(r >> 17) & 0x7F for r in model.code[:model.inv_fa if model.inv_kind & T.INV_PROGRAM else None] if (r & 0xFF) in (M.OPS["SEND"], M.OPS["BCAST"])}
    timed = {(r >> 17) & 0x7F for r in model.code if (r & 0xFF) in (M.OPS["TSET"], M.OPS["TREP"], M.OPS["TCANCEL"])}
    assert len(sent) >= 16 and max(sent) > 16 and timed == set(timers)
    hi = 65535 if model.wide else 255
    assert any(int(e["p0"]) | int(e["p0_hi"]) << 8 == hi for e in events)
    for n_events in (64, T.MAX_EXT_EVENTS):
        ev = LT.limits_trace(LT.SEEDS[layout], model, n_events)
        assert len(ev) == n_events and oracle.trace_validate(model, ev) == (0, "")
        kinds = set(int(k) for k in ev["kind"])
        assert {T.EV_START, T.EV_SEND, T.EV_WAIT_QUIESCENCE, T.EV_KILL, T.EV_PARTITION} <= kinds
        assert set(int(a) for a in ev["a"][ev["kind"] == T.EV_START]) == set(range(model.n_actors))


def test_one_step_beyond_each_limit_is_refused_by_name(oracle):
    """33 message types, 5 classes, 1025 rows, 5 timer types: the oracle's orc_model_validate names the limit (the library's
    demi_model_load: tests/test_limits_gpu.py::test_model_load_refuses_one_step_beyond_each_limit, device and emulator)."""
    for what, match in LT.beyond_the_limits():
        model = what(LT.limits_model(LT.SEEDS["narrow"], "narrow"))
        code, msg = oracle.model_validate(model)
        assert code == T.ERR_INVALID_MODEL and match in msg, (match, code, msg)


class _Watching(ScalaRandomScheduler):
    """The transliterated RandomScheduler, noting which timers were armed and which cancels met an armed timer."""

    def __init__(self, *a, **kw):
        self.armed, self.cancelled = set(), set()
        super().__init__(*a, **kw)

    def registerCancellable(self, ongoingTimer, receiver, msg):
        self.armed.add((receiver, msg[0]))
        super().registerCancellable(ongoingTimer, receiver, msg)

    def notify_timer_cancel(self, rcv, msg):
        if self.handle_timer_cancel(rcv, msg) or self.pendingEvents.remove(DEAD, rcv, msg) is not None:
            self.cancelled.add((rcv, msg[0]))


@pytest.mark.parametrize("layout", LT.LAYOUTS)
def test_the_oracles_executions_have_the_properties_the_tables_were_built_for(oracle, layout):
    """The conditions on the chosen seeds and limits, on the ORACLE's output (and the transliteration's bookkeeping, which the
    oracle is held against in the same breath): at most 5 % capacity aborts, at least 90 % distinct hashes, violations, every
    timer type delivered, timer (actor 7 - 15 for big -, timer index 3) armed and cancelled while armed."""
    model, events, lim = _workload(layout)
    n = 4000
    for strategy in (T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO):
        l = T.Limits(lim.max_messages, lim.invariant_check_interval, lim.p_max, 0, 0, 0, strategy)
        v = oracle.random_explore(model, events, n, seed_base=1000, limits=l, n_threads=4)
        assert ((v["flags"] & OVF) != 0).sum() <= 0.05 * n
        assert len(np.unique(v["hash"])) >= 0.9 * n
        assert ((v["flags"] & T.V_VIOLATION) != 0).sum() >= 1
    long_model, long_events, long_lim = _workload(layout, T.MAX_EXT_EVENTS)
    v = oracle.random_explore(long_model, long_events, 1000, seed_base=1000, limits=long_lim, n_threads=4)
    assert ((v["flags"] & OVF) != 0).sum() <= 50 and len(np.unique(v["hash"])) >= 900
    delivered, armed, cancelled = set(), set(), set()
    top = (model.n_actors - 1, LT.TIMER_TYPES[3])
    for seed in range(1000, 1030):
        vv, rec, _ = oracle.random_execute(model, events, seed, lim)
        if vv.flags & OVF:
            continue
        ev = rec[rec["kind"] == T.REC_MSG_EVENT]
        delivered |= set(int(t) for t in ev["msg_type"])
        s = _Watching(oracle, model, events, seed, lim.max_messages, lim.invariant_check_interval)
        s.execute()
        assert (int(vv.flags), int(vv.fingerprint), int(vv.hash)) == s.verdict()
        armed |= s.armed
        cancelled |= s.cancelled
    assert set(LT.TIMER_TYPES) <= delivered
    assert len([t for t in delivered if t in LT.INTERNAL_TYPES and t > 16]) >= 1 and {20, 30} <= delivered
    assert top in armed and top in cancelled


@pytest.mark.parametrize("layout", LT.LAYOUTS)
def test_limits_tables_equal_the_scala_transliteration(oracle, layout):
    """Whole executions, delivery by delivery, verdict and hash: FullyRandom through _compare, SrcDstFIFO through the
    transliterated container (limit_tables.ScalaSrcDstFIFO) as the scheduler's pending set."""
    model, events, lim = _workload(layout)
    checked, violations = _compare(oracle, model, events, [5000 + 7919 * i for i in range(200)], lim.max_messages, lim.invariant_check_interval, p_max=lim.p_max)
    assert checked >= 190 and violations >= 1
    fifo = T.Limits(lim.max_messages, lim.invariant_check_interval, lim.p_max, 0, 0, 0, T.STRATEGY_SRC_DST_FIFO)
    checked = 0
    for seed in [9000 + 104729 * i for i in range(120)]:
        v, rec, _ = oracle.random_execute(model, events, seed, fifo)
        if v.flags & OVF:
            continue
        s, _counts = LT.srcdst_fifo_execution(oracle, model, events, seed, fifo)
        got = [(int(e["snd"]), int(e["rcv"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"])) for e in rec if e["kind"] == T.REC_MSG_EVENT]
        assert got == s.deliveries and (int(v.flags), int(v.fingerprint), int(v.hash)) == s.verdict(), seed
        checked += 1
    assert checked >= 110
    long_model, long_events, long_lim = _workload(layout, T.MAX_EXT_EVENTS)
    checked, _ = _compare(oracle, long_model, long_events, [77 + 31 * i for i in range(12)], long_lim.max_messages, long_lim.invariant_check_interval, p_max=long_lim.p_max)
    assert checked >= 10


@pytest.mark.parametrize("k1", [False, True], ids=["queue", "k1-schedule"])
@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_generated_handlers_equal_the_row_interpreter_on_limits_tables(oracle, tmp_path, layout, k1):
    """Random states x random messages of all 32 types to actors of all 4 classes: same new state, same effect rows, same
    FX_CAP overflow (tests/test_jit_cpu.py's comparison); k1: the RandomScheduler kernel's flavour with its effect-slot
    schedule, when the table has one."""
    model, _, _ = _workload(layout)
    wide = model.wide
    L = _host_vm(model, tmp_path, k1)
    sched = L.fx_schedule
    ms = model.to_struct()
    A, NT = model.n_actors, model.n_msg_types
    hs = np.full(T.MAX_CLASSES * T.MAX_MSG_TYPES, 0xFFFF, dtype=np.uint32)
    hs[:len(model.handler_start)] = model.handler_start
    ac = sum((c & 15) << (4 * i) for i, c in enumerate(model.actor_class))
    fw = 2 if wide else 1
    st = np.zeros(8 * fw * 64, dtype=np.uint64)
    fxq = np.zeros(FX_CAP * 64, dtype=np.uint64 if wide else np.uint32)
    fx = (Effect * 64)()
    want_state = (C.c_uint64 * fw)()
    hi = 65536 if wide else 256
    pb, pm = (16, 0xFFFF) if wide else (8, 0xFF)
    rng = np.random.default_rng(17)
    seen_fx, seen_types, seen_timer_rows = 0, set(), set()
    for it in range(40000):
        me, typ = int(rng.integers(A)), int(rng.integers(NT))
        src = int(rng.choice([int(rng.integers(A)), T.DEADLETTERS]))
        p0, p1 = [hi - 1 if rng.integers(8) == 0 else int(rng.integers(hi if it % 2 else 6)) for _ in range(2)]
        fields = [hi - 1 if rng.integers(16) == 0 else int(x) for x in (rng.integers(0, 6, 8) if it % 3 else rng.integers(0, hi, 8))]
        words = M.pack_state_wide(fields) if wide else [M.pack_state(fields)]
        for k, wv in enumerate(words):
            st[(fw * me + k) * 64] = wv
            want_state[k] = wv
        w = typ | (me << 5) | (src << 8) | (p0 << 16) | (p1 << (16 + pb))
        flags = C.c_uint32(0)
        n = L.run(hs.ctypes.data, ac, NT, st.ctypes.data, fxq.ctypes.data, w, C.byref(flags))
        wn = oracle.lib().orc_vm_run(C.byref(ms), me, want_state, typ, src, p0, p1, (1 << A) - 1, fx, 64, C.byref(L.app_rng))
        if wn < 0:
            assert flags.value & T.V_QUEUE_OVF
            continue
        assert not flags.value
        assert [int(st[(fw * me + k) * 64]) for k in range(fw)] == [int(x) for x in want_state], (it, me, typ, fields)
        got = []
        for k in (range(n) if sched is None else [j for j in range(len(sched)) if (n >> j) & 1]):
            f = int(fxq[(k if sched is None else sched[k][3]) * 64])
            op, t_, target, q0, q1 = f & 31, (f >> 5) & 31, (f >> 10) & 15, (f >> 14) & pm, (f >> (14 + pb)) & pm
            if sched is not None and sched[k][0] != 0:
                op, t_ = sched[k][1], sched[k][2]
            elif sched is not None:
                assert op in (M.OPS["SEND"], M.OPS["BCAST"])
            if op == M.OPS["SEND"]:
                if target < A:
                    got.append((0, target, t_, q0, q1))
            elif op == M.OPS["BCAST"]:
                got += [(0, r, t_, q0, q1) for r in range(A) if r != me]
            else:
                got.append((1 + op - M.OPS["TSET"], me, t_, 0, 0))
        assert got == [(e.kind, e.target, e.msg_type, e.p0, e.p1) for e in fx[:wn]], (it, me, typ, fields)
        seen_fx += len(got)
        seen_types |= {g[2] for g in got if g[0] == 0}
        seen_timer_rows |= {g[2] for g in got if g[0] != 0}
    assert seen_fx > 1000 and len(seen_types) >= 16 and max(seen_types) > 16 and seen_timer_rows == set(LT.TIMER_TYPES)


@pytest.mark.parametrize("layout", LT.LAYOUTS)
def test_limits_tables_compile_for_gfx950(layout):
    """Every kernel of the specialised translation unit - the 64-bit `tix_packed` of K1 (more than 16 message types), the
    type-of-timer-index packing of the BIG layout with four timer types - through the device-free demi_specialize_check."""
    model, _, _ = _workload(layout)
    try:
        size, kernel = _native.specialize_check(model.to_struct())
    except _native.DemiError as e:
        if "hiprtc not found" in str(e):
            pytest.skip("no hiprtc in this environment")
        raise
    assert size > 10000 and "k1_random_explore" in kernel and "k2_replay" in kernel and "k3_dpor" in kernel


def test_seed_rejecting_draw_inverts_the_generator():
    from demi_amd.fuzzer import JavaRandom
    for k in (1, 2, 7, 34):
        for bound in (3, 5, 6, 7, 100, 127):
            r = JavaRandom(LT.seed_rejecting_draw(k, low=12345))
            for _ in range(k - 1):
                r.next(31)
            assert r.next(31) == (1 << 31) - 1                       # ... which nextInt(bound) rejects:
            u = (1 << 31) - 1
            assert ((u - u % bound + bound - 1) & 0xFFFFFFFF) >= (1 << 31)
    # ... and a power of two never retries
    assert JavaRandom(LT.seed_rejecting_draw(1)).next_int(64) == 63


@pytest.mark.parametrize("workload", ["raft5", "limits"])
def test_crafted_seeds_take_the_retry_branch_at_every_call_site(oracle, workload):
    """The candidate seeds (the k-th step of the generator is the draw 2^31 - 1, k = 1 and seven values above) through the
    transliterations under a counting java.util.Random: at least 64 per strategy really retry at a bound that is no power of
    two; FullyRandom's draw (`rng`), and under SrcDstFIFO the draw over all messages, the draw of the (src, dst) pair and the
    draw of timersAndExternals' own generator (`te_rng`) are each hit; the oracle equals the transliteration on every one
    (asserted inside kept_seeds).  tests/test_limits_gpu.py runs the same candidates through every K1 variant."""
    if workload == "raft5":
        from demi_amd.apps import raft5_config2
        model, events, lim = raft5_config2()
    else:
        model, events, lim = _workload("narrow")
    cands = LT.candidate_seeds()
    first = set(cands[:48])                                           # (k = 1: the first draw)
    kept, sites = LT.kept_seeds(oracle, model, events, lim, T.STRATEGY_FULLY_RANDOM, cands)
    assert len(kept) >= 64 and sites.get("rng", 0) >= 64
    assert first & set(kept) and set(kept) - first
    kept, sites = LT.kept_seeds(oracle, model, events, lim, T.STRATEGY_SRC_DST_FIFO, cands)
    assert len(kept) >= 64 and min(sites.get(k, 0) for k in ("rng", "pair", "te_rng")) >= 1, sites
    assert first & set(kept) and set(kept) - first
