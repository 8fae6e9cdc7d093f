"""GPU suite of the fuzz campaign for messages with more than two fields: k_fuzz_generate_fields against the host mirror byte for
byte (events and payload areas), K1 with a workgroup per test and the tests' areas against the plain path (trace_load(events,
areas) + random_explore per test) and the CPU oracle with the same areas, and the campaign against fuzz() driven by the mirror.
The cases and what they must contain are tests/fuzz_fields_cases.py's, asserted in tests/test_fuzz_fields_cpu.py."""
import os

import numpy as np
import pytest

from demi_amd import _native, fuzzer as F, model as M, types as T
from demi_amd.runner_utils import fuzz, fuzz_campaign
from demi_amd.schedulers import FullyRandom, RandomScheduler, SchedulerConfig, SrcDstFIFO

from . import fuzz_campaign_cases as FC
from . import fuzz_fields_cases as FF

pytestmark = pytest.mark.gpu
EMU = os.environ.get("DEMI_EMU") == "1"
OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF


@pytest.fixture(scope="module")
def ctxs():
    """one context per table, specialised where asked (the hiprtc compile is paid once per table)"""
    made = {}

    def get(name, model_ctor, specialize):
        if name not in made:
            made[name] = _native.Context(0)
            made[name].model_load(model_ctor().to_struct())
            if specialize:
                made[name].model_specialize()
        return made[name]
    yield get
    for c in made.values():
        c.close()


def _case_ctx(ctxs, case):
    return ctxs(case.name, case.model_ctor, True)


def _flags_of(verdicts):
    return (1 if (verdicts["flags"] & T.V_VIOLATION).any() else 0) | (2 if (verdicts["flags"] & OVF).any() else 0)


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("npay", [3, 4, 5, 6])
def test_generated_tests_and_areas_equal_the_mirror(ctxs, npay, explicit):
    """the widths 16 / 12 / 9 / 8; 65 tests = a full wave and a wave of one lane, then a launch of one test; an alternative of two
    fields beside one of the table's full count; CONST at 2^W - 1 in a middle field, RANDOM with bounds that are no powers of two
    in the fields 2 and 3 (one explicit seed takes nextInt's retry inside such a draw), COUNTER in field 5; stride 255.
    COUNTER's mask is NOT reached here and cannot be: a test holds fewer than 256 Sends and the narrowest field has 8 bits."""
    cfg = FF.GenConfig(npay)
    ctx = ctxs("pay%d" % npay, lambda: FF.pay_table(npay), False)                  # (the generator is no specialised kernel)
    seeds = FF.gen_seeds(npay, explicit)
    if explicit:
        assert set(FF.rejected_bounds(cfg, FF.field_rejecting_seed(npay))) & set(FF.FIELD_BOUNDS)      # the mirror: the retry happens
    want = FF.mirror_tests(npay, explicit)
    for n in (FF.N_TESTS, 1):
        ev, ar, n_ev, n_b = ctx.fuzz_generate(n, cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, cfg.postfix, seed_base=FF.SEED_BASE,
                                              seeds=seeds[:n] if explicit else None)
        assert ev.shape == ar.shape == (n, 255)
        assert n_ev.tolist() == [len(e) for e, _ in want[:n]]
        assert n_b.tolist() == [FC.n_batches(e) for e, _ in want[:n]]
        wev, war = FF.packed(want[:n], cfg.stride)
        assert ev.tobytes() == wev.tobytes()                                        # the tail of every row is zero
        assert ar.tobytes() == war.tobytes()
    assert (war != 0).sum() > 100 and ((war >> np.uint64(2 * T.payload_bits(npay))) != 0).any()


def test_generator_refusals_by_name(ctxs):
    w = F.FuzzerWeights()
    prefix = [F.start(a) for a in range(5)]

    class Raw(F.FieldSendGenerator):
        """a generator struct the mirror would refuse: built field by field, without the mirror's own checks"""

        def __init__(self, fields, n_fields=None):
            self.fields, self.n_fields = fields, len(fields) if n_fields is None else n_fields

        def to_struct(self):
            s = np.zeros(1, dtype=F.FIELD_GEN_DTYPE)
            s["n_alts"] = 1
            a = s["alts"][0][0]
            a["msg_type"], a["target_kind"], a["target_actor"], a["n_fields"] = 0, F.TARGET_FIXED, 0, self.n_fields
            for k, (kind, arg) in enumerate(self.fields):
                a["kind"][k], a["arg"][k] = kind, arg
            return s

    def refused(ctx, what, fields, n_fields=None):
        with pytest.raises(_native.DemiError) as e:
            ctx.fuzz_generate(2, 6, w, Raw(fields, n_fields), prefix)
        assert what in str(e.value), str(e.value)

    pay4 = ctxs("pay4", lambda: FF.pay_table(4), False)
    refused(pay4, "describes 5 fields", [F.CONST(0)] * 5)                                 # more fields than the table has
    refused(pay4, "describes 7 fields", [F.CONST(0)] * 4, n_fields=7)
    refused(pay4, "CONST(4096) does not fit 12 bits", [F.CONST(0), F.CONST(0), F.CONST(4096)])
    refused(pay4, "RANDOM(0)", [F.CONST(0), F.CONST(0), F.CONST(0), F.RANDOM(0)])
    refused(pay4, "RANDOM(257)", [F.RANDOM(257)])
    refused(pay4, "unknown field kind 3", [F.CONST(0), (3, 0)])
    pay6 = ctxs("pay6", lambda: FF.pay_table(6), False)
    refused(pay6, "CONST(256) does not fit 8 bits", [F.CONST(0)] * 5 + [F.CONST(256)])
    narrow = ctxs("raft5", lambda: M.raft_model(5), False)
    refused(narrow, "no DEMI_MODEL_PAYLOADS", [F.CONST(0)] * 3)                           # three fields on a table of two
    refused(narrow, "CONST(256) does not fit 8 bits", [F.CONST(256)])
    # what demi_fuzz_generate refuses, this entry point refuses in the same words
    with pytest.raises(_native.DemiError, match="without a Start"):
        pay4.fuzz_generate(2, 6, w, FF.mixed_gen(4), [])
    # the unspecialised DEMI_MODEL_PAYLOADS table: generated, but not explored
    raw = _native.Context(0)
    try:
        raw.model_load(FF.ledger_model().to_struct())
        raw.fuzz_generate(2, 6, w, FF.ledger_gen(), [F.start(a) for a in range(4)])
        with pytest.raises(_native.DemiError, match="compiled table"):
            raw.random_explore_tests(None, 4, FF.LEDGER.limits(), n_tests=2, with_areas=True)
        with pytest.raises(_native.DemiError, match="compiled table"):
            raw.fuzz_campaign(6, w, FF.ledger_gen(), [F.start(a) for a in range(4)], FF.LEDGER.limits(), max_tests=4)
        # ... and the two-field entry points keep refusing it by name
        with pytest.raises(_native.DemiError, match="DEMI_MODEL_PAYLOADS"):
            raw.random_explore_tests(None, 4, FF.LEDGER.limits(), n_tests=2)
    finally:
        raw.close()


# ------------------------------------------------------------------------------------------------ K1 with a workgroup per test
_plain = {}


def _plain_path(ctx, case, strategy, epc, with_areas=True):
    """trace_load(events, areas) + random_explore per test, once per variant"""
    key = (case.name, strategy, epc, with_areas)
    if key not in _plain:
        out = []
        for ev, ar in case.tests():
            ctx.trace_load(ev, ar if with_areas else None)
            out.append(ctx.random_explore(epc, case.limits(strategy), seed_base=FF.K1_SEED_BASE))
        _plain[key] = out
    return _plain[key]


def _wide_rows(case):
    """the case's tests as host arrays with a stride LARGER than the longest test (a kernel that indexes rows by the launch's
    n_ev instead of the stride reads the wrong row)"""
    tests = case.tests()
    stride = max(len(e) for e, _ in tests) + 5
    ev = np.zeros((len(tests), stride), dtype=T.EXT_EVENT_DTYPE)
    ar = np.zeros((len(tests), stride), dtype=np.uint64)
    for i, (e, a) in enumerate(tests):
        ev[i, :len(e)], ar[i, :len(a)] = e, a
    return ev, ar, [len(e) for e, _ in tests]


@pytest.mark.parametrize("epc", [1, 70])
@pytest.mark.parametrize("strategy", [T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO])
@pytest.mark.parametrize("name", list(FF.K1_CASES))
def test_tests_launch_with_areas_equals_the_plain_path_and_the_oracle(ctxs, monkeypatch, name, strategy, epc):
    case = FF.K1_CASES[name]
    ctx = _case_ctx(ctxs, case)
    lim = case.limits(strategy)
    if EMU:
        epc = min(epc, 66)
    want = case.oracle(strategy, epc)
    plain = _plain_path(ctx, case, strategy, epc)
    ev, ar, n_ev = _wide_rows(case)
    for lanes in (1, 64):
        monkeypatch.setenv("DEMI_K1_LANES_PER_WAVE", str(lanes))
        v, f = ctx.random_explore_tests(ev, epc, lim, seed_base=FF.K1_SEED_BASE, n_ev=n_ev, areas=ar)
        monkeypatch.delenv("DEMI_K1_LANES_PER_WAVE")
        assert v.shape == (3, epc)
        for i in range(3):
            assert v[i].tobytes() == plain[i].tobytes() == want[i].tobytes(), (lanes, i)
            assert int(f[i]) == _flags_of(want[i]), (lanes, i)
    # a list of per-test arrays is packed by the binding: the same answer
    v2, f2 = ctx.random_explore_tests([e for e, _ in case.tests()], epc, lim, seed_base=FF.K1_SEED_BASE, areas=[a for _, a in case.tests()])
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()


@pytest.mark.parametrize("strategy", [T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO])
def test_a_violation_that_depends_on_a_field_beyond_the_second(ctxs, strategy):
    """the ledger's invariant breaks when the memo - field 3 of a Deposit - is booked: with the tests' areas the flag is set, with
    areas = NULL (P0 / P1 only, what a load without staged areas makes) it is not; a kernel that ignores test_areas fails here"""
    case, epc = FF.LEDGER, 70 if not EMU else 66
    ctx = _case_ctx(ctxs, case)
    lim = case.limits(strategy)
    ev, ar, n_ev = _wide_rows(case)
    v, f = ctx.random_explore_tests(ev, epc, lim, seed_base=FF.K1_SEED_BASE, n_ev=n_ev, areas=ar)
    assert (f & 1).all() and any(0 < int((x["flags"] & T.V_VIOLATION).sum()) < epc for x in v)
    v0, f0 = ctx.random_explore_tests(ev, epc, lim, seed_base=FF.K1_SEED_BASE, n_ev=n_ev, with_areas=True)
    assert not (f0 & 1).any() and not (v0["flags"] & T.V_VIOLATION).any()
    plain0, want0 = _plain_path(ctx, case, strategy, epc, with_areas=False), case.oracle(strategy, epc, False)
    for i in range(3):
        assert v0[i].tobytes() == plain0[i].tobytes() == want0[i].tobytes(), i


@pytest.mark.parametrize("name", list(FF.K1_CASES))
def test_resident_tests_and_areas_are_what_the_host_arrays_are(ctxs, name, oracle):
    """tests = NULL after demi_fuzz_generate_fields: events and areas explored without ever leaving the device"""
    case = FF.K1_CASES[name]
    ctx = _case_ctx(ctxs, case)
    n, epc, num_events = 3, 20, 12
    weights = F.FuzzerWeights(kill=0.1, send=0.5, wait_quiescence=0.1, partition=0.1, unpartition=0.1)
    ev, ar, n_ev, _ = ctx.fuzz_generate(n, num_events, weights, case.gen_ctor(), case.prefix, seed_base=FF.K1_SEED_BASE)
    for strategy in (T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO):
        lim = case.limits(strategy)
        v, f = ctx.random_explore_tests(None, epc, lim, seed_base=FF.K1_SEED_BASE, n_tests=n, with_areas=True)
        v2, f2 = ctx.random_explore_tests(ev, epc, lim, seed_base=FF.K1_SEED_BASE, n_ev=n_ev, areas=ar)
        assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()
        for i in range(n):
            mev, mar = F.generate_fuzz_test_fields(num_events, weights, case.gen_ctor(), case.prefix, FF.K1_SEED_BASE + i)
            assert F.array_to_events(ev[i, :n_ev[i]]) == mev and ar[i, :n_ev[i]].tolist() == mar
            try:
                oracle.set_ext_areas(ar[i, :n_ev[i]])
                want = oracle.random_explore(case.model(), ev[i, :n_ev[i]], epc, seed_base=FF.K1_SEED_BASE, limits=lim)
            finally:
                oracle.set_ext_areas(None)
            assert v[i].tobytes() == want.tobytes() and int(f[i]) == _flags_of(want), (strategy, i)
    # the ledger again: the resident areas matter
    if name == "ledger":
        assert any(int(a) >> 18 for a in ar.ravel())


def test_two_field_generator_on_the_narrow_table_gives_the_old_entry_points_bytes(ctxs):
    """a FieldSendGenerator of two-field alternatives on raft5 through the three new entry points: events, verdicts, flags and the
    campaign's result are the old entry points'; the areas of a table without DEMI_MODEL_PAYLOADS are zero"""
    cfg = FC.RAFT5
    ctx = ctxs("raft5", lambda: M.raft_model(5), False)
    old = cfg.gen()
    new = F.FieldSendGenerator([(m, t, [p0, p1]) for m, t, p0, p1 in old.alternatives], M.raft_model(5))
    n, epc = (40, 16) if not EMU else (6, 8)
    ev0, n_ev0, n_b0 = ctx.fuzz_generate(n, cfg.num_events, cfg.weights, old, cfg.prefix, seed_base=FC.SEED_BASE)
    v0, f0 = ctx.random_explore_tests(None, epc, FC.k1_limits(), seed_base=FC.K1_SEED_BASE, n_tests=n)
    ev1, ar1, n_ev1, n_b1 = ctx.fuzz_generate(n, cfg.num_events, cfg.weights, new, cfg.prefix, seed_base=FC.SEED_BASE)
    v1, f1 = ctx.random_explore_tests(None, epc, FC.k1_limits(), seed_base=FC.K1_SEED_BASE, n_tests=n, with_areas=True)
    assert ev1.tobytes() == ev0.tobytes() and n_ev1.tolist() == n_ev0.tolist() and n_b1.tolist() == n_b0.tolist() and not ar1.any()
    assert v1.tobytes() == v0.tobytes() and f1.tobytes() == f0.tobytes()
    v2, f2 = ctx.random_explore_tests(ev1, epc, FC.k1_limits(), seed_base=FC.K1_SEED_BASE, n_ev=n_ev1, areas=ar1)
    assert v2.tobytes() == v0.tobytes() and f2.tobytes() == f0.tobytes()
    if not EMU:
        from .test_fuzz_campaign_gpu import CAMPAIGN_EPC, CAMPAIGN_SEED
        lim = T.Limits(200, 30, 64, 0, 0, 0)
        kw = dict(executions_per_test=CAMPAIGN_EPC, tests_per_launch=8, max_tests=40, test_seed_base=CAMPAIGN_SEED)
        r0, e0 = ctx.fuzz_campaign(cfg.num_events, cfg.weights, old, cfg.prefix, lim, **kw)
        r1, e1, a1 = ctx.fuzz_campaign(cfg.num_events, cfg.weights, new, cfg.prefix, lim, **kw)
        assert bytes(r0) == bytes(r1) and r1.found and e1.tobytes() == e0.tobytes() and not a1.any()


# ------------------------------------------------------------------------------------------------ the campaign
def _campaign_args():
    return (FF.CAMPAIGN_NUM_EVENTS, FF.CAMPAIGN_WEIGHTS, FF.campaign_gen(), FF.CAMPAIGN_PREFIX)


def test_campaign_result_and_the_found_tests_areas(ctxs, oracle):
    """tests_per_launch = 4, the first violating test is test 5: found in the second launch; its events and areas are the ones of a
    host loop over the mirror's tests"""
    ctx = _case_ctx(ctxs, FF.LEDGER)
    lim = FF.campaign_limits()
    res, ev, ar = ctx.fuzz_campaign(*_campaign_args(), lim, executions_per_test=FF.CAMPAIGN_EPC, tests_per_launch=4, max_tests=12,
                                    test_seed_base=FF.CAMPAIGN_SEED)
    assert (res.found, res.test_index, res.exec_index, res.launches, res.tests_run, res.capacity_aborts) == (1, FF.CAMPAIGN_TEST, FF.CAMPAIGN_EXEC, 2, 8, 0)
    # the host loop: the mirror's tests one after the other through the plain path
    first = None
    for i in range(12):
        mev, mar = FF.campaign_test(i)
        ctx.trace_load(mev, mar)
        v = ctx.random_explore(FF.CAMPAIGN_EPC, lim, seed_base=0)
        hit = np.nonzero(v["flags"] & T.V_VIOLATION)[0]
        if len(hit):
            first = (i, int(hit[0]), v[int(hit[0])])
            break
    assert first is not None and first[:2] == (res.test_index, res.exec_index)
    assert T.VERDICT_DTYPE.itemsize == len(bytes(res.verdict)) and bytes(res.verdict) == first[2].tobytes()
    assert ev.tobytes() == mev.tobytes() and ar.tobytes() == mar.tobytes() and res.n_events == len(mev)
    # no violating test among the first four: one launch, nothing found
    res, ev, ar = ctx.fuzz_campaign(*_campaign_args(), lim, executions_per_test=FF.CAMPAIGN_EPC, tests_per_launch=4, max_tests=4,
                                    test_seed_base=FF.CAMPAIGN_SEED)
    assert (res.found, res.launches, res.tests_run) == (0, 1, 4) and ev is None and ar is None


def _same(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return
    (t1, v1, i1, f1), (t2, v2, i2, f2) = a, b
    assert t1.events.tobytes() == t2.events.tobytes() and t1.original_externals.tobytes() == t2.original_externals.tobytes()
    assert t1.ext_areas is not None and t1.ext_areas.tobytes() == t2.ext_areas.tobytes()
    assert v1 == v2 and i1.tobytes() == i2.tobytes() and f1.tobytes() == f2.tobytes()


def test_campaign_equals_fuzz_driven_by_the_mirror_on_one_context(ctxs):
    """runner_utils.fuzz_campaign with a FieldSendGenerator against fuzz() over generate_fuzz_test_fields' (events, areas), both
    strategies on ONE caller's context: the table is compiled once, the context is still open afterwards.  (fuzz() builds a
    scheduler per test; here they share the module's context, so that the table is not compiled once per test.)"""
    ctx = _case_ctx(ctxs, FF.LEDGER)
    model = FF.ledger_model()
    sc = SchedulerConfig(model=model)

    class Shared(RandomScheduler):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._ctx.close()
            self._ctx, self._loaded_model = ctx, True

        def shutdown(self):
            pass

    kw = dict(maxMessages=FF.CAMPAIGN_MAX_MESSAGES, invariant_check_interval=1, executions_per_test=FF.CAMPAIGN_EPC)
    for strategy_ctor, exec_index in ((FullyRandom, FF.CAMPAIGN_EXEC), (SrcDstFIFO, 2)):
        want = fuzz(FF.campaign_test, sc, max_tests=12, randomizationStrategyCtor=strategy_ctor, scheduler_ctor=Shared, provenance_device=0, **kw)
        got = fuzz_campaign(_campaign_args(), sc, max_tests=12, tests_per_launch=4, test_seed_base=FF.CAMPAIGN_SEED,
                            randomizationStrategyCtor=strategy_ctor, ctx=ctx, **kw)
        assert want is not None
        _same(got, want)
        mev, mar = FF.campaign_test(FF.CAMPAIGN_TEST)
        n = len(got[0].original_externals)
        assert got[0].original_externals.tobytes() == mev[:n].tobytes() and got[0].ext_areas.tobytes() == mar[:n].tobytes()
        # a campaign without a violation returns None, as fuzz() does
        assert fuzz(FF.campaign_test, sc, max_tests=4, randomizationStrategyCtor=strategy_ctor, scheduler_ctor=Shared, **kw) is None
        assert fuzz_campaign(_campaign_args(), sc, max_tests=4, tests_per_launch=4, test_seed_base=FF.CAMPAIGN_SEED,
                             randomizationStrategyCtor=strategy_ctor, ctx=ctx, **kw) is None
    # the caller's context is still open and still specialised
    assert ctx.is_specialized()
    ctx.trace_load(*FF.campaign_test(0))
    assert len(ctx.random_explore(4, FF.campaign_limits(), seed_base=0)) == 4
