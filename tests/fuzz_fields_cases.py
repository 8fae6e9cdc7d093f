"""Shared inputs of the suites of the fuzz campaign for messages with more than two fields (tests/test_fuzz_fields_*.py): the
tables per field count, the generator configurations, the host mirror's tests for them (computed once per process), the K1 cases
and the campaign case.  What the cases must contain is asserted on the mirror and the oracle alone in
tests/test_fuzz_fields_cpu.py, so that a GPU comparison that passes has compared the paths it claims to."""
import functools

import numpy as np

from demi_amd import fuzzer as F, model as M, types as T

from . import fuzz_campaign_cases as FC
from .limit_tables import seed_rejecting_draw

N_TESTS = 65             # one full wave plus a wave of one lane
SEED_BASE = 0xF1E1D000
FIELD_BOUNDS = (13, 200)  # RANDOM bounds of fields >= 2: no powers of two, and no other draw of a test has them (sets hold <= 10)


@functools.lru_cache(maxsize=None)
def pay_table(npay):
    """a small random wide table with npay fields per message (the builder of tests/test_payloads_gpu.py's random tables)"""
    from .test_jit_cpu import _random_handler_payloads
    rng = np.random.default_rng(160 + npay)
    msgs = [("E", T.MSG_EXTERNAL), ("A", T.MSG_INTERNAL), ("B", T.MSG_INTERNAL), ("Tm", T.MSG_TIMER)]
    h = {(0, name): _random_handler_payloads(rng, int(rng.integers(3, 12)), len(msgs), npay) for name, _ in msgs}
    return M.build_model("fz_pay%d" % npay, 5, msgs, h, [[int(x) for x in rng.integers(0, 65536, 8)] for _ in range(5)],
                         (T.INV_NEVER, 0, 77, 0), wide=True, payloads=npay)


def full_fields(npay):
    """the alternative with the table's full field count: CONST at 2^W - 1 in a middle field (field 1; field 4 too from five
    fields on), RANDOM with bounds that are no powers of two in the fields 2 and 3, COUNTER in field 5"""
    top = (1 << T.payload_bits(npay)) - 1
    return [F.RANDOM(3), F.CONST(top), F.RANDOM(FIELD_BOUNDS[0]), F.RANDOM(FIELD_BOUNDS[1]), F.CONST(top), F.COUNTER][:npay]


def mixed_gen(npay):
    """an alternative of two fields and one of the table's full count: the lanes of a wave draw different numbers of values"""
    return F.FieldSendGenerator([(0, F.FIXED(1), [F.COUNTER, F.RANDOM(7)]), (0, F.RANDOM_ALIVE, full_fields(npay))], pay_table(npay))


class GenConfig:
    """stride 255: five Starts and a Send in the prefix, a Send in the postfix, 247 generated events, the final WaitQuiescence"""

    def __init__(self, npay):
        self.npay, self.n_actors = npay, 5
        self.prefix = [F.start(a) for a in range(5)] + [F.send(2, 0, 0xABCD, 0x1234)]
        self.postfix = [F.send(3, 0, 0xFFFF, 0x0F0F)]
        self.num_events = T.MAX_EXT_EVENTS - len(self.prefix) - len(self.postfix) - 1
        self.weights = F.FuzzerWeights(kill=0.004, send=0.5, wait_quiescence=0.1, partition=0.1, unpartition=0.1)

    @property
    def stride(self):
        return F.fuzz_stride(self.num_events, self.prefix, self.postfix)

    def gen(self):
        return mixed_gen(self.npay)


class _Logging(FC._Counting):
    """java.util.Random that also keeps the bound of every draw nextInt rejects"""

    def __init__(self, seed):
        super().__init__(seed)
        self.rejected_bounds = []

    def next_int(self, bound=None):
        before = self.rejected
        v = super().next_int(bound)
        self.rejected_bounds += [bound] * (self.rejected - before)
        return v


def rejected_bounds(cfg, seed):
    """the bounds at which the mirror's test of `seed` takes nextInt's retry"""
    made = []
    orig = F.JavaRandom

    def ctor(s):
        made.append(_Logging(s))
        return made[-1]
    F.JavaRandom = ctor
    try:
        F.generate_fuzz_test_fields(cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed, cfg.postfix)
    finally:
        F.JavaRandom = orig
    return made[0].rejected_bounds


@functools.lru_cache(maxsize=None)
def field_rejecting_seed(npay):
    """a seed of seed_rejecting_draw whose rejected draw falls into the draw of a field >= 2 (the first such k)"""
    cfg = GenConfig(npay)
    for low in range(0x155, 0x165):
        for k in range(3, 32):
            seed = seed_rejecting_draw(k, low=low + 16 * npay)
            if set(rejected_bounds(cfg, seed)) & set(FIELD_BOUNDS):
                return seed
    raise AssertionError("none of the candidate seeds rejects a draw inside a field")


def gen_seeds(npay, explicit, n=N_TESTS):
    if not explicit:
        return [SEED_BASE + i for i in range(n)]
    seeds = FC.explicit_seeds(n)
    seeds[n // 2] = field_rejecting_seed(npay)
    return seeds


@functools.lru_cache(maxsize=None)
def mirror_tests(npay, explicit=False, n=N_TESTS):
    """the mirror's n tests of GenConfig(npay): a tuple of (events, areas)"""
    cfg = GenConfig(npay)
    return tuple(tuple(map(tuple, F.generate_fuzz_test_fields(cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, s, cfg.postfix)))
                 for s in gen_seeds(npay, explicit, n))


def packed(tests, stride):
    """(events [n, stride], areas [n, stride]) of mirror tests, zero behind a test's length"""
    ev = np.zeros((len(tests), stride), dtype=T.EXT_EVENT_DTYPE)
    ar = np.zeros((len(tests), stride), dtype=np.uint64)
    for i, (e, a) in enumerate(tests):
        ev[i, :len(e)] = F.events_to_array(list(e))
        ar[i, :len(a)] = np.array(a, dtype=np.uint64)
    return ev, ar


# ---- K1 with a workgroup per test and the tests' areas: the ledger table of tests/test_payloads_gpu.py (its invariant breaks when
# a Deposit's FOURTH field, the memo 0x1A5, is booked) and the raft with akka-raft's field sets
MEMO = 0x1A5
K1_SEED_BASE = 0x5EED9000


@functools.lru_cache(maxsize=None)
def ledger_model():
    from .test_payloads_gpu import _ledger_model
    return _ledger_model()


@functools.lru_cache(maxsize=None)
def raft_fields_model():
    return M.raft_model(5, log_cap=8, real_fields=True)


def ledger_gen(memo_alts=1):
    """Deposits of five fields; `memo_alts` of the eight alternatives carry the memo in field 3"""
    plain = (0, F.RANDOM_ALIVE, [F.RANDOM(200), F.RANDOM(100), F.RANDOM(256), F.RANDOM(256), F.RANDOM(8)])
    memo = (0, F.FIXED(2), [F.COUNTER, F.RANDOM(100), F.CONST(5), F.CONST(MEMO), F.CONST(0)])
    return F.FieldSendGenerator([memo] * memo_alts + [plain] * (8 - memo_alts), ledger_model())


def raft_fields_gen():
    """ClientCommand with all five fields of the table described"""
    return F.FieldSendGenerator([(M.M_CLIENT, F.RANDOM_ALIVE, [F.COUNTER, F.CONST(0), F.RANDOM(13), F.RANDOM(200), F.CONST(511)])],
                                raft_fields_model())


class K1Case:
    def __init__(self, name, model, gen, prefix, weights, lengths, lim):
        self.name, self.model_ctor, self.gen_ctor, self.prefix, self.weights, self.lengths, self.lim = name, model, gen, prefix, weights, lengths, lim

    def model(self):
        return self.model_ctor()

    def limits(self, strategy=T.STRATEGY_FULLY_RANDOM):
        return T.Limits(self.lim[0], self.lim[1], 64, 0, 0, 0, strategy)

    @functools.lru_cache(maxsize=None)
    def tests(self):
        """three tests of different lengths (num_events differs): [(events array, areas array)]"""
        out = []
        for i, n in enumerate(self.lengths):
            ev, ar = F.generate_fuzz_test_fields(n, self.weights, self.gen_ctor(), self.prefix, K1_SEED_BASE + i)
            out.append((F.events_to_array(ev), np.array(ar, dtype=np.uint64)))
        return tuple(out)

    @functools.lru_cache(maxsize=None)
    def oracle(self, strategy, epc, with_areas=True):
        """the CPU oracle's verdicts per test (set_ext_areas + random_explore), computed once"""
        from oracle import oracle_py as O
        O.build()
        out = []
        try:
            for ev, ar in self.tests():
                O.set_ext_areas(ar if with_areas else None)
                out.append(O.random_explore(self.model(), ev, epc, seed_base=K1_SEED_BASE, limits=self.limits(strategy)))
        finally:
            O.set_ext_areas(None)
        return tuple(out)


_SENDS = F.FuzzerWeights(kill=0.02, send=0.5, wait_quiescence=0.15, partition=0.1, unpartition=0.1)
# (max_messages 4, the invariant checked after every delivery: which of a test's Deposits and Posts an execution delivers is the
# schedule's business)
LEDGER = K1Case("ledger", ledger_model, functools.partial(ledger_gen, 2), [F.start(a) for a in range(4)], _SENDS, (14, 5, 9), (4, 1))
RAFT_FIELDS = K1Case("raft_fields", raft_fields_model, raft_fields_gen, FC.raft_prefix(5), _SENDS, (12, 30, 4), (200, 30))
K1_CASES = {c.name: c for c in (LEDGER, RAFT_FIELDS)}


# ---- the campaign: the ledger table, one alternative of eight with the memo.  CAMPAIGN_SEED was chosen with the mirror and the oracle
# (tests/test_fuzz_fields_cpu.py asserts it): under CAMPAIGN_EPC executions per test (seeds 0 ..) the tests 0 .. CAMPAIGN_TEST - 1 are
# clean and test CAMPAIGN_TEST violates first in execution CAMPAIGN_EXEC - beyond the first launch of four tests
CAMPAIGN_NUM_EVENTS = 8
CAMPAIGN_WEIGHTS = F.FuzzerWeights(kill=0.02, send=0.4, wait_quiescence=0.15, partition=0.1, unpartition=0.1)
CAMPAIGN_PREFIX = [F.start(a) for a in range(4)]
CAMPAIGN_MAX_MESSAGES = 3       # (with the invariant checked after every delivery: whether the memo is among an execution's three is the schedule's business)
CAMPAIGN_EPC = 8
CAMPAIGN_SEED = 0xCA4D1400
CAMPAIGN_TEST, CAMPAIGN_EXEC = 5, 1      # (SrcDstFIFO: the same test, execution 2)


def campaign_gen():
    return ledger_gen(1)


def campaign_limits(strategy=T.STRATEGY_FULLY_RANDOM):
    return T.Limits(CAMPAIGN_MAX_MESSAGES, 1, 64, 0, 0, 0, strategy)


@functools.lru_cache(maxsize=None)
def campaign_test(i, seed_base=None):
    """(events array, areas array) of the campaign's test i"""
    seed_base = CAMPAIGN_SEED if seed_base is None else seed_base
    ev, ar = F.generate_fuzz_test_fields(CAMPAIGN_NUM_EVENTS, CAMPAIGN_WEIGHTS, campaign_gen(), CAMPAIGN_PREFIX, seed_base + i)
    return F.events_to_array(ev), np.array(ar, dtype=np.uint64)


def campaign_first_violation(max_tests, strategy=T.STRATEGY_FULLY_RANDOM, seed_base=None):
    """(test, execution) of the first violating test under the oracle with the tests' areas, or None"""
    from oracle import oracle_py as O
    O.build()
    try:
        for i in range(max_tests):
            ev, ar = campaign_test(i, seed_base)
            O.set_ext_areas(ar)
            v = O.random_explore(ledger_model(), ev, CAMPAIGN_EPC, seed_base=0, limits=campaign_limits(strategy))
            hit = np.nonzero(v["flags"] & T.V_VIOLATION)[0]
            if len(hit):
                return i, int(hit[0])
    finally:
        O.set_ext_areas(None)
    return None
