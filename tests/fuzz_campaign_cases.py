"""Shared inputs of the fuzz-campaign suites (tests/test_fuzz_campaign_*.py): the Fuzzer configurations whose seed sets the
GPU tests generate on the device, the host mirror's tests for them (computed once per process) and the conditions those seed
sets must contain - asserted on the mirror alone in tests/test_fuzz_campaign_cpu.py, so that a GPU comparison that passes has
compared the paths it claims to."""
import functools

from demi_amd import fuzzer as F, types as T
from demi_amd.model import M_BOOTSTRAP, M_CLIENT

N_TESTS = 300            # not a multiple of 64: the generator's last wave is partial
SEED_BASE = 0xF0220000


def raft_prefix(n_actors):
    return [F.start(a) for a in range(n_actors)] + [F.send(a, M_BOOTSTRAP) for a in range(n_actors)]


def raft_gen():
    return F.raft_send_generator()


def mixed_gen():
    """every target and field kind, more than one alternative (the alternative's own draw)"""
    return F.SendGenerator([(M_CLIENT, F.RANDOM_ALIVE, F.COUNTER, F.CONST(0)),
                            (M_CLIENT, F.FIXED(1), F.RANDOM(7), F.RANDOM(256)),
                            (M_BOOTSTRAP, F.RANDOM_ALIVE, F.CONST(0), F.CONST(0))])


class Config:
    def __init__(self, name, n_actors, num_events, weights, gen=raft_gen, postfix=()):
        self.name, self.n_actors, self.num_events, self.weights, self.gen_ctor = name, n_actors, num_events, weights, gen
        self.prefix, self.postfix = raft_prefix(n_actors), list(postfix)

    @property
    def stride(self):
        return F.fuzz_stride(self.num_events, self.prefix, self.postfix)

    def gen(self):
        return self.gen_ctor()


# kill weight raised, 3 actors: tests that end early because every node was killed
KILLS = Config("kills", 3, 24, F.FuzzerWeights(kill=0.15, send=0.3, wait_quiescence=0.1, partition=0.1, unpartition=0.1))
# 2 actors = one pair, no WaitQuiescence: every extra double is the retry on an empty partition / unpartition set
ONE_PAIR = Config("one_pair", 2, 24, F.FuzzerWeights(kill=0.0, send=0.2, wait_quiescence=0.0, partition=0.4, unpartition=0.4), gen=mixed_gen)
# no partitions: every extra double is the retry after two WaitQuiescence in a row
WAITS = Config("waits", 3, 24, F.FuzzerWeights(kill=0.0, send=0.4, wait_quiescence=0.6, partition=0.0, unpartition=0.0),
               postfix=[F.send(0, M_CLIENT, 9, 0)])
# config 2's shape: default weights, 5 actors, 50 events
RAFT5 = Config("raft5", 5, 40, F.FuzzerWeights(), gen=mixed_gen)
# nothing generated: the prefix and the final WaitQuiescence alone
PREFIX_ONLY = Config("prefix_only", 3, 0, F.FuzzerWeights())
# the largest test the boundary takes: stride exactly DEMI_MAX_EXT_EVENTS
STRIDE_255 = Config("stride_255", 5, T.MAX_EXT_EVENTS - 10 - 1, F.FuzzerWeights(kill=0.001))
STRIDE_256 = Config("stride_256", 5, T.MAX_EXT_EVENTS - 10, F.FuzzerWeights(kill=0.001))      # refused
CONFIGS = [KILLS, ONE_PAIR, WAITS, RAFT5, PREFIX_ONLY, STRIDE_255]


def explicit_seeds(n=N_TESTS):
    """seeds that are no arithmetic progression (the `seeds` form of the entry point)"""
    return [(0x9E3779B97F4A7C15 * (i + 1) ^ (i << 40)) & ((1 << 64) - 1) for i in range(n)]


class _Counting(F.JavaRandom):
    """counts nextDouble calls and the draws nextInt rejects"""

    def __init__(self, seed):
        super().__init__(seed)
        self.doubles, self.rejected = 0, 0

    def next_double(self):
        self.doubles += 1
        return super().next_double()

    def next_int(self, bound=None):
        if bound is None or bound & (bound - 1) == 0:
            return super().next_int(bound)
        u = self.next(31)
        while ((u - u % bound + bound - 1) & 0xFFFFFFFF) >= (1 << 31):
            self.rejected += 1
            u = self.next(31)
        return u % bound


def mirror_test(cfg, seed, counting=False):
    """the host mirror's test; counting: (events, nextDouble calls, rejected nextInt draws)"""
    if not counting:
        return F.generate_fuzz_test(cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed, cfg.postfix)
    made = []
    orig = F.JavaRandom

    def ctor(s):
        made.append(_Counting(s))
        return made[-1]
    F.JavaRandom = ctor
    try:
        ev = F.generate_fuzz_test(cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed, cfg.postfix)
    finally:
        F.JavaRandom = orig
    return ev, made[0].doubles, made[0].rejected


@functools.lru_cache(maxsize=None)
def mirror_tests(name, explicit=False, n=N_TESTS):
    """the mirror's n tests of configuration `name`, under SEED_BASE + i or explicit_seeds()[i]: a tuple of event lists"""
    cfg = {c.name: c for c in CONFIGS}[name]
    seeds = explicit_seeds(n) if explicit else [SEED_BASE + i for i in range(n)]
    return tuple(tuple(mirror_test(cfg, s)) for s in seeds)


def n_batches(events):
    return 1 + sum(1 for e in events if e[0] == T.EV_WAIT_QUIESCENCE)


# ---- K1 with a workgroup per test: 37 tests over config 2's table (5 raft nodes), lengths from 11 to 51 events
K1_KILLS5 = Config("k1_kills5", 5, 40, F.FuzzerWeights(kill=0.12, send=0.3, wait_quiescence=0.1, partition=0.1, unpartition=0.1))
K1_PREFIX5 = Config("k1_prefix5", 5, 0, F.FuzzerWeights())
K1_SEED_BASE = 0x5EED8000      # (chosen with the oracle: at ONE execution per test a violating test exists under both strategies)


@functools.lru_cache(maxsize=None)
def k1_tests(n=37):
    """event arrays: the prefix alone, tests that end early at differing lengths, full-length tests of config 2's shape"""
    ev = [mirror_test(K1_PREFIX5, 1)]
    ev += [mirror_test(K1_KILLS5, SEED_BASE + i) for i in range((n - 1) // 2)]
    ev += list(mirror_tests("raft5"))[:n - len(ev)]
    return tuple(F.events_to_array(list(e)) for e in ev)


def k1_limits(strategy=T.STRATEGY_FULLY_RANDOM, p_max=64):
    return T.Limits(200, 30, p_max, 0, 0, 0, strategy)


@functools.lru_cache(maxsize=None)
def k1_oracle(strategy, epc, p_max=64, n=37):
    """the CPU oracle's verdicts per test: trace_load(test i) + random_explore(K1_SEED_BASE + k), computed once"""
    from demi_amd.model import raft_model
    from oracle import oracle_py as O
    O.build()
    model = raft_model(5)
    return tuple(O.random_explore(model, ev, epc, seed_base=K1_SEED_BASE, limits=k1_limits(strategy, p_max)) for ev in k1_tests(n))
