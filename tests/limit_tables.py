"""Tables at the limits include/demi_gpu.h declares, and seeds that force the retry loop of java.util.Random.nextInt(bound).
A helper module of tests/test_limits_cpu.py and tests/test_limits_gpu.py (TEST INFRASTRUCTURE; no fixture, no test).

limits_model(seed, layout): a random valid table with DEMI_MAX_MSG_TYPES (32) message types, DEMI_MAX_CLASSES (4) actor classes,
DEMI_MAX_TIMER_TYPES (4) timer types and 900 .. DEMI_MAX_CODE (1024) rows, for 8 actors (narrow, wide) or 16 (big).  The type
ids are laid out so that the code the smaller tables of the suites never reach is reached:
  timers     ids 5, 18, 27, 31 = timer indices 0..3 (two ids >= 16: the 64-bit `tix_packed` shift of K1; id 31: the top of
             the 5-bit type field); with actor 7 (15) receiving, timer (7, index 3) is bit 31 of the narrow timer mask and
             (15, index 3) bit 63 of the BIG one, and the timer directory runs with NTT = 4;
  externals  ids 0, 1, 20, 30;
  internals  the other 24 ids, 16 of them >= 10.
Handlers are tests/test_jit_cpu.py::_random_handler (few_effects) and its wide variant with the effect rows re-typed: SEND /
BCAST choose among all 24 internal types, TSET / TREP / TCANCEL among all four timer types (the helper itself only knows types
1, 2 and n_types - 1).  Some handlers start with hand-written rows so that the properties tests/test_limits_cpu.py asserts
on the oracle's executions do not hang on luck alone: the class of actor 7 (15) arms timer 31 on external 30 and cancels it on
external 20, every class arms one timer type on external 0, external 30 is broadcast as an internal type, and a third of
the internal handlers answer their sender (a hop count in P0 ends the exchange).

The invariant descriptors below were picked by looking at the ORACLE's final states of 4000 executions per table (never at a
kernel's): a field and a value that some, not most, executions end in.

seed_rejecting_draw / candidate_seeds / kept_seeds: seeds whose k-th scheduler draw takes nextInt's retry branch (below)."""
import numpy as np

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.fuzzer import events_to_array, kill, partition, send, start, unpartition, wait_quiescence

LAYOUTS = ("narrow", "wide", "big")
TIMER_TYPES = (5, 18, 27, 31)
EXTERNAL_TYPES = (0, 1, 20, 30)
INTERNAL_TYPES = tuple(t for t in range(T.MAX_MSG_TYPES) if t not in TIMER_TYPES and t not in EXTERNAL_TYPES)
MSGS = [("E%d" % t if t in EXTERNAL_TYPES else "Tm%d" % t if t in TIMER_TYPES else "I%d" % t,
         T.MSG_EXTERNAL if t in EXTERNAL_TYPES else T.MSG_TIMER if t in TIMER_TYPES else T.MSG_INTERNAL) for t in range(T.MAX_MSG_TYPES)]

# the table seed the suites use per layout, and (kind, fa, va, fb) per (seed, layout): see the module docstring (the oracle's
# violation rates under limits_of() and limits_trace(seed, model): 16 %, 7 %, 19 % of 4000 executions)
SEEDS = {"narrow": 2, "wide": 3, "big": 7}
INVARIANTS = {(2, "narrow"): (T.INV_NEVER, 7, 186, 0), (3, "wide"): (T.INV_NEVER, 5, 110, 0), (7, "big"): (T.INV_NEVER, 0, 29696, 0)}

_OP_SEND, _OP_BCAST, _OP_TSET, _OP_TREP, _OP_TCANCEL = (M.OPS[k] for k in ("SEND", "BCAST", "TSET", "TREP", "TCANCEL"))


def n_actors_of(layout):
    return T.MAX_ACTORS_BIG if layout == "big" else T.MAX_ACTORS


def limits_of(layout, n_events=0):
    """The Limits the suites run the limits tables under (max_messages, invariant interval, p_max)."""
    return T.Limits(300 if n_events <= 64 else 1000, 9, 128 if layout == "big" else 64, 0, 0, 0)


def _retype(asm, rng, internals=None, timers=None):
    """The effect rows of a handler of _random_handler with their message type drawn again: among ALL internal types for SEND /
    BCAST, among ALL timer types for TSET / TREP / TCANCEL (aux = bits 17..23 of the row word)."""
    for i, r in enumerate(asm.rows):
        op = r & 0xFF
        if op in (_OP_SEND, _OP_BCAST):
            ty = (internals or INTERNAL_TYPES)[int(rng.integers(len(internals or INTERNAL_TYPES)))]
        elif op in (_OP_TSET, _OP_TREP, _OP_TCANCEL):
            ty = (timers or TIMER_TYPES)[int(rng.integers(len(timers or TIMER_TYPES)))]
        else:
            continue
        asm.rows[i] = (r & ~(0x7F << 17)) | (ty << 17)
    return asm


def _prepend(asm, first):
    """The rows of `first` in front of the rows of `asm` (their label names are disjoint)."""
    k = len(first.rows)
    first.rows += asm.rows
    first._fix += [(i + k, lab) for i, lab in asm._fix]
    first._labels.update({name: v + k for name, v in asm._labels.items()})
    return first


def limits_model(seed, layout="narrow", invariant=None, n_actors=None, n_timer_types=4):
    from .test_jit_cpu import _random_handler, _random_handler_wide
    assert layout in LAYOUTS
    wide = layout != "narrow"
    A = n_actors or n_actors_of(layout)                      # (n_actors: a BIG table of 9 .. 15 actors, see tests/test_limits_gpu.py)
    assert A == n_actors_of(layout) or (layout == "big" and T.MAX_ACTORS < A <= T.MAX_ACTORS_BIG)
    NC, NT = T.MAX_CLASSES, T.MAX_MSG_TYPES
    # (n_timer_types = 3: id 27 is one more internal type - the timer directory and the timer masks with NTT = 3 < DEMI_MAX_TIMER_TYPES,
    # timer index 2 at id 31)
    assert n_timer_types in (3, 4)
    timers = TIMER_TYPES if n_timer_types == 4 else (5, 18, 31)
    internals = tuple(t for t in range(NT) if t not in timers and t not in EXTERNAL_TYPES)
    msgs = [(MSGS[t][0], T.MSG_TIMER if t in timers else T.MSG_EXTERNAL if t in EXTERNAL_TYPES else T.MSG_INTERNAL) for t in range(NT)]
    rng = np.random.default_rng([seed, LAYOUTS.index(layout), 0x11417])
    actor_class = [a % NC for a in range(A)]                 # every class used; actor 7 (and 15) is of class 3
    pairs = [(c, t) for c in range(NC) for t in range(NT)]
    skipped = {pairs[int(i)] for i in rng.choice(len(pairs), 3, replace=False)} - {(c, t) for c in range(NC) for t in (0, 20, 30)}
    keys = sorted(p for p in pairs if p not in skipped)
    want = int(rng.integers(950, 990))                       # rows in all: the budget below steers every handler's length by what is left
    hi = 65535 if wide else 255
    h, used = {}, 0
    for (c, t) in keys:
        left = len(keys) - len(h)
        n = max(2, min(14, round((want - used) / left) - 1 + int(rng.integers(-2, 3))))
        if wide and n >= 8:                                  # (the wide variant puts 2 .. 7 rows of 16-bit constants in front)
            a = _retype(_random_handler_wide(rng, n - 5, NT), rng, internals, timers)
        else:
            a = _retype(_random_handler(rng, n, NT, few_effects=True), rng, internals, timers)
        first = M.Asm()
        if t == 0:
            first.tset(timers[c % len(timers)])                       # every timer type armed by some class
        if t == 30 and c == actor_class[A - 1]:
            first.tset(timers[-1])                       # timer (A - 1, index 3): the top bit of the timer mask
        if t == 20 and c == actor_class[A - 1]:
            first.tcancel(timers[-1])
        if t == 30:                                          # traffic of the internal types: a broadcast per external 30 ...
            first.bcast(internals[int(rng.integers(len(internals)))], M.P0, M.P1)
        if t in internals and rng.integers(3) == 0:     # ... and replies to the sender that die out after at most three hops
            first.skipz(M.P0, "hop").sub(M.T3, M.P0, 1).and_(M.T3, M.T3, 3)
            first.send(internals[int(rng.integers(len(internals)))], M.SRC, M.T3, M.P1).label("hop")
        if t == 1:
            first.mov(M.F[7], hi & 0xFF)                     # the largest field value (wide: 65535)
            if wide:
                first.movhi(M.F[7], M.F[7], hi >> 8)
        h[(c, MSGS[t][0])] = a = _prepend(a, first) if first.rows else a
        used += len(a.rows) + 1
    init = [[int(x) for x in rng.integers(0, hi + 1, 8)] for _ in range(A)]
    init[A - 1][0] = hi
    inv = invariant if invariant is not None else INVARIANTS.get((seed, layout), (T.INV_NONE, 0, 0, 0))
    model = M.build_model("limits_%s_%d" % (layout, seed), A, msgs, h, init, inv, actor_class=actor_class, n_classes=NC, wide=wide)
    assert 900 <= len(model.code) <= T.MAX_CODE, len(model.code)
    return model


def limits_trace(seed, model, n_events=64, dpor=False):
    """Start of every actor, then Sends of the four external types (payloads up to the field width's maximum), some
    WaitQuiescence, a few Partition / UnPartition and at most one Kill; n_events in all (at most DEMI_MAX_EXT_EVENTS = 255).
    dpor: Start / Send / WaitQuiescence only (what DPORwHeuristics takes)."""
    A = model.n_actors
    assert A <= n_events <= T.MAX_EXT_EVENTS
    hi = 65535 if model.wide else 255
    rng = np.random.default_rng([seed, A, n_events, int(dpor), 0x7ACE])
    ev = [start(a) for a in range(A)]
    # the deliveries the properties of tests/test_limits_cpu.py look for: timer 31 of the last actor armed, then cancelled
    fixed = [send(A - 1, 30, hi, 0), send(A - 1, 20, 0, hi)] + [send(c, 0, c, hi) for c in range(T.MAX_CLASSES)] + [send(A - 1, 1, hi, hi)]
    if not dpor:                                             # (every kind of event in every trace, however the dice fall)
        fixed += [partition(0, 1), wait_quiescence(), unpartition(0, 1), kill(T.MAX_CLASSES)]
    ev += fixed[:max(0, n_events - len(ev))]
    parts, killed = [], [] if dpor else [T.MAX_CLASSES]                                   # (well-formed: what DDMin's atoms pair - a Kill after its actor's Start, an UnPartition with its Partition)
    while len(ev) < n_events:
        k = int(rng.integers(0, 40))
        a, b = int(rng.integers(A)), int(rng.integers(A))
        if k < 4 and ev[-1][0] != T.EV_WAIT_QUIESCENCE:
            ev.append(wait_quiescence())
        elif k == 4 and not dpor and a != b and (a, b) not in parts:
            parts.append((a, b))
            ev.append(partition(a, b))
        elif k == 5 and not dpor and parts:
            ev.append(unpartition(*parts.pop(int(rng.integers(len(parts))))))
        elif k == 6 and not dpor and T.MAX_CLASSES <= a < A - 1 and a not in killed and not killed:
            killed.append(a)
            ev.append(kill(a))
        else:
            p = [int(rng.integers(hi + 1)) if rng.integers(4) else hi for _ in range(2)]
            ev.append(send(a if rng.integers(4) else A - 1, EXTERNAL_TYPES[int(rng.integers(4))], p[0], p[1]))
    return events_to_array(ev)


# ----------------------------------------------------------------------------------------------------- crafted seeds
# java.util.Random.nextInt(bound) draws r = next(31) and, for a bound that is no power of two, rejects it when
# r - r % bound + bound - 1 overflows 31 bits: probability (2^31 mod bound) / 2^31, below 6e-8 for the schedulers' bounds, so
# random seeds never reach the retry (demi_device.hpp jr_next_int; DEMI_OP_RND's generator is always seeded 0 and cannot be
# steered).  But the state after the k-th step is chosen freely when the seed is: s_k = (r << 17) | low with r = 2^31 - 1 is
# rejected for EVERY such bound, the LCG s -> s * M + 0xB mod 2^48 is a bijection, and new Random(seed) starts at seed ^ M.
JR_MULT = 0x5DEECE66D
JR_MASK = (1 << 48) - 1
JR_MULT_INV = pow(JR_MULT, -1, 1 << 48)


def seed_rejecting_draw(k, low=0, r=(1 << 31) - 1):
    """The seed of a java.util.Random whose k-th next(31) (k = 1: the first) returns r (default: the largest value, which
    nextInt(bound) rejects for every bound that is no power of two)."""
    assert k >= 1 and 0 <= low < (1 << 17) and 0 <= r < (1 << 31)
    s = (r << 17) | low
    for _ in range(k):
        s = ((s - 0xB) * JR_MULT_INV) & JR_MASK
    return s ^ JR_MULT


def candidate_seeds(ks=(1, 2, 3, 5, 8, 13, 21, 34), per_k=48):
    """Seeds whose k-th generator step is a rejected draw, for each k of `ks` (whether an execution reaches its k-th step at a
    bound that is no power of two is the execution's business: kept_seeds keeps those that do)."""
    return [seed_rejecting_draw(k, (low * 2654435761 + k) & 0x1FFFF) for k in ks for low in range(per_k)]


def _counting_random(seed, counts, site):
    """A java.util.Random (demi_amd.fuzzer.JavaRandom, the transliterations' generator) that counts in counts[site[0]] every
    draw nextInt(bound) rejects - the retry branch - at a bound that is no power of two."""
    from demi_amd.fuzzer import JavaRandom

    class Counting(JavaRandom):
        def next_int(self, bound=None):
            if bound is None or bound & (bound - 1) == 0:
                return JavaRandom.next_int(self, bound)
            u = self.next(31)
            while ((u - u % bound + bound - 1) & 0xFFFFFFFF) >= (1 << 31):
                counts[site[0]] = counts.get(site[0], 0) + 1
                u = self.next(31)
            return u % bound
    return Counting(seed)


def fully_random_execution(oracle, model, events, seed, lim):
    """One execution by the literal transliteration of RandomScheduler + FullyRandom (tests/test_random_scheduler_transliteration_cpu.py)
    under a counting generator -> (the scheduler after execute(), {"rng": rejected draws})."""
    from .test_random_scheduler_transliteration_cpu import ScalaRandomScheduler
    counts = {}
    s = ScalaRandomScheduler(oracle, model, events, seed, lim.max_messages, lim.invariant_check_interval)
    s.pendingEvents.pendingEvents.rand = _counting_random(seed, counts, ["rng"])
    s.execute()
    return s, counts


class ScalaSrcDstFIFO:
    """SrcDstFIFO (RandomScheduler.scala:702-909) as the pending-message container of the transliterated RandomScheduler, for
    executions in which no actor is blocked (tables without CRASH rows): += (:786-804), getNonBlockedMessage (:716-760, what
    RandomScheduler asks it through), dequeue (:762-772), remove (:858-: a cancelled timer leaves timersAndExternals, a
    FullyRandom of its own).  The reference seeds both generators with the clock; the restatement with the execution's seed.
    An element is (snd, rcv, msg, uniq id); counts: rejected draws per call site ("rng" = rand.nextInt(allMessages.size),
    "pair" = rand.nextInt(srcDsts.size), "te_rng" = timersAndExternals' generator)."""

    def __init__(self, seed):
        from .test_random_scheduler_transliteration_cpu import FullyRandom
        self.counts, self._site = {}, ["rng"]
        self.srcDsts, self.srcDstToMessages = [], {}
        self.rand = _counting_random(seed, self.counts, self._site)
        self.timersAndExternals = FullyRandom(seed)
        self.timersAndExternals.pendingEvents.rand = _counting_random(seed, self.counts, ["te_rng"])

    def _te(self):
        return self.timersAndExternals.pendingEvents.arr

    def size(self):                                   # allMessages.size
        return len(self._te()) + sum(len(q) for q in self.srcDstToMessages.values())

    def isEmpty(self):
        return self.size() == 0

    def add(self, e):
        if e[0] == "deadLetters":
            self.timersAndExternals.add(e)
            return
        key = (e[0], e[1])
        if key not in self.srcDstToMessages:
            self.srcDsts.append(key)
            self.srcDstToMessages[key] = []
        self.srcDstToMessages[key].append(e)

    insert = add

    def remove(self, snd, rcv, msg):
        assert snd == "deadLetters"                   # (RandomScheduler only cancels timers)
        return self.timersAndExternals.remove(snd, rcv, msg)

    def removeRandomElement(self):
        """getNonBlockedMessage(blockedActors = {})"""
        if not self.srcDstToMessages:
            return self.timersAndExternals.removeRandomElement()
        self._site[0] = "rng"
        if self.rand.next_int(self.size()) < len(self._te()):
            return self.timersAndExternals.removeRandomElement()
        self._site[0] = "pair"
        idx = self.rand.next_int(len(self.srcDsts))
        key = self.srcDsts[idx]
        q = self.srcDstToMessages[key]
        ret = q.pop(0)
        if not q:
            del self.srcDstToMessages[key]
            del self.srcDsts[idx]
        return ret


def srcdst_fifo_execution(oracle, model, events, seed, lim):
    """One execution by the transliterated RandomScheduler over ScalaSrcDstFIFO -> (the scheduler, rejected draws per site)."""
    from .test_random_scheduler_transliteration_cpu import ScalaRandomScheduler
    assert not any((r & 0xFF) == M.OPS["CRASH"] for r in model.code), "ScalaSrcDstFIFO: no blocked actors"
    c = ScalaSrcDstFIFO(seed)
    s = ScalaRandomScheduler(oracle, model, events, seed, lim.max_messages, lim.invariant_check_interval, strategy=c)
    s.execute()
    return s, c.counts


def kept_seeds(oracle, model, events, lim, strategy, candidates=None):
    """The candidate seeds whose execution really takes nextInt's retry branch at a bound that is no power of two, by the
    TRANSLITERATIONS' count (never a kernel's), and the rejections per call site over all of them.  Executions the oracle
    aborts on one of its capacities are left out (they are no behaviour of the reference)."""
    l = T.Limits(lim.max_messages, lim.invariant_check_interval, lim.p_max, 0, 0, 0, strategy)
    kept, sites = [], {}
    for seed in (candidate_seeds() if candidates is None else candidates):
        v, rec, _ = oracle.random_execute(model, events, seed, l)
        if v.flags & (T.V_PENDING_OVF | T.V_QUEUE_OVF):
            continue
        s, counts = (srcdst_fifo_execution if strategy == T.STRATEGY_SRC_DST_FIFO else fully_random_execution)(oracle, model, events, seed, l)
        got = [(int(e["snd"]), int(e["rcv"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"])) for e in rec if e["kind"] == T.REC_MSG_EVENT]
        assert got == s.deliveries and (int(v.flags), int(v.fingerprint), int(v.hash)) == s.verdict(), "seed %d: the oracle is not the transliteration" % seed
        if sum(counts.values()):
            kept.append(seed)
            for k, c in counts.items():
                sites[k] = sites.get(k, 0) + c
    return kept, sites


# ----------------------------------------------------------------------------------------------------- one step beyond
def beyond_the_limits():
    """(mutation of a limits table, the words the refusal must contain): 33 message types, 5 classes, 1025 rows, 5 timer types."""
    def types33(m):
        nt = m.n_msg_types
        m.handler_start = [x for c in range(m.n_classes) for x in m.handler_start[c * nt:(c + 1) * nt] + [0xFFFF]]
        m.msg_names, m.msg_class = m.msg_names + ["I32"], m.msg_class + [T.MSG_INTERNAL]
        return m

    def classes5(m):
        m.n_classes, m.handler_start = m.n_classes + 1, m.handler_start + [0xFFFF] * m.n_msg_types
        return m

    def rows1025(m):
        m.code = m.code + [M.row(M.OPS["HALT"])] * (T.MAX_CODE + 1 - len(m.code))
        return m

    def timers5(m):
        m.msg_class = list(m.msg_class)
        m.msg_class[INTERNAL_TYPES[0]] = T.MSG_TIMER
        return m

    return [(types33, "n_msg_types"), (classes5, "n_classes"), (rows1025, "code_len"), (timers5, "timer types")]
