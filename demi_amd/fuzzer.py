"""External-event trace generation with the distribution of DEMi's Fuzzer.

Follows src/main/scala/verification/fuzzing/Fuzzer.scala (weights :24-29, event choice :44-57,
generateNextEvent :83-120, generateFuzzTest :122-175).  The reference reseeds from the wall clock
on every call (:67-68, :177-179), so its traces are not reproducible; here one seeded
java.util.Random drives every choice and the generated traces are frozen as golden files.
Trace generation is off the hot path.
"""
from dataclasses import dataclass
from typing import Callable, List, Tuple

import numpy as np

from . import types as T

_MULT = 0x5DEECE66D
_MASK = (1 << 48) - 1


class JavaRandom:
    """java.util.Random (JDK javadoc LCG)."""

    def __init__(self, seed: int):
        self.s = (seed ^ _MULT) & _MASK

    def next(self, bits: int) -> int:
        self.s = (self.s * _MULT + 0xB) & _MASK
        v = self.s >> (48 - bits)
        if v >= 1 << 31:
            v -= 1 << 32
        return v

    def next_int(self, bound: int = None) -> int:
        if bound is None:
            return self.next(32)
        r = self.next(31)
        m = bound - 1
        if bound & m == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            t = (u - r + m) & 0xFFFFFFFF
            if t < (1 << 31):
                return r
            u = self.next(31)

    def next_double(self) -> float:
        return ((self.next(26) << 27) + self.next(27)) * (1.0 / (1 << 53))


@dataclass
class FuzzerWeights:          # Fuzzer.scala:24-29
    kill: float = 0.01
    send: float = 0.3
    wait_quiescence: float = 0.1
    partition: float = 0.1
    unpartition: float = 0.1


Event = Tuple[int, int, int, int, int, int]   # kind, a, b, msg_type, p0, p1


def start(a):
    return (T.EV_START, a, 0, 0, 0, 0)


def kill(a):
    return (T.EV_KILL, a, 0, 0, 0, 0)


def send(a, msg_type, p0=0, p1=0):
    return (T.EV_SEND, a, 0, msg_type, p0, p1)


def partition(a, b):
    return (T.EV_PARTITION, a, b, 0, 0, 0)


def unpartition(a, b):
    return (T.EV_UNPARTITION, a, b, 0, 0, 0)


def wait_quiescence():
    return (T.EV_WAIT_QUIESCENCE, 0, 0, 0, 0, 0)


def events_to_array(events: List[Event]) -> np.ndarray:
    arr = np.zeros(len(events), dtype=T.EXT_EVENT_DTYPE)
    for i, e in enumerate(events):
        kind, a, b, msg_type, p0, p1 = e
        arr[i]["kind"], arr[i]["a"], arr[i]["b"], arr[i]["msg_type"] = kind, a, b, msg_type
        arr[i]["p0"], arr[i]["p1"] = p0 & 0xFF, p1 & 0xFF
        arr[i]["p0_hi"], arr[i]["p1_hi"] = p0 >> 8, p1 >> 8          # 16-bit payloads: wide models only
    return arr


def array_to_events(arr: np.ndarray) -> List[Event]:
    return [(int(e["kind"]), int(e["a"]), int(e["b"]), int(e["msg_type"]), int(e["p0"]) | (int(e["p0_hi"]) << 8),
             int(e["p1"]) | (int(e["p1_hi"]) << 8)) for e in arr]


class _RandSet:
    """RandomizedHashSet (schedulers/Util.scala:110-185) driven by the shared RNG."""

    def __init__(self, rng):
        self.arr, self.rng = [], rng

    def insert(self, v):
        self.arr.append(v)

    def remove_random(self):
        i = self.rng.next_int(len(self.arr))
        v = self.arr[i]
        self.arr[i] = self.arr[-1]
        self.arr.pop()
        return v

    def get_random(self):
        return self.arr[self.rng.next_int(len(self.arr))]

    def __len__(self):
        return len(self.arr)


def generate_fuzz_test(num_events: int, weights: FuzzerWeights, message_gen: Callable, prefix: List[Event],
                       seed: int, postfix: List[Event] = ()) -> List[Event]:
    """Fuzzer.generateFuzzTest (Fuzzer.scala:122-175).  message_gen(rng, alive_set) -> Send event."""
    rng = JavaRandom(seed)
    nodes = [e[1] for e in prefix if e[0] == T.EV_START]
    alive = _RandSet(rng)
    for n in nodes:
        alive.insert(n)
    parted, unparted = _RandSet(rng), _RandSet(rng)
    for i in range(len(nodes)):
        for j in range(i + 1, len(nodes)):
            unparted.insert((nodes[i], nodes[j]))
    weights_list = [weights.kill, weights.send, weights.partition, weights.unpartition]
    total = sum(weights_list) + weights.wait_quiescence

    def next_event():
        while True:
            scaled = rng.next_double() * total
            cur, cls = 0.0, None
            for idx, w in enumerate(weights_list):
                cur += w
                if scaled < cur:
                    cls = idx
                    break
            if cls is None:
                return wait_quiescence()
            if cls == 0:
                if len(alive) == 0:
                    return None
                return kill(alive.remove_random())
            if cls == 1:
                return message_gen(rng, alive)
            if cls == 2:
                if len(unparted) == 0:
                    continue
                pair = unparted.remove_random()
                parted.insert(pair)
                return partition(*pair)
            if len(parted) == 0:
                continue
            pair = parted.remove_random()
            unparted.insert(pair)
            return unpartition(*pair)

    out = list(prefix)
    just_wq = bool(out) and out[-1][0] == T.EV_WAIT_QUIESCENCE
    for _ in range(num_events):
        ev = next_event()
        while ev is not None and ev[0] == T.EV_WAIT_QUIESCENCE and just_wq:
            ev = next_event()
        if ev is None:
            return out
        just_wq = ev[0] == T.EV_WAIT_QUIESCENCE
        out.append(ev)
    out.extend(postfix)
    if out and out[-1][0] != T.EV_WAIT_QUIESCENCE:
        out.append(wait_quiescence())
    return out


def raft_trace(n_actors: int, n_events: int, seed: int, weights: FuzzerWeights = None, exact: bool = True) -> List[Event]:
    """Start x A, Bootstrap x A, then Fuzzer-distributed events; exactly n_events long (exact=False: at
    most n_events + 1; the Fuzzer stops early once every node is killed)."""
    from .model import M_BOOTSTRAP, M_CLIENT
    weights = weights or FuzzerWeights()
    prefix = [start(a) for a in range(n_actors)] + [send(a, M_BOOTSTRAP) for a in range(n_actors)]
    counter = [0]

    def gen(rng, alive):
        counter[0] += 1
        target = alive.get_random() if len(alive) else 0
        return send(target, M_CLIENT, counter[0] & 0xFF, 0)

    if not exact:
        return generate_fuzz_test(n_events - len(prefix), weights, gen, prefix, seed)
    # the Fuzzer appends a final WaitQuiescence only when the last event is not one, so a given seed
    # may not hit the requested length exactly: retry with a derived seed (deterministic)
    for attempt in range(64):
        for k in (n_events - len(prefix), n_events - len(prefix) - 1):
            counter[0] = 0
            tr = generate_fuzz_test(k, weights, gen, prefix, seed + attempt * 0x9E3779B9)
            if len(tr) == n_events:
                return tr
    raise ValueError("cannot build a trace of exactly %d events" % n_events)


# ---------------------------------------------------------------------------------------------------------------------
# A message generator that can cross the C ABI (include/demi_gpu.h demi_fuzz_send_gen).  Fuzzer takes the application's
# MessageGenerator closure (Fuzzer.scala:31-35); k_fuzz_generate (csrc/k_fuzz.hpp) cannot call one, so the usual closures
# are restated as data: 1..8 alternatives (msg_type, target, p0, p1).  The draw order is the contract between this mirror
# and the kernel: the alternative with next_int(n) only when n > 1, then the target, then p0, then p1.
FUZZ_MAX_ALTS = 8
TARGET_RANDOM_ALIVE, TARGET_FIXED = 0, 1
FIELD_CONST, FIELD_COUNTER, FIELD_RANDOM = 0, 1, 2

RANDOM_ALIVE = (TARGET_RANDOM_ALIVE, 0)
COUNTER = (FIELD_COUNTER, 0)


def FIXED(actor):
    return (TARGET_FIXED, int(actor))


def CONST(v):
    return (FIELD_CONST, int(v))


def RANDOM(bound):
    return (FIELD_RANDOM, int(bound))


SEND_ALT_DTYPE = np.dtype([("msg_type", "u1"), ("target_kind", "u1"), ("target_actor", "u1"), ("p0_kind", "u1"),
                           ("p1_kind", "u1"), ("pad", "u1", (3,)), ("p0_arg", "<u4"), ("p1_arg", "<u4")])     # demi_fuzz_send_alt
SEND_GEN_DTYPE = np.dtype([("n_alts", "<u4"), ("field_bits", "<u4"), ("alts", SEND_ALT_DTYPE, (FUZZ_MAX_ALTS,))])  # demi_fuzz_send_gen


class SendGenerator:
    """alternatives: [(msg_type, target, p0, p1)] with target RANDOM_ALIVE / FIXED(actor) and p0, p1 each CONST(v) /
    COUNTER / RANDOM(bound).  COUNTER = the Sends generated so far in this test, starting at 1, masked to the field's
    width (field_bits: 8, or 16 for a DEMI_MODEL_WIDE table).  Callable as generate_fuzz_test's message_gen; the counter
    restarts whenever it is handed a generator it has not seen, i.e. with every generate_fuzz_test."""

    def __init__(self, alternatives, field_bits: int = 8):
        alternatives = [tuple(a) for a in alternatives]
        if not 1 <= len(alternatives) <= FUZZ_MAX_ALTS:
            raise ValueError("a SendGenerator holds 1..%d alternatives" % FUZZ_MAX_ALTS)
        if field_bits not in (8, 16):
            raise ValueError("field_bits is 8, or 16 for a wide table")
        lim = 1 << field_bits
        for msg_type, target, p0, p1 in alternatives:
            if not 0 <= msg_type < 32:
                raise ValueError("message type %r" % (msg_type,))
            if target[0] not in (TARGET_RANDOM_ALIVE, TARGET_FIXED) or not 0 <= target[1] < 16:
                raise ValueError("target %r" % (target,))
            for kind, arg in (p0, p1):
                if kind == FIELD_CONST and not 0 <= arg < lim:
                    raise ValueError("CONST(%d) does not fit %d bits" % (arg, field_bits))
                if kind == FIELD_RANDOM and not 1 <= arg <= min(lim, 256):
                    raise ValueError("RANDOM(%d): the bound is 1..%d" % (arg, min(lim, 256)))
                if kind not in (FIELD_CONST, FIELD_COUNTER, FIELD_RANDOM):
                    raise ValueError("payload field %r" % ((kind, arg),))
        self.alternatives, self.field_bits = alternatives, field_bits
        self._rng, self.counter = None, 0

    def __call__(self, rng, alive):
        if rng is not self._rng:
            self._rng, self.counter = rng, 0
        self.counter += 1
        alts = self.alternatives
        msg_type, target, p0, p1 = alts[rng.next_int(len(alts))] if len(alts) > 1 else alts[0]
        if target[0] == TARGET_RANDOM_ALIVE:
            a = alive.get_random() if len(alive) else 0
        else:
            a = target[1]
        mask = (1 << self.field_bits) - 1

        def field(f):
            if f[0] == FIELD_CONST:
                return f[1]
            if f[0] == FIELD_COUNTER:
                return self.counter & mask
            return rng.next_int(f[1])

        v0 = field(p0)
        v1 = field(p1)
        return send(a, msg_type, v0, v1)

    def to_struct(self) -> np.ndarray:
        s = np.zeros(1, dtype=SEND_GEN_DTYPE)
        s["n_alts"], s["field_bits"] = len(self.alternatives), self.field_bits
        for i, (msg_type, target, p0, p1) in enumerate(self.alternatives):
            a = s["alts"][0][i]
            a["msg_type"], a["target_kind"], a["target_actor"] = msg_type, target[0], target[1]
            a["p0_kind"], a["p0_arg"], a["p1_kind"], a["p1_arg"] = p0[0], p0[1], p1[0], p1[1]
        return s


# The same for messages with more than two fields (include/demi_gpu.h demi_fuzz_field_gen, k_fuzz_generate_fields): an alternative
# is (msg_type, target, [field, ..]) with up to six fields.  The draw order: the alternative with next_int(n) only when n > 1, the
# target, then the fields 0, 1, .. in that order - with two fields each, SendGenerator's.  The field width is the table's.
MAX_PAYLOADS = 6
FIELD_ALT_DTYPE = np.dtype([("msg_type", "u1"), ("target_kind", "u1"), ("target_actor", "u1"), ("n_fields", "u1"),
                            ("kind", "u1", (MAX_PAYLOADS,)), ("pad", "u1", (2,)), ("arg", "<u4", (MAX_PAYLOADS,))])     # demi_fuzz_field_alt
FIELD_GEN_DTYPE = np.dtype([("n_alts", "<u4"), ("pad", "<u4"), ("alts", FIELD_ALT_DTYPE, (FUZZ_MAX_ALTS,))])          # demi_fuzz_field_gen


def model_field_layout(model):
    """(fields per message, field width W) of a table, as the library derives them: 2 fields of 8 bits for a narrow table, of 16
    for a wide one; DEMI_MODEL_PAYLOADS(n): n fields of DEMI_PAYLOAD_BITS(n) = 16, 12, 9, 8 bits."""
    npay = int(getattr(model, "payloads", 0) or 0)
    if npay > 2:
        return npay, T.payload_bits(npay)
    return 2, 16 if getattr(model, "wide", False) else 8


class FieldSendGenerator:
    """alternatives: [(msg_type, target, [field, ..])] with target RANDOM_ALIVE / FIXED(actor) and up to as many fields as a
    message of `model` has, each CONST(v) / COUNTER / RANDOM(bound); the fields an alternative leaves out are 0.  COUNTER = the
    Sends generated so far in this test, starting at 1, masked to the field width.  Callable as generate_fuzz_test's
    message_gen: the Send it returns carries P0 / P1 = fields 0 / 1, and `sent` remembers every generated Send's field list
    (one list per Send of the current test, in order) - generate_fuzz_test_fields makes the payload areas of them."""

    def __init__(self, alternatives, model):
        self.n_payloads, self.field_bits = model_field_layout(model)
        self.with_areas = int(getattr(model, "payloads", 0) or 0) > 2
        alternatives = [(a[0], tuple(a[1]), [tuple(f) for f in a[2]]) for a in alternatives]
        if not 1 <= len(alternatives) <= FUZZ_MAX_ALTS:
            raise ValueError("a FieldSendGenerator holds 1..%d alternatives" % FUZZ_MAX_ALTS)
        lim = 1 << self.field_bits
        for msg_type, target, fields in alternatives:
            if not 0 <= msg_type < 32:
                raise ValueError("message type %r" % (msg_type,))
            if target[0] not in (TARGET_RANDOM_ALIVE, TARGET_FIXED) or not 0 <= target[1] < 16:
                raise ValueError("target %r" % (target,))
            if len(fields) > self.n_payloads:
                raise ValueError("%d fields described, a message of the table has %d" % (len(fields), self.n_payloads))
            for kind, arg in fields:
                if kind not in (FIELD_CONST, FIELD_COUNTER, FIELD_RANDOM):
                    raise ValueError("unknown field kind %r" % ((kind, arg),))
                if kind == FIELD_CONST and not 0 <= arg < lim:
                    raise ValueError("CONST(%d) does not fit %d bits" % (arg, self.field_bits))
                if kind == FIELD_RANDOM and not 1 <= arg <= min(lim, 256):
                    raise ValueError("RANDOM(%d): the bound is 1..%d" % (arg, min(lim, 256)))
        self.alternatives = alternatives
        self._rng, self.counter, self.sent, self._sent_events = None, 0, [], []

    def __call__(self, rng, alive):
        if rng is not self._rng:
            self._rng, self.counter, self.sent, self._sent_events = rng, 0, [], []
        self.counter += 1
        alts = self.alternatives
        msg_type, target, fields = alts[rng.next_int(len(alts))] if len(alts) > 1 else alts[0]
        if target[0] == TARGET_RANDOM_ALIVE:
            a = alive.get_random() if len(alive) else 0
        else:
            a = target[1]
        mask = (1 << self.field_bits) - 1
        vals = []
        for kind, arg in fields:
            vals.append(arg if kind == FIELD_CONST else self.counter & mask if kind == FIELD_COUNTER else rng.next_int(arg))
        ev = send(a, msg_type, vals[0] if len(vals) > 0 else 0, vals[1] if len(vals) > 1 else 0)
        self.sent.append(vals)
        self._sent_events.append(ev)
        return ev

    def area(self, vals) -> int:
        """the payload area of a Send with these fields: 0 for a table without DEMI_MODEL_PAYLOADS"""
        return T.pay_area(vals, self.n_payloads) if self.with_areas else 0

    def to_struct(self) -> np.ndarray:
        s = np.zeros(1, dtype=FIELD_GEN_DTYPE)
        s["n_alts"] = len(self.alternatives)
        for i, (msg_type, target, fields) in enumerate(self.alternatives):
            a = s["alts"][0][i]
            a["msg_type"], a["target_kind"], a["target_actor"], a["n_fields"] = msg_type, target[0], target[1], len(fields)
            for k, (kind, arg) in enumerate(fields):
                a["kind"][k], a["arg"][k] = kind, arg
        return s


def generate_fuzz_test_fields(num_events: int, weights: FuzzerWeights, field_gen: FieldSendGenerator, prefix: List[Event],
                              seed: int, postfix: List[Event] = ()):
    """generate_fuzz_test with a FieldSendGenerator: (events, areas), areas[i] the 48-bit payload area of event i - of a
    generated Send its fields packed by T.pay_area, of a Send of the prefix / postfix what trace_load makes of P0 / P1 with
    nothing staged, 0 for every other event and for a table without DEMI_MODEL_PAYLOADS.  The mirror of
    k_fuzz_generate_fields, byte for byte."""
    field_gen._rng = None                       # (this test's count starts at 1, whatever the generator object generated before)
    field_gen.sent, field_gen._sent_events = [], []
    events = generate_fuzz_test(num_events, weights, field_gen, prefix, seed, postfix)
    # (a generated Send is the very tuple the generator returned; a Send of the prefix / postfix is not)
    made = {id(e): vals for e, vals in zip(field_gen._sent_events, field_gen.sent)}
    areas = [0 if e[0] != T.EV_SEND else field_gen.area(made[id(e)] if id(e) in made else [e[4], e[5]]) for e in events]
    return events, areas


def raft_send_generator() -> SendGenerator:
    """raft_trace's closure as a descriptor: ClientRequest(counter) to a random live node."""
    from .model import M_CLIENT
    return SendGenerator([(M_CLIENT, RANDOM_ALIVE, COUNTER, CONST(0))])


def fuzz_stride(num_events: int, prefix, postfix=()) -> int:
    """The longest test generate_fuzz_test(num_events, ..) can return: prefix + num_events + postfix + the final WaitQuiescence."""
    return len(prefix) + num_events + len(postfix) + 1


def fuzz_thresholds(weights: FuzzerWeights):
    """(totalMass, cumulative kill, send, partition, unpartition), each computed by the very expressions of
    generate_fuzz_test: the doubles the device multiplies by and compares against."""
    weights_list = [weights.kill, weights.send, weights.partition, weights.unpartition]
    total = sum(weights_list) + weights.wait_quiescence
    cur, cum = 0.0, []
    for w in weights_list:
        cur += w
        cum.append(cur)
    return (total, *cum)
