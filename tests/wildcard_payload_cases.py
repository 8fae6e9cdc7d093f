"""Helper (no tests live here): the transliterated wildcard STSScheduler, clusterizers, WildcardMinimizer and WildcardTestOracle of
tests/test_wildcard_transliteration_cpu.py / tests/test_wildcard_ddmin_cpu.py for tables whose messages carry MORE THAN TWO FIELDS
(DEMI_MODEL_PAYLOADS) and for DEMI_MODEL_ARRAY tables, the workloads the wildcard kernels are held against on such tables, and the
ledger workload of the DPOR-with-areas tests.

The base transliteration writes a message as (type, p0, p1) and ScalaRandomScheduler asserts payloads == 2.  Here a message is
(type, area): `area` is the message's whole payload as demi_rec_event stores it (p0 | p1 << 16 | p_hi << 32).  The sender and the
receiver stay where the reference keeps them - the keys of pendingEvents and the arguments of tell - so a message's identity as the
scheduler compares it is (type, snd, rcv, area).  Delivery goes through orc_vm_run_area; what is recorded as p0 / p1 / p_hi comes
from the area.  Everything else - pendingEvents, the selectors, the clusterizers' iterators - is the base classes' code."""
import ctypes as C
from collections import OrderedDict

import numpy as np

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.apps import raft5_config2
from demi_amd.fuzzer import events_to_array, send, start, wait_quiescence
from demi_amd.minification import DDMin, EventDagView, UnmodifiedEventDag
from demi_amd.schedulers import EventTrace, MinimizationStats, ViolationFingerprint

from . import test_wildcard_transliteration_cpu as X
from .test_internal_min_cpu import _verified_mcs
from .test_minification_cpu import _violating_execution
from .test_random_scheduler_transliteration_cpu import DEAD, MASK64, _Effect

P_MAX = 128


def area_of(e):
    return int(e["p0"]) | int(e["p1"]) << 16 | int(e["p_hi"]) << 32


def _split(area):
    return area & 0xFFFF, (area >> 16) & 0xFFFF, (area >> 32) & 0xFFFF


class _TwoFieldView:
    """The model as ScalaRandomScheduler's constructor wants to see it (it asserts messages of two fields, because ITS messages
    are (type, p0, p1)); every other attribute is the model's.  The scheduler below swaps the model back in right after."""

    def __init__(self, model):
        self._model = model

    payloads = 2

    def __getattr__(self, name):
        return getattr(self._model, name)


# ====================================================================== STSScheduler with wildcards, messages (type, area)
class AreaWildcardSTSScheduler(X.ScalaWildcardSTSScheduler):
    def __init__(self, oracle, model, externals, rec, wildcards, present, subseq=None):
        super().__init__(oracle, _TwoFieldView(model), externals, rec, wildcards, present, subseq)
        self.model = model
        self.npay = int(getattr(model, "payloads", 2))
        self.max_pending = 0                          # (test bookkeeping) the most messages that were pending at once

    def _msg(self, k):
        e = self.trace[k]
        if self.wild[k] is not None:
            return self.wild[k]
        return (int(e["msg_type"]), area_of(e))

    # event_produced (:561-623): appendMsgSend
    def tell(self, snd, rcv, msg):
        uniq = self.next_uniq
        self.next_uniq += 1
        external = snd == DEAD and self.model.msg_class[msg[0]] == T.MSG_EXTERNAL
        ext_idx = self.ext_idx_queue.pop(0) if external else 255
        if self.enqueuedExternalMessages[msg] > 0 or not self.crosses_partition(snd, rcv):
            self.pendingEvents.setdefault((snd, rcv), OrderedDict()).setdefault(msg, []).append(uniq)
            p0, p1, p_hi = _split(msg[1])
            self.events.append((T.REC_MSG_SEND, self.dl if snd == DEAD else snd, rcv, msg[0], p0, p1,
                                1 if external else 2 if snd == DEAD else 0, ext_idx, p_hi, uniq))
            self.max_pending = max(self.max_pending, sum(len(q) for h in self.pendingEvents.values() for q in h.values()))

    def advanceReplay(self):
        while not self.trace_finished():
            e = self.trace[self.traceIdx]
            kind = int(e["kind"])
            snd = DEAD if int(e["snd"]) == self.dl else int(e["snd"])
            rcv = int(e["rcv"])
            if kind in (T.REC_SPAWN, T.REC_KILL, T.REC_PARTITION, T.REC_UNPARTITION):
                if kind == T.REC_SPAWN:
                    self.inaccessible.discard(rcv)
                    self.killed.discard(rcv)
                    self.blockedActors.discard(rcv)
                elif kind == T.REC_KILL:
                    self.killed.add(rcv)
                    self.inaccessible.add(rcv)
                elif kind == T.REC_PARTITION:
                    self.partitioned.add((int(e["snd"]), rcv))
                else:
                    self.partitioned.discard((int(e["snd"]), rcv))
                two = kind in (T.REC_PARTITION, T.REC_UNPARTITION)
                self.events.append((kind, int(e["snd"]) if two else 0, rcv, 0, 0, 0, 0, int(e["ext_idx"]), 0, 0))
                self.kept[self.index[self.traceIdx]] = 1
            elif kind == T.REC_MSG_SEND:
                if int(e["flags"]) & 1:                # EventTypes.isExternal(m): the recorded MsgSend carries the whole message
                    if rcv in self.actorToActorRef:
                        self.ext_idx_queue.append(int(e["ext_idx"]))
                        self.kept[self.index[self.traceIdx]] = 1
                    self.enqueue_message(None, rcv, (int(e["msg_type"]), area_of(e)))
            elif kind == T.REC_MSG_EVENT:
                if self.messagePending(snd, rcv, self._msg(self.traceIdx)):
                    break                              # "Yay, it's already enabled."
                self.ignored += 1                      # "Ignoring message"
                self.ignoredAbsentIndices.add(self.traceIdx)
            self.traceIdx += 1

    # :643-776
    def schedule_new_message(self):
        self.send_external_messages()
        self.advanceReplay()
        self.send_external_messages()
        if self.trace_finished():
            return None
        e = self.trace[self.traceIdx]
        snd = DEAD if int(e["snd"]) == self.dl else int(e["snd"])
        rcv = int(e["rcv"])
        msg = self._msg(self.traceIdx)
        outerKey = (snd, rcv)
        if isinstance(msg, X.WildCardMatch):
            pendingKeyValues = sorted(self.pendingEvents[outerKey].items(), key=lambda kv: kv[1][0])    # sortBy(_._2.head.id)
            pendingValues = [kv[0] for kv in pendingKeyValues]
            selectedMsgIdx = msg.msgSelector(pendingValues, lambda i: None)
            assert selectedMsgIdx is not None          # .get
            innerKey = pendingKeyValues[selectedMsgIdx][0]
            t0 = innerKey[0]
            if len({m for m in pendingValues if m[0] == t0}) >= 2:
                self.ambiguous += 1
        else:
            innerKey = msg
        queue = self.pendingEvents[outerKey][innerKey]
        assert queue, "Shouldnt be empty"
        uniq = queue.pop(0)
        if not queue:
            del self.pendingEvents[outerKey][innerKey]
            if not self.pendingEvents[outerKey]:
                del self.pendingEvents[outerKey]
        p0, p1, p_hi = _split(innerKey[1])
        self.events.append((T.REC_MSG_EVENT, self.dl if snd == DEAD else snd, rcv, innerKey[0], p0, p1, 0, 255, p_hi, uniq))   # appendMsgEvent
        self.kept[self.index[self.traceIdx]] = 1
        self.traceIdx += 1
        self.messagesScheduledSoFar += 1
        return (snd, rcv, innerKey, 0)

    def dispatch_new_message(self, snd, rcv, msg):
        mtype, area = msg
        src = self.dl if snd == DEAD else snd
        self.deliveries.append((src, rcv, mtype, area))
        if self.enqueuedExternalMessages[msg] > 0:                  # handle_event_consumed
            self.enqueuedExternalMessages[msg] -= 1
        c = self.timerToCancellable.get((rcv, msg))                 # "Check if it was a repeating timer. If so, retrigger it"
        if c is not None and c in self.ongoingCancellableTasks:
            self.handleTick(rcv, msg, c)
        st = (C.c_uint64 * self.stw)(*self.state[rcv])              # the actor's receive
        fx = (_Effect * 64)()
        lib = self.oracle.lib()
        if self.npay > 2:
            n = lib.orc_vm_run_area(C.byref(self.ms), rcv, st, mtype, src, area, self.exists, fx, 64, C.byref(self.seededRandom))
        else:
            n = lib.orc_vm_run(C.byref(self.ms), rcv, st, mtype, src, area & 0xFFFF, (area >> 16) & 0xFFFF, self.exists, fx, 64,
                               C.byref(self.seededRandom))
        assert n >= 0
        self.state[rcv] = [int(w) for w in st]
        for e in fx[:n]:
            if e.kind == 0:
                self.tell(rcv, int(e.target), (int(e.msg_type), int(e.area) if self.npay > 2 else int(e.p0) | int(e.p1) << 16))
            elif e.kind in (1, 2):                                  # scheduleOnce / schedule: the timer message has no payload
                self.registerCancellable(e.kind == 2, rcv, (int(e.msg_type), 0))
            elif e.kind == 3:
                self.cancelTimer(rcv, (int(e.msg_type), 0))
            elif e.kind == 4:                                       # actorCrashed
                self.blockedActors.add(rcv)

    def test(self, looking_for, match_mask):
        self.advanceReplay()
        while True:
            nxt = self.schedule_new_message()
            if nxt is None:
                break
            self.dispatch_new_message(nxt[0], nxt[1], nxt[2])
        assert self.trace_finished()
        fp = self.test_invariant()
        found = looking_for if fp and ((fp ^ looking_for) & match_mask) == 0 else 0
        h = 0xCBF29CE484222325
        for snd, rcv, mtype, area in self.deliveries:
            if self.wide:                              # the 64-bit word: header | area << 16
                w = (mtype | (rcv << 5) | (snd << 8) | (area << 16)) & MASK64
            else:
                w = mtype | (rcv << 5) | (snd << 8) | ((area & 0xFF) << 16) | (((area >> 16) & 0xFF) << 24)
            h = ((h ^ w) * 0x100000001B3) & MASK64
        for a in range(self.model.n_actors):
            for w in self.state[a]:
                h = ((h ^ w) * 0x100000001B3) & MASK64
        flags = (T.V_VIOLATION if found else 0) | (T.V_DIVERGED if self.ignored else 0) | min(self.messagesScheduledSoFar, 0xFFFF) << 16
        return flags, found, h


def run_candidate(oracle, model, trace, fp, wildcards, present, subseq=None):
    """One replay: (verdict triple, kept marks, executed trace, ignored record indices, scheduler)."""
    s = AreaWildcardSTSScheduler(oracle, model, trace.original_externals, trace.events, wildcards, present, subseq)
    v = s.test(fp.code, model.fp_match_mask)
    return v, s.kept, s.executed(), s.ignored_records(), s


def delivery_words(ev):
    """{(snd, rcv, type, area)} of the MsgEvents of a record array."""
    return {(int(e["snd"]), int(e["rcv"]), int(e["msg_type"]), area_of(e)) for e in ev if int(e["kind"]) == T.REC_MSG_EVENT}


def leaves_through_a_field_past_the_second(model, executed, recorded):
    """Does `executed` deliver a message whose AREA differs from that of EVERY recorded delivery in a field of index >= 2."""
    npay = int(getattr(model, "payloads", 2))
    if npay <= 2:
        return False
    rec_areas = [area_of(e) for e in recorded if int(e["kind"]) == T.REC_MSG_EVENT]
    hi = lambda a: tuple(T.payload_fields(a, npay)[2:])
    rec_hi = {hi(a) for a in rec_areas}
    return any(hi(area_of(e)) not in rec_hi for e in executed if int(e["kind"]) == T.REC_MSG_EVENT)


# ====================================================================== the clusterizers over (type, area) messages
def _msg_events(trace):
    ev = trace.events
    return [(int(i), int(ev["id"][i]), (int(ev["msg_type"][i]), area_of(ev[i])), None) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]]


class AreaFingerprinter(X.ScalaFingerprinter):
    def getLogicalClock(self, msg):
        k = self.model.clock_field.get(msg[0])
        return None if k is None else T.payload_fields(msg[1], int(getattr(self.model, "payloads", 2)))[k]


class AreaSingletonClusterizer(X.ScalaSingletonClusterizer):
    def __init__(self, originalTrace, fingerprinter, resolutionStrategy):
        super().__init__(originalTrace, fingerprinter, resolutionStrategy)
        self.me = _msg_events(originalTrace)          # (the base class's ids and sets read the types only: they stand)


class AreaClockClusterIterator(X.ScalaClockClusterIterator):
    def __init__(self, originalTrace, fingerprinter):
        self.fp = fingerprinter
        self.me = _msg_events(originalTrace)
        self.allIds = {id_ for _, id_, m, _ in self.me
                       if not fingerprinter.causesClockIncrement(m) and fingerprinter.getLogicalClock(m) is not None}
        self.firstClusterRemoval = True
        self.nextClockToRemove = -1
        self.blacklist = set()
        self.clocks = []
        self.clocks = self.computeRemainingClocks()


class AreaClockClusterizer(X.ScalaClockClusterizer):
    def __init__(self, originalTrace, fingerprinter, resolutionStrategy, aggressiveness=X.ALL_TIMERS_FIRST_ITR, skipClockClusters=False):
        self.originalTrace, self.fingerprinter, self.resolutionStrategy = originalTrace, fingerprinter, resolutionStrategy
        self.aggressiveness, self.skipClockClusters = aggressiveness, skipClockClusters
        self.me = _msg_events(originalTrace)
        self.clusterIterator = AreaClockClusterIterator(originalTrace, fingerprinter)
        assert self.clusterIterator.hasNext()
        self.currentCluster = self.clusterIterator.next()
        self.tryingFirstCluster = True
        self.timerIterator = X.ScalaOneAtATimeIterator(id_ for _, id_, m, _ in self.me if fingerprinter.causesClockIncrement(m))
        self.currentTimers = set()
        self.removed_clusters = []


class AreaWildcardMinimizer(X.ScalaWildcardMinimizer):
    """ScalaWildcardMinimizer over the schedulers and clusterizers above.  subseq: the externals (indices into the trace's) every
    replay keeps - WildcardTestOracle's use - or None for all of them."""

    def __init__(self, *a, subseq=None, memo=None, **kw):
        super().__init__(*a, **kw)
        self.subseq, self.memo = subseq, memo
        self.left_through_p_hi = 0
        self.max_pending = 0
        self.cluster_proposals = 0

    def testWithSTSSched(self, startTrace, present, wild):
        self.total_replays += 1
        key = None if self.memo is None else (self.subseq, np.asarray(present, dtype=bool).tobytes())
        if key is not None and key in self.memo:
            v, executed, ignored = self.memo[key]
        else:
            v, kept, executed, ignored, s = run_candidate(self.oracle, self.model, startTrace, self.violation, wild, present,
                                                          subseq=None if self.subseq is None else list(self.subseq))
            self.ambiguous += s.ambiguous
            self.max_pending = max(self.max_pending, s.max_pending)
            if key is not None:
                self.memo[key] = (v, executed, ignored)
        if leaves_through_a_field_past_the_second(self.model, executed, startTrace.events):
            self.left_through_p_hi += 1           # (counted over every replay, reproducing or not)
        if not (v[0] & T.V_VIOLATION):
            return None, set()
        if delivery_words(executed) - delivery_words(startTrace.events):
            self.left_the_recording += 1
        if self.subseq is not None:
            executed = executed.copy()            # the records name their external by its index: re-based on the subsequence
            for e in executed:
                if int(e["ext_idx"]) != 255:
                    e["ext_idx"] = self.subseq.index(int(e["ext_idx"]))
            return EventTrace(executed, startTrace.original_externals[list(self.subseq)]), set()
        return EventTrace(executed, self.mcs), ignored

    def minimize(self):
        fpr = AreaFingerprinter(self.model)
        aggressiveness = X.STOP_IMMEDIATELY if self.skipClockClusters else X.ALL_TIMERS_FIRST_ITR
        _resolutionStrategy = self.resolutionStrategy if self.resolutionStrategy is not None else X.ScalaBackTrackStrategy()
        if self.clusteringStrategy in ("ClockClusterizer", "ClockThenSingleton"):
            clusterizer = AreaClockClusterizer(self.trace, fpr, _resolutionStrategy, skipClockClusters=self.skipClockClusters,
                                               aggressiveness=aggressiveness)
            self.clock_values = list(clusterizer.clusterIterator.clocks)
        else:
            clusterizer = AreaSingletonClusterizer(self.trace, fpr, _resolutionStrategy)
        minTrace = self.doMinimize(clusterizer, self.trace)
        if self.clusteringStrategy == "ClockThenSingleton":
            minTrace = self.doMinimize(AreaSingletonClusterizer(minTrace, fpr, _resolutionStrategy), minTrace)
        return minTrace


class AreaTransliteratedDevice(X.TransliteratedDevice):
    """Stands in for StsWildcardOracle: every replay is an AreaWildcardSTSScheduler."""

    def test_batch(self, presents, violation):
        self.launches += 1
        return [bool(run_candidate(self.oracle, self.model, self.trace, violation, self.wild, p)[0][0] & T.V_VIOLATION) for p in presents]

    def executed(self, present, violation):
        v, kept, executed, ignored, _ = run_candidate(self.oracle, self.model, self.trace, violation, self.wild, present)
        if not (v[0] & T.V_VIOLATION):
            return None
        return EventTrace(executed, self.trace.original_externals, self.trace.ext_areas), ignored


# ====================================================================== WildcardTestOracle.scala, RunnerUtils.wildcardDDMin
class AreaWildcardTestOracle:
    """WildcardTestOracle.scala:11-61 (the shape of tests/test_wildcard_ddmin_cpu.py ScalaWildcardTestOracle)."""

    def __init__(self, oracle, model, strategy, originalTrace):
        self.oracle, self.model, self.strategy, self.originalTrace = oracle, model, strategy, originalTrace
        self.minTrace = originalTrace
        self.externalsForMinTrace = ()
        self.first_hits = []
        self.longer = 0
        self.memo = {}

    def test(self, events, violation_fingerprint, stats):
        minimizer = AreaWildcardMinimizer(self.oracle, self.model, self.originalTrace.original_externals, self.originalTrace,
                                          violation_fingerprint, skipClockClusters=True, resolutionStrategy=X.STRATEGIES[self.strategy][0](),
                                          subseq=tuple(events), memo=self.memo)
        trace = minimizer.minimize()
        if stats is not None:
            stats.increment_replays(minimizer.total_replays)
        self.first_hits.append(minimizer.total_replays - 1 if minimizer.successes else None)
        if trace is not minimizer.trace:
            if len(trace.events) < len(self.minTrace.events):
                self.minTrace = trace
                self.externalsForMinTrace = tuple(events)
            return trace
        self.longer += bool(minimizer.successes)
        return None


def scala_wildcard_ddmin(oracle, model, originalTrace, violation, strategy):
    """RunnerUtils.wildcardDDMin with the externals runTheGamut hands it (tests/test_wildcard_ddmin_cpu.py scala_wildcard_ddmin)."""
    externals = originalTrace.original_externals
    wo = AreaWildcardTestOracle(oracle, model, strategy, originalTrace)
    dag = UnmodifiedEventDag(externals)
    keep = tuple(i for i in dag.events if int(externals[i]["kind"]) != T.EV_WAIT_QUIESCENCE)
    stats = MinimizationStats()
    ddmin = DDMin(wo, stats=stats)
    mcs = ddmin.minimize(EventDagView(dag, keep), violation)
    consulted_hits = list(wo.first_hits)
    min_after_search = (tuple(wo.externalsForMinTrace), len(wo.minTrace.events))
    if mcs.length < len(keep):
        validated = ddmin.verify_mcs(mcs, violation)
        if validated is None:
            ret = (tuple(wo.externalsForMinTrace), wo.minTrace)
        else:
            ret = (tuple(mcs.events), EventTrace(validated.events, externals[list(mcs.events)]))
    else:
        ret = (tuple(mcs.events), originalTrace)
    return {"mcs": ret[0], "trace": ret[1], "consulted": list(ddmin.consulted), "first_hits": consulted_hits,
            "total_replays": stats.total_replays, "longer": wo.longer, "min": min_after_search, "memo": wo.memo}


# ====================================================================== the workloads
# Found by search on the CPU (tests/test_wildcard_payloads_cpu.py test_workload_conditions holds what they were chosen for) and
# pinned: (index into the violating executions of the trace found from apps.SEED_BASE).
REAL5 = dict(n=5, election_budget=2, log_cap=8, real_fields=True)      # wide, array_len 8, payloads 5: the application of the issue
REAL3 = dict(n=3, election_budget=2, log_cap=4, real_fields=True)
ARRAY5 = dict(n=5, election_budget=2, log_cap=8)                        # DEMI_MODEL_ARRAY without DEMI_MODEL_PAYLOADS
# table -> [(which execution, model arguments, index into the violating executions)]: "mcs" is the verified-MCS execution (fuzz ->
# DDMin -> re-based on the MCS), "full" the violating execution with every external that was injected.  On raft5_config2's trace
# no violating execution of the five-node table replicates an entry before the violation (every p_hi is 0), so the three-node
# table is loaded with its full executions: their client commands put fields past the second one on the wire.
WORKLOADS = {"real5": (("mcs", REAL5, 0), ("mcs", REAL5, 2)),
             "real3": (("full", REAL3, 0), ("full", REAL3, 16), ("full", REAL3, 26)),
             "array5": (("mcs", ARRAY5, 0), ("mcs", ARRAY5, 2))}
# the wildcardDDMin workload on the five-node real-field table: the 20-event trace of the fuzzer (18 externals injected), its second
# violating execution, BackTrackStrategy - consultations that reproduce only without a later timer (first_hit 13) and ones in
# which no proposal reproduces, an MCS of 6 of the 18
DDMIN_EVENTS, DDMIN_SKIP, DDMIN_STRATEGY = 20, 1, "BackTrackStrategy"

_memo = {}


def _model(kw):
    kw = dict(kw)
    return M.raft_model(kw.pop("n"), **kw)


def raft3_events():
    return events_to_array([start(a) for a in range(3)] + [send(a, M.M_BOOTSTRAP) for a in range(3)] +
                           [send(a % 3, M.M_CLIENT, 1 + a) for a in range(6)] + [wait_quiescence()] +
                           [send(a % 3, M.M_CLIENT, 7 + a) for a in range(4)])


def _events_and_limits(kw):
    if kw["n"] == 5:
        _, events, lim = raft5_config2()
        return events, lim
    return raft3_events(), T.Limits(120, 0, 128, 0, 0, 0)


def workload(oracle, kw, skip):
    """(model, verified-MCS trace, fingerprint): fuzz -> DDMin -> verified MCS, as X.raft5_workload."""
    key = ("mcs", tuple(sorted(kw.items())), skip)
    if key not in _memo:
        model = _model(kw)
        events, lim = _events_and_limits(kw)
        trace, fp = _verified_mcs(oracle, model, events, lim, skip)
        _memo[key] = (model, trace, fp)
    return _memo[key]


def full_workload(oracle, kw, skip):
    """(model, the violating execution with all the externals that were injected, fingerprint), as D.workload."""
    key = ("full", tuple(sorted(kw.items())), skip)
    if key not in _memo:
        model = _model(kw)
        events, lim = _events_and_limits(kw)
        vv, rec, used = _violating_execution(oracle, model, events, lim, skip)
        _memo[key] = (model, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint))
    return _memo[key]


def ddmin_workload(oracle):
    """(model, the violating execution with all the externals that were injected, fingerprint, strategy)."""
    if "ddmin" not in _memo:
        from demi_amd.apps import TRACE_SEED
        from demi_amd.fuzzer import raft_trace
        model = _model(REAL5)
        events = events_to_array(raft_trace(5, DDMIN_EVENTS, TRACE_SEED))
        vv, rec, used = _violating_execution(oracle, model, events, T.Limits(200, 30, 64, 0, 0, 0), DDMIN_SKIP)
        _memo["ddmin"] = (model, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint), DDMIN_STRATEGY)
    return _memo["ddmin"]


def ddmin_reference(oracle):
    if "ddmin_ref" not in _memo:
        model, trace, fp, strategy = ddmin_workload(oracle)
        _memo["ddmin_ref"] = scala_wildcard_ddmin(oracle, model, trace, fp, strategy)
    return _memo["ddmin_ref"]


def get(oracle, spec):
    which, kw, skip = spec
    return (workload if which == "mcs" else full_workload)(oracle, kw, skip)


# ====================================================================== the ledger workload of the DPOR tests
# (the smallest shape at which the gather can go wrong: the Send with the memo is neither the first nor the last external, so a
# subsequence without an earlier Send needs areas[original index], not a prefix; every DPOR instance of the Python loops compiles
# the table for itself, so the number of subsequences consulted is what the GPU tests' time is made of)
LEDGER_ACTORS, LEDGER_SENDS = 2, 3


def ledger_workload():
    """tests/test_payloads_gpu.py's ledger table (five fields; the invariant is decided by the FOURTH field of an external
    Deposit) with Start / Send externals only, and the payload area of every external.  -> (model, externals, areas)."""
    from .test_payloads_gpu import _ledger_model
    model = _ledger_model(LEDGER_ACTORS)
    rng = np.random.default_rng(11)
    ev, areas = [start(a) for a in range(LEDGER_ACTORS)], [0] * LEDGER_ACTORS
    for i in range(LEDGER_SENDS):
        acct, amount = int(rng.integers(0, 512)), int(rng.integers(0, 512))
        fields = [acct, amount, int(rng.integers(0, 512)), 0x1A5 if i == LEDGER_SENDS - 2 else int(rng.integers(0, 0x1A0)), int(rng.integers(0, 512))]
        ev.append(send(int(rng.integers(0, LEDGER_ACTORS)), 0, acct, amount))
        areas.append(T.pay_area(fields, 5))
    return model, events_to_array(ev), np.array(areas, dtype=np.uint64)


def ledger_execution(oracle, model, events, areas, seed=3):
    """A violating execution of the ledger workload recorded by the oracle given the areas: (EventTrace with ext_areas, fingerprint)."""
    oracle.set_ext_areas(areas)
    try:
        v, rec, _ = oracle.random_execute(model, events, seed, T.Limits(200, 0, 64, 0, 0, 0))
    finally:
        oracle.set_ext_areas(None)
    assert v.flags & T.V_VIOLATION
    return EventTrace(rec, events, areas.copy()), ViolationFingerprint(int(v.fingerprint), model.fp_match_mask)


def oracle_backend_with_areas(oracle, log=None):
    """DPORwHeuristics' `backend` over the CPU oracle that takes the areas keyword: orc_set_ext_areas per consultation."""
    def backend(model, externals, prefixes, params, shared=None, areas=None):
        if log is not None:
            log.append((np.array(externals), None if areas is None else np.array(areas, dtype=np.uint64)))
        oracle.set_ext_areas(areas)
        try:
            return oracle.dpor_batch(model, externals, prefixes, params, shared)
        finally:
            oracle.set_ext_areas(None)
    return backend
