"""CPU suite: the wildcard (fungible-clock) minimizers transliterated from the Scala, and the demi_amd mirror's host logic
against them.

  STSScheduler.messagePending / schedule_new_message for MsgEvent(snd, rcv, WildCardMatch(selector, _))
                                                            (schedulers/STSScheduler.scala:380-402, 696-711)
  SrcDstFIFOOnly, BackTrackStrategy, FirstAndLastBacktrack, LastOnlyStrategy
                                                            (minification/wildcard_minimization/AmbiguityResolutionStrategies.scala)
  SingletonClusterizer                                      (.../OneAtATimeClusterizer.scala)
  ClockClusterizer, ClockClusterIterator, OneAtATimeIterator, Aggressiveness   (.../ClockClusterizer.scala)
  WildcardMinimizer.minimize / doMinimize with TestScheduler.STSSched         (.../WildcardMinimizer.scala)
  RunnerUtils.testWithStsSched                              (RunnerUtils.scala:913-943)

ScalaWildcardSTSScheduler is ScalaSTSScheduler (tests/test_sts_scheduler_transliteration_cpu.py) with pendingEvents as the
reference has it, taking a trace whose MsgEvents may be wildcards; it records the ignoredAbsentIndices and returns the
executed trace.  The executed trace is written down in the library's convention (demi_replay_get_kept): applied external
events, external MsgSends, every MsgEvent, and the MsgSend of every DELIVERED internal / timer message where it was sent;
Uniq ids renumbered in order of appearance.  tests/test_wildcard_gpu.py holds the kernel against this file, bit for bit."""
from collections import OrderedDict

import numpy as np
import pytest

from demi_amd import model as M
from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.apps import SEED_BASE, raft5_config2
from demi_amd.fuzzer import FuzzerWeights, events_to_array, raft_trace
from demi_amd.schedulers import EventTrace, MinimizationStats, ViolationFingerprint

from .test_internal_min_cpu import _verified_mcs
from .test_minification_cpu import _scala_subsequence_intersection
from .test_random_scheduler_transliteration_cpu import DEAD, MASK64
from .test_sts_scheduler_transliteration_cpu import ScalaSTSScheduler


# ====================================================================== AmbiguityResolutionStrategies.scala
class ScalaSrcDstFIFOOnly:
    def resolve(self, msgSelector, pending, backtrackSetter):
        if len(pending) > 0:                       # pending.headOption match { case Some(msg) =>
            return 0 if msgSelector(pending[0]) else None
        return None


class ScalaBackTrackStrategy:
    def resolve(self, msgSelector, pending, backtrackSetter):
        matching = [(msg, i) for i, msg in enumerate(pending) if msgSelector(msg)]
        if matching:
            alreadyTried = {matching[0][0]}
            for msg, i in reversed(matching[1:]):
                if msg not in alreadyTried:
                    alreadyTried.add(msg)
                    backtrackSetter(i)
            return matching[0][1]
        return None


class ScalaFirstAndLastBacktrack:
    def resolve(self, msgSelector, pending, backtrackSetter):
        matching = [(msg, i) for i, msg in enumerate(pending) if msgSelector(msg)]
        if matching:
            alreadyTried = {matching[0][0]}
            for msg, i in reversed(matching[1:]):          # .find
                if msg not in alreadyTried:
                    alreadyTried.add(msg)
                    backtrackSetter(i)
                    break
            return matching[0][1]
        return None


class ScalaLastOnlyStrategy:
    def resolve(self, msgSelector, pending, backtrackSetter):
        matching = [(msg, i) for i, msg in enumerate(pending) if msgSelector(msg)]
        return matching[-1][1] if matching else None


STRATEGIES = {"SrcDstFIFOOnly": (ScalaSrcDstFIFOOnly, W.SrcDstFIFOOnly), "BackTrackStrategy": (ScalaBackTrackStrategy, W.BackTrackStrategy),
              "FirstAndLastBacktrack": (ScalaFirstAndLastBacktrack, W.FirstAndLastBacktrack),
              "LastOnlyStrategy": (ScalaLastOnlyStrategy, W.LastOnlyStrategy)}
SCALA_OF_POLICY = {T.WILDCARD_HEAD: ScalaSrcDstFIFOOnly, T.WILDCARD_FIRST: ScalaBackTrackStrategy, T.WILDCARD_LAST: ScalaLastOnlyStrategy}


class WildCardMatch:
    def __init__(self, msgSelector, name=""):
        self.msgSelector, self.name = msgSelector, name


def class_tag_wildcard(mtype, strategy):
    """WildCardMatch((lst, backtrackSetter) => resolutionStrategy.resolve(messageFilter, lst, backtrackSetter), name=classTag)"""
    def messageFilter(pendingMsg):
        return pendingMsg[0] == mtype                 # ClassTag(pendingMsg.getClass) == classTag
    return WildCardMatch(lambda lst, backtrackSetter: strategy.resolve(messageFilter, lst, backtrackSetter), name=str(mtype))


def type_set_wildcard(types, policy):
    """The selector the device knows as (type set, policy), out of the transliterated strategies."""
    strategy = SCALA_OF_POLICY[policy]()
    return WildCardMatch(lambda lst, bs: strategy.resolve(lambda m: bool((types >> m[0]) & 1), lst, bs), name="%x/%d" % (types, policy))


# ====================================================================== STSScheduler with wildcards
class ScalaWildcardSTSScheduler(ScalaSTSScheduler):
    """wtrace: [(record index, WildCardMatch | None)] - the events of the (projected) trace, MsgEvents possibly wildcarded."""

    def __init__(self, oracle, model, externals, rec, wildcards, present, subseq=None):
        """wildcards[i]: WildCardMatch or None per record; present[i]: is the MsgEvent at record i part of the trace."""
        if subseq is None:
            subseq = [i for i in range(len(externals)) if int(externals[i]["kind"]) != T.EV_WAIT_QUIESCENCE]
        super().__init__(oracle, model, externals, rec, subseq)
        proj = _scala_subsequence_intersection(rec, externals, subseq, model)
        self.index = [i for i in proj if int(rec[i]["kind"]) != T.REC_MSG_EVENT or present[i]]
        self.trace = [rec[i] for i in self.index]
        self.wild = [wildcards[i] if int(rec[i]["kind"]) == T.REC_MSG_EVENT else None for i in self.index]
        self.ignoredAbsentIndices = set()             # indices into self.trace (IgnoreAbsentCallback)
        self.kept = np.zeros(len(rec), dtype=np.uint8)
        self.events = []                              # event_orchestrator.events: tuples in REC_EVENT field order
        self.ext_idx_queue = []
        self.uniq_of_delivery = None
        self.ambiguous = 0                            # wildcards that met two or more matching groups (FIRST != LAST)

    def _msg(self, k):
        e = self.trace[k]
        if self.wild[k] is not None:
            return self.wild[k]
        return (int(e["msg_type"]), int(e["p0"]), int(e["p1"]))

    # event_produced (:561-623): appendMsgSend
    def tell(self, snd, rcv, msg):
        uniq = self.next_uniq
        self.next_uniq += 1
        external = snd == DEAD and self.model.msg_class[msg[0]] == T.MSG_EXTERNAL
        ext_idx = self.ext_idx_queue.pop(0) if external else 255
        if self.enqueuedExternalMessages[msg] > 0 or not self.crosses_partition(snd, rcv):
            self.pendingEvents.setdefault((snd, rcv), OrderedDict()).setdefault(msg, []).append(uniq)
            self.events.append((T.REC_MSG_SEND, self.dl if snd == DEAD else snd, rcv, msg[0], msg[1], msg[2],
                                1 if external else 2 if snd == DEAD else 0, ext_idx, 0, uniq))

    # :380-402
    def messagePending(self, sender, receiver, msg):
        self.send_external_messages()
        hash_ = self.pendingEvents.get((sender, receiver))
        if hash_ is not None:
            if isinstance(msg, WildCardMatch):
                lst = sorted((u, m) for m, q in hash_.items() for u in q)         # hash.values.flatten.toSeq.sortBy(id)
                queueOpt = msg.msgSelector([m for _, m in lst], lambda i: None)
            else:
                queueOpt = hash_.get(msg)
        else:
            queueOpt = None
        if queueOpt is not None:
            return receiver not in self.blockedActors
        return False

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
                if int(e["flags"]) & 1:                # EventTypes.isExternal(m)
                    if rcv in self.actorToActorRef:
                        self.ext_idx_queue.append(int(e["ext_idx"]))
                        self.kept[self.index[self.traceIdx]] = 1
                    self.enqueue_message(None, rcv, (int(e["msg_type"]), int(e["p0"]), int(e["p1"])))
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
        if isinstance(msg, WildCardMatch):
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
        # appendMsgEvent
        self.events.append((T.REC_MSG_EVENT, self.dl if snd == DEAD else snd, rcv, innerKey[0], innerKey[1], innerKey[2], 0, 255, 0, uniq))
        self.kept[self.index[self.traceIdx]] = 1
        self.traceIdx += 1
        self.messagesScheduledSoFar += 1
        return (snd, rcv, innerKey, 0)

    def notify_timer_cancel(self, rcv, msg):
        if self.handle_timer_cancel(rcv, msg):
            return
        inner = self.pendingEvents.get((DEAD, rcv))
        if inner is not None and msg in inner:
            inner[msg].pop(0)                          # queue.dequeueFirst(t => message == msg)
            if not inner[msg]:
                del inner[msg]
                if not inner:
                    del self.pendingEvents[(DEAD, rcv)]

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
        for snd, rcv, mtype, p0, p1 in self.deliveries:
            w = mtype | (rcv << 5) | (snd << 8) | (p0 << 16) | (p1 << (32 if self.wide else 24))
            h = ((h ^ w) * 0x100000001B3) & MASK64
        for a in range(self.model.n_actors):
            for w in self.state[a]:
                h = ((h ^ w) * 0x100000001B3) & MASK64
        flags = (T.V_VIOLATION if found else 0) | (T.V_DIVERGED if self.ignored else 0) | min(self.messagesScheduledSoFar, 0xFFFF) << 16
        return flags, found, h

    def ignored_records(self):
        return {self.index[k] for k in self.ignoredAbsentIndices}

    def executed(self):
        """event_orchestrator.events in the library's convention (module docstring), as REC_EVENT records."""
        delivered = {e[9] for e in self.events if e[0] == T.REC_MSG_EVENT}
        out, renum = [], {}
        for e in self.events:
            if e[0] == T.REC_MSG_SEND and not (e[6] & 1) and e[9] not in delivered:
                continue
            e = list(e)
            if e[0] in (T.REC_MSG_SEND, T.REC_MSG_EVENT):
                e[9] = renum.setdefault(e[9], len(renum) + 1)
            out.append(tuple(e))
        return np.array(out, dtype=T.REC_EVENT_DTYPE) if out else np.zeros(0, dtype=T.REC_EVENT_DTYPE)


def run_candidate(oracle, model, trace, fp, wildcards, present, subseq=None):
    """One replay: (verdict triple, kept marks, executed trace, ignored record indices, scheduler)."""
    s = ScalaWildcardSTSScheduler(oracle, model, trace.original_externals, trace.events, wildcards, present, subseq)
    v = s.test(fp.code, model.fp_match_mask)
    return v, s.kept, s.executed(), s.ignored_records(), s


def wildcards_of(type_sets, policies):
    return [type_set_wildcard(int(t), int(p)) if int(t) else None for t, p in zip(type_sets, policies)]


# ====================================================================== the clusterizers, line by line
def _msg_events(trace):
    """[(record index, id, msg, external)] of the UniqueMsgEvents."""
    ev = trace.events
    return [(int(i), int(ev["id"][i]), (int(ev["msg_type"][i]), int(ev["p0"][i]), int(ev["p1"][i])), None)
            for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]]


class ScalaFingerprinter:
    """MessageFingerprinter's clock hooks (MessageFingerprints.scala:26-31) over the model's metadata."""

    def __init__(self, model):
        self.model = model

    def causesClockIncrement(self, msg):
        return msg[0] in self.model.clock_increment_types

    def getLogicalClock(self, msg):
        k = self.model.clock_field.get(msg[0])
        return None if k is None else msg[1 + k]

    def isExternal(self, msg):
        return self.model.msg_class[msg[0]] == T.MSG_EXTERNAL


class ScalaSingletonClusterizer:
    def __init__(self, originalTrace, fingerprinter, resolutionStrategy):
        self.originalTrace, self.fingerprinter, self.resolutionStrategy = originalTrace, fingerprinter, resolutionStrategy
        self.me = _msg_events(originalTrace)
        self.sortedIds = sorted(id_ for _, id_, m, _ in self.me if not fingerprinter.isExternal(m))
        self.allIds = set(self.sortedIds) | {id_ for _, id_, m, _ in self.me if fingerprinter.isExternal(m)}
        self.successfullyRemoved = set()
        self.ignoredLastRun = -1
        self.firstRun = True

    def getNextTrace(self, violationReproducedLastRun, ignoredAbsentIds):
        if not self.sortedIds:
            return None
        if violationReproducedLastRun:
            self.successfullyRemoved = (self.successfullyRemoved | set(ignoredAbsentIds)) | {self.ignoredLastRun}
        if not self.firstRun:
            self.ignoredLastRun = self.sortedIds[0]
            self.sortedIds = self.sortedIds[1:]
        else:
            self.firstRun = False
        currentCluster = self.allIds - (self.successfullyRemoved - {self.ignoredLastRun})
        n = len(self.originalTrace.events)
        present, wild = np.zeros(n, dtype=bool), [None] * n
        for i, id_, msg, _ in self.me:
            if self.fingerprinter.isExternal(msg):
                present[i] = True
            elif id_ in currentCluster:
                present[i] = True
                wild[i] = class_tag_wildcard(msg[0], self.resolutionStrategy)
        return present, wild


class ScalaClockClusterIterator:
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

    def computeRemainingClocks(self):
        lowest = self.clocks[0] if self.clocks else 0
        vals = set()
        for _, id_, m, _ in self.me:
            if id_ not in self.blacklist:
                c = self.fp.getLogicalClock(m)
                if c is not None:
                    vals.add(c)
        out = sorted(vals)
        while out and out[0] < lowest:                 # dropWhile
            out = out[1:]
        return out

    def current(self):
        currentClockToRemove = -1 if self.firstClusterRemoval else self.nextClockToRemove
        out = set()
        for _, id_, m, _ in self.me:
            if self.fp.causesClockIncrement(m):
                continue
            clock = self.fp.getLogicalClock(m)
            if clock is None:
                out.add(id_)
            elif clock == currentClockToRemove or id_ in self.blacklist:
                pass
            else:
                out.add(id_)
        return out

    def next(self):
        if self.firstClusterRemoval:
            ret = self.current()
            self.firstClusterRemoval = False
            return ret
        self.nextClockToRemove = self.clocks[0]
        ret = self.current()
        self.clocks = self.clocks[1:]
        return ret

    def hasNext(self):
        return self.firstClusterRemoval or len(self.clocks) > 0

    def producedViolation(self, previouslyIncluded, ignoredAbsents):
        self.blacklist = self.blacklist | self.inverse(previouslyIncluded)
        if ignoredAbsents:
            self.blacklist = self.blacklist | (self.allIds & set(ignoredAbsents))
            self.clocks = self.computeRemainingClocks()

    def inverse(self, toInclude):
        return self.allIds - set(toInclude)


class ScalaOneAtATimeIterator:
    def __init__(self, all_):
        self.all = set(all_)
        self.toRemove = sorted(self.all)
        self.first = True
        self.blacklist = set()

    def current(self):
        if self.first:
            return self.all - self.blacklist
        return (self.all - {self.toRemove[0]}) - self.blacklist

    def next(self):
        if self.first:
            ret = self.current()
            self.first = False
            return ret
        ret = self.current()
        self.toRemove = self.toRemove[1:]
        return ret

    def hasNext(self):
        return self.first or len(self.toRemove) > 0

    def producedViolation(self, previouslyIncluded, ignoredAbsents):
        self.blacklist = self.blacklist | self.inverse(previouslyIncluded) | (self.all & set(ignoredAbsents))

    def reset(self):
        self.toRemove = sorted(self.all - self.blacklist)
        self.first = True

    def inverse(self, toInclude):
        return self.all - set(toInclude)


NONE, ALL_TIMERS_FIRST_ITR, STOP_IMMEDIATELY = 0, 1, 2


class ScalaClockClusterizer:
    def __init__(self, originalTrace, fingerprinter, resolutionStrategy, aggressiveness=ALL_TIMERS_FIRST_ITR, skipClockClusters=False):
        self.originalTrace, self.fingerprinter, self.resolutionStrategy = originalTrace, fingerprinter, resolutionStrategy
        self.aggressiveness, self.skipClockClusters = aggressiveness, skipClockClusters
        self.me = _msg_events(originalTrace)
        self.clusterIterator = ScalaClockClusterIterator(originalTrace, fingerprinter)
        assert self.clusterIterator.hasNext()
        self.currentCluster = self.clusterIterator.next()
        self.tryingFirstCluster = True
        self.timerIterator = ScalaOneAtATimeIterator(id_ for _, id_, m, _ in self.me if fingerprinter.causesClockIncrement(m))
        self.currentTimers = set()
        self.removed_clusters = []                      # (test bookkeeping) clock values whose cluster was proposed for removal

    def getNextTrace(self, violationReproducedLastRun, ignoredAbsentIds):
        if violationReproducedLastRun:
            self.timerIterator.producedViolation(self.currentTimers, ignoredAbsentIds)
            self.clusterIterator.producedViolation(self.currentCluster, ignoredAbsentIds)
        if (not self.timerIterator.hasNext() or
                (self.aggressiveness == ALL_TIMERS_FIRST_ITR and violationReproducedLastRun and not self.tryingFirstCluster) or
                (self.aggressiveness == STOP_IMMEDIATELY and violationReproducedLastRun)):
            self.tryingFirstCluster = False
            if not self.clusterIterator.hasNext() or self.skipClockClusters:
                return None
            self.timerIterator.reset()
            self.currentCluster = self.clusterIterator.next()
            self.removed_clusters.append(self.clusterIterator.nextClockToRemove)
        assert self.timerIterator.hasNext()
        self.currentTimers = self.timerIterator.next()
        n = len(self.originalTrace.events)
        present, wild = np.zeros(n, dtype=bool), [None] * n
        fpr = self.fingerprinter
        for i, id_, msg, _ in self.me:
            if fpr.isExternal(msg):
                present[i] = True
            elif id_ in self.currentTimers:
                present[i] = True

                def sel(lst, backtrackSetter):
                    idx = next((k for k, m in enumerate(lst) if fpr.causesClockIncrement(m)), -1)     # indexWhere
                    return None if idx == -1 else idx
                wild[i] = WildCardMatch(sel, name="CausesClockIncrement")
            elif id_ in self.currentCluster:
                present[i] = True
                wild[i] = class_tag_wildcard(msg[0], self.resolutionStrategy)
        return present, wild


class ScalaWildcardMinimizer:
    """WildcardMinimizer with TestScheduler.STSSched; `test` is RunnerUtils.testWithStsSched."""

    def __init__(self, oracle, model, mcs, trace, violation, skipClockClusters=False, resolutionStrategy=None,
                 clusteringStrategy="ClockClusterizer"):
        self.oracle, self.model, self.mcs, self.violation = oracle, model, mcs, violation
        self.trace = EventTrace(trace.events, mcs)
        self.skipClockClusters = skipClockClusters
        self.resolutionStrategy = resolutionStrategy
        self.clusteringStrategy = clusteringStrategy
        self.total_replays = 0
        self.proposals = []
        self.successes = 0
        self.ambiguous = 0
        self.left_the_recording = 0
        self.removed_clusters_that_reproduced = []
        self.clock_values = []

    def testWithSTSSched(self, startTrace, present, wild):
        self.total_replays += 1                         # stats.increment_replays (STSScheduler.test)
        v, kept, executed, ignored, s = run_candidate(self.oracle, self.model, startTrace, self.violation, wild, present)
        self.ambiguous += s.ambiguous
        if not (v[0] & T.V_VIOLATION):
            return None, set()
        words = lambda ev: {(int(e["snd"]), int(e["rcv"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"]))
                            for e in ev if int(e["kind"]) == T.REC_MSG_EVENT}
        if words(executed) - words(startTrace.events):
            self.left_the_recording += 1
        return EventTrace(executed, self.mcs), ignored

    def minimize(self):
        fpr = ScalaFingerprinter(self.model)
        aggressiveness = STOP_IMMEDIATELY if self.skipClockClusters else ALL_TIMERS_FIRST_ITR
        _resolutionStrategy = self.resolutionStrategy if self.resolutionStrategy is not None else ScalaBackTrackStrategy()
        if self.clusteringStrategy in ("ClockClusterizer", "ClockThenSingleton"):
            clusterizer = ScalaClockClusterizer(self.trace, fpr, _resolutionStrategy, skipClockClusters=self.skipClockClusters,
                                                aggressiveness=aggressiveness)
            self.clock_values = list(clusterizer.clusterIterator.clocks)
        else:
            clusterizer = ScalaSingletonClusterizer(self.trace, fpr, _resolutionStrategy)
        minTrace = self.doMinimize(clusterizer, self.trace)
        if self.clusteringStrategy == "ClockThenSingleton":
            minTrace = self.doMinimize(ScalaSingletonClusterizer(minTrace, fpr, _resolutionStrategy), minTrace)
        return minTrace

    def doMinimize(self, clusterizer, startTrace):
        minTrace = startTrace
        ev = startTrace.events
        nextTrace = clusterizer.getNextTrace(False, set())
        while nextTrace is not None:
            present, wild = nextTrace
            self.proposals.append(present)
            ret, ignoredAbsentIndices = self.testWithSTSSched(startTrace, present, wild)
            ignoredAbsentIds = set()
            if ret is not None:
                self.successes += 1
                if isinstance(clusterizer, ScalaClockClusterizer) and clusterizer.removed_clusters and not clusterizer.tryingFirstCluster:
                    self.removed_clusters_that_reproduced.append(clusterizer.removed_clusters[-1])
                if len(ret.events) <= len(minTrace.events):
                    minTrace = ret
                for i in ignoredAbsentIndices:
                    ignoredAbsentIds.add(int(ev["id"][i]))
            nextTrace = clusterizer.getNextTrace(ret is not None, ignoredAbsentIds)
        return minTrace


# ====================================================================== the mirror against the transliteration
class TransliteratedDevice:
    """Stands in for StsWildcardOracle (same interface): every replay is a ScalaWildcardSTSScheduler."""

    def __init__(self, oracle, model):
        self.oracle, self.model = oracle, model
        self.launches = 0

    def load(self, trace, type_sets, policies):
        self.trace, self.wild = trace, wildcards_of(type_sets, policies)

    def test_batch(self, presents, violation):
        self.launches += 1
        return [bool(run_candidate(self.oracle, self.model, self.trace, violation, self.wild, p)[0][0] & T.V_VIOLATION) for p in presents]

    def executed(self, present, violation):
        v, kept, executed, ignored, _ = run_candidate(self.oracle, self.model, self.trace, violation, self.wild, present)
        if not (v[0] & T.V_VIOLATION):
            return None
        return EventTrace(executed, self.trace.original_externals), ignored


# The workloads: verified-MCS executions of raft5_config2's trace on the raft table with election_budget = 2, for these violating
# seeds (index into the violating executions found from SEED_BASE).  With the default budget of 1 no wildcard ever meets two
# matching groups and no clock cluster goes; these were chosen on the transliteration alone (test_workload_conditions).
WORKLOAD_SKIPS = (0, 2, 3)
WORKLOAD_MODEL = {"election_budget": 2}


def raft5_workload(oracle, skip, **model_kw):
    model, events, lim = raft5_config2()
    if model_kw:
        model = M.raft_model(5, **model_kw)
    trace, fp = _verified_mcs(oracle, model, events, lim, skip)
    return model, trace, fp


def fault_heavy_workload(oracle, seed=1):
    """The fault-heavy trace of tests/test_sts_scheduler_transliteration_cpu.py (kills, partitions), as one loaded execution."""
    model = M.raft_model(5, election_budget=2)
    w = FuzzerWeights(kill=0.12, send=0.4, wait_quiescence=0.13, partition=0.2, unpartition=0.15)
    events = events_to_array(raft_trace(5, 70, seed, w, exact=False))
    vv, rec, _ = oracle.random_execute(model, events, SEED_BASE + seed, T.Limits(300, 10, 128, 0, 0, 0))
    used = events[:T.verdict_trace_idx(vv.flags)]
    return model, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint if vv.fingerprint else 0x1000103)


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_strategies_equal_their_transliterations(strategy):
    scala, mirror = STRATEGIES[strategy][0](), STRATEGIES[strategy][1]()
    rng = np.random.default_rng(3)
    for _ in range(300):
        pending = [(int(rng.integers(0, 3)), int(rng.integers(0, 2)), 0) for _ in range(int(rng.integers(0, 6)))]
        t = int(rng.integers(0, 3))
        sel = lambda m: m[0] == t
        assert scala.resolve(sel, pending, lambda i: None) == mirror.resolve(sel, pending, lambda i: None)
        # and as the device knows it: (type set, policy)
        assert type_set_wildcard(1 << t, mirror.policy).msgSelector(pending, lambda i: None) == scala.resolve(sel, pending, lambda i: None)


@pytest.mark.parametrize("clustering", ["ClockClusterizer", "SingletonClusterizer", "ClockThenSingleton"])
@pytest.mark.parametrize("strategy", ["BackTrackStrategy", "LastOnlyStrategy", "SrcDstFIFOOnly"])
def test_mirror_proposes_and_returns_what_the_transliteration_does(oracle, clustering, strategy):
    model, trace, fp = raft5_workload(oracle, WORKLOAD_SKIPS[0])
    ref = ScalaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=STRATEGIES[strategy][0](),
                                 clusteringStrategy=clustering)
    want = ref.minimize()
    for max_batch in (1, 16384):
        stats = MinimizationStats()
        m = W.WildcardMinimizer(W.SchedulerConfig(model=model), trace.original_externals, trace, fp,
                                resolutionStrategy=STRATEGIES[strategy][1](), clusteringStrategy=clustering, stats=stats,
                                max_batch=max_batch, oracle=TransliteratedDevice(oracle, model))
        _, got = m.minimize()
        assert len(m.proposals) == len(ref.proposals) and all((a == b).all() for a, b in zip(m.proposals, ref.proposals))
        assert stats.total_replays == ref.total_replays
        assert len(got.events) == len(want.events) and (got.events == want.events).all()


def test_skip_clock_clusters_only_explores_timers(oracle):
    model, trace, fp = raft5_workload(oracle, WORKLOAD_SKIPS[1])
    ref = ScalaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, skipClockClusters=True)
    want = ref.minimize()
    stats = MinimizationStats()
    m = W.WildcardMinimizer(W.SchedulerConfig(model=model), trace.original_externals, trace, fp, skipClockClusters=True, stats=stats,
                            oracle=TransliteratedDevice(oracle, model))
    _, got = m.minimize()
    assert stats.total_replays == ref.total_replays and (got.events == want.events).all()


def test_a_model_without_clocks_degenerates_as_the_default_fingerprinter(oracle):
    model, trace, fp = raft5_workload(oracle, WORKLOAD_SKIPS[0])
    model.clock_increment_types, model.clock_field = frozenset(), {}
    ref = ScalaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp)
    ref.minimize()
    assert ref.total_replays == 1 and ref.clock_values == []      # one trace: everything wildcarded, nothing to remove
    stats = MinimizationStats()
    W.WildcardMinimizer(W.SchedulerConfig(model=model), trace.original_externals, trace, fp, stats=stats,
                        oracle=TransliteratedDevice(oracle, model)).minimize()
    assert stats.total_replays == 1


def test_workload_conditions(oracle):
    """What the GPU comparison rests on, asserted on the transliteration's runs alone: (a) an ambiguous wildcard (two or more
    matching groups, FIRST != LAST), (b) a replay that leaves the recorded trace, (c) two or more clock values and a whole clock
    cluster removed, (d) the wildcard stages end with fewer deliveries than the internal minimization left."""
    from demi_amd.internal_minimization import LeftToRightOneAtATime, STSSchedMinimizer, countMsgEvents
    from .test_internal_min_cpu import OracleRemoval
    ambiguous = left = 0
    cluster_removed = shrunk = False
    for skip in WORKLOAD_SKIPS:
        model, trace, fp = raft5_workload(oracle, skip, **WORKLOAD_MODEL)
        ref = ScalaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=ScalaLastOnlyStrategy(),
                                     clusteringStrategy="ClockThenSingleton")
        ref.minimize()
        ambiguous += ref.ambiguous
        left += ref.left_the_recording
        cluster_removed |= len(ref.clock_values) >= 2 and bool(ref.removed_clusters_that_reproduced)
        # (d): DDMin -> IntMin -> WildcardsNoBackTracks -> WildcardsLastOnly, as run_the_gamut chains them
        _, intmin = STSSchedMinimizer(trace.original_externals, trace, fp, LeftToRightOneAtATime(trace, model), OracleRemoval(oracle, model)).minimize()
        cur = intmin
        for strat in (None, ScalaLastOnlyStrategy()):
            cur = ScalaWildcardMinimizer(oracle, model, cur.original_externals, cur, fp, resolutionStrategy=strat).minimize()
        shrunk |= countMsgEvents(cur) < countMsgEvents(intmin)
    assert ambiguous > 0 and left > 0 and cluster_removed and shrunk
