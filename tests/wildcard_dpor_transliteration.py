"""The wildcard minimizer with TestScheduler.DPORwHeuristics, transliterated from the Scala: the reference of
tests/test_wildcard_dpor_cpu.py, tests/test_wildcard_dpor_gpu.py and tests/test_wildcard_dpor_emu_cpu.py.

  DPORwHeuristics.getMatchingMessage for a WildCardMatch head, its backtrackSetter, equivalentTo's case for Unique(_, -1) of an
    external message, getNextMatchingMessage with the ignoreAbsentCallback, stopAfterNextTrace, skipBacktrackComputation,
    start_trace's resetCallback, test()                     (schedulers/DPORwHeuristics.scala:337, 428-449, 474-555, 588-622,
                                                             855-942, 1020-1026, 1142-1185, 1193-1242)
  DPORwHeuristicsUtil.convertToEventTrace / convertToDPORTrace                                     (:1246-1303)
  WildcardMinimizer.testWithDpor, doMinimize's DPOR branch  (minification/wildcard_minimization/WildcardMinimizer.scala:67-114, 190-241)

ScalaWildcardDPOR is ScalaDPORwHeuristics (tests/test_dpor_scheduler_transliteration_cpu.py) with those; the strategies and the
clusterizers are the ones of tests/test_wildcard_transliteration_cpu.py.  Pinned deviations, asserted where they apply:
  * the time budget is a count: dpor() after interleaving number dpor_budget returns None (0: unbounded; the first always runs);
  * an ignored index with no proposal event behind it (`adjustedTrace.get(i).get` would throw) is dropped and counted;
  * the ext_idx of an external delivery in the converted trace is the Send that enqueued it: equal words from deadLetters to
    one receiver are delivered in send order.
Beside the Scala's own state every interleaving leaves a record in the device's terms (node keys as include/demi_gpu.h defines
them, trace indices): its next trace, verdict, executed trace, ignored positions, the deliveries a wildcard picked and the
alternatives in the order the backtrackSetter was called."""
import ctypes as C
import heapq

import numpy as np

from demi_amd import types as T
from demi_amd.incremental_ddmin import convertToDPORTrace
from demi_amd.schedulers import EventTrace

from .test_dpor_scheduler_transliteration_cpu import SCHEDULER, ScalaDPORwHeuristics, Unique
from .test_random_scheduler_transliteration_cpu import MASK64
from .test_wildcard_transliteration_cpu import ScalaWildcardMinimizer, WildCardMatch


class ProposalUnique(Unique):
    """Unique(MsgEvent(snd, rcv, msg | WildCardMatch), id = -1) of a proposal; rec: the record it stands for."""
    __slots__ = ("rec",)

    def __init__(self, event, rec):
        super().__init__(event, -1)
        self.rec = rec


def proposal_uniques(model, trace, present, wild):
    """testWithDpor's `uniques` (:71-80): the proposal's UniqueMsgEvents only, each with id -1."""
    ev = trace.events
    out = []
    for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]:
        i = int(i)
        if not present[i]:
            continue
        msg = wild[i] if wild[i] is not None else (int(ev["msg_type"][i]), int(ev["p0"][i]), int(ev["p1"][i]))
        out.append(ProposalUnique(("msg", int(ev["snd"][i]), int(ev["rcv"][i]), msg), i))      # (deadLetters is the same number in both)
    return out


class ScalaWildcardDPOR(ScalaDPORwHeuristics):
    """new DPORwHeuristics(prioritizePendingUponDivergence = true, stopIfViolationFound = false, startFromBackTrackPoints =
    false, skipBacktrackComputation = true, stopAfterNextTrace = true, budget) + setMaxMessagesToSchedule + setInitialTrace."""

    def __init__(self, oracle, model, externals, uniques, looking_for, dpor_budget=0):
        super().__init__(oracle, model, externals, depth_bound=0, max_messages=len(uniques), trackHistory=True,
                         prioritizePendingUponDivergence=True)
        # setMaxMessagesToSchedule(uniques.size): 0 is a cap too in the Scala (should_cap_messages = true)
        self.should_cap_messages = True
        self.stopAfterNextTrace, self.skipBacktrackComputation = True, True
        self._initialTrace = list(uniques)
        self.looking_for, self.dpor_budget = looking_for, dpor_budget
        self.origNextTraceSize = 0
        self.records = []
        self.exhausted = self.budget_reached = False
        self.skipped_explored = self.points = 0
        self._keys = {}

    # ------------------------------------------------------------------ the device's terms
    def word_of(self, u):
        _, snd, rcv, (mtype, p0, p1) = u.event
        if self.wide:
            return mtype | (rcv << 5) | (snd << (9 if self.big else 8)) | (p0 << 16) | (p1 << 32)
        return mtype | (rcv << 5) | (snd << 8) | (p0 << 16) | (p1 << 24)

    def key_of(self, u):
        k = self._keys.get(u)
        if k is None:
            if u.event[0] == "root":
                k = T.DPOR_ROOT_KEY
            elif u.event[0] == "wq":
                k = T.dpor_marker_key(u.id - 100000)
            else:
                k = ((self.key_of(self.parentOf[u]) ^ self.word_of(u)) * T.DPOR_PRIME) & MASK64
            self._keys[u] = k
        return k

    def _period(self, u):
        if u.event[0] == "wq":
            return u.id - 100000 + 1
        p = self.quiescentPeriod[u]
        return p - 100000 + 1 if p else 0

    def trace_entries(self, trace):
        out = np.zeros(len(trace), dtype=T.DPOR_TRACE_DTYPE)
        for i, u in enumerate(trace):
            kind = {"root": 0, "msg": 1, "wq": 2}[u.event[0]]
            out[i] = (self.key_of(u), self.word_of(u) & 0xFFFFFFFF if kind == 1 else 0,
                      trace.index(self.parentOf[u]) if u in self.parentOf else 0, self._period(u), len(self.pathToRoot(u)) - 1, kind)
        return out

    # ------------------------------------------------------------------ :994-1018
    def getCommonPrefix(self, earlier, later):
        laterPath = list(reversed(self.pathToRoot(later)))
        earlierPath = set(self.pathToRoot(earlier))
        return [x for x in laterPath if x in earlierPath]

    def isExternal(self, u):
        return u.event[1] == self.DEAD and self.model.msg_class[u.event[3][0]] == T.MSG_EXTERNAL

    # ------------------------------------------------------------------ :474-537
    def getMatchingMessage(self):
        u = self.getNextTraceMessage()
        if u is None:
            return None
        if u.event[0] == "msg" and isinstance(u.event[3], WildCardMatch):
            _, snd, rcv, wc = u.event
            if rcv in self.blockedActors:
                return None
            queue = self.pendingEvents.get((snd, rcv))
            if queue is None:
                return None
            pending = list(queue)                         # queue.toIndexedSeq: ALL pending messages, in send order
            pos = self._expecting_idx

            def backtrackSetter(idx):
                priorEvent = self.currentTrace[-1]
                toPlayNext = pending[idx]
                commonPrefix = self.getCommonPrefix(priorEvent, toPlayNext)
                branchI = self.currentTrace.index(commonPrefix[-1])
                traceToPlayNext = self.currentTrace[1:] + [toPlayNext] + list(self.nextTrace)
                heapq.heappush(self.backTrack, (-branchI, self.seq, (priorEvent, toPlayNext), traceToPlayNext))
                self.seq += 1
                self.points += 1
                self._rec["alts"].append((self.key_of(toPlayNext), self.word_of(toPlayNext) & 0xFFFFFFFF, len(self.currentTrace), pos,
                                          self.currentTrace.index(self.parentOf[toPlayNext])))
                self._rec["branches"].append(branchI)

            idx = wc.msgSelector([p.event[3] for p in pending], backtrackSetter)
            if idx is None:
                return None
            found = pending[idx]
            priorEvent = self.currentTrace[-1]
            self.setExplored(len(self.currentTrace) - 1, (priorEvent, found))
            self._rec["wild"].append(len(self.currentTrace))
            self._picked = found
            queue.pop(next(i for i, o in enumerate(queue) if o is found))
            return found
        if u.event[0] == "msg":
            _, snd, rcv, _m = u.event
            if rcv in self.blockedActors:
                return None
            q = self.pendingEvents.get((snd, rcv))
            if q is None:
                return None
            for i, other in enumerate(q):                 # dequeueFirst(equivalentTo(u, _))
                if u.id == -1 and self.isExternal(u) and self.isExternal(other):
                    if other.event[3] == u.event[3]:      # rcv1 == rcv2 && fingerprint(msg1) == fingerprint(msg2)
                        return q.pop(i)
                elif other.id == u.id:                    # (id1 = -1 never equals a graph id: an exact internal delivery never matches)
                    return q.pop(i)
            return None
        q = self.pendingEvents.get((SCHEDULER, SCHEDULER))
        if q is None:
            return None
        for i, other in enumerate(q):
            if other.id == u.id:
                return q.pop(i)
        return None

    # ------------------------------------------------------------------ :542-648
    def getNextMatchingMessage(self):
        foundMatching = None
        while self.nextTrace and foundMatching is None:
            self._expecting_idx = self.origNextTraceSize - len(self.nextTrace)
            foundMatching = self.getMatchingMessage()
            if foundMatching is None:
                self._rec["ignored"].add(self._expecting_idx)           # ignoreAbsentCallback(idx)
        return foundMatching

    def schedule_new_message(self):
        while True:
            self.messagesScheduledSoFar += 1
            if self.should_cap_messages and self.messagesScheduledSoFar > self.max_messages:
                return None
            if self.stopAfterNextTrace and not self.nextTrace:
                return None
            self._picked = None
            if not self.awaitingQuiescence:
                assert self.prioritizePendingUponDivergence
                result = self.getNextMatchingMessage()
                if result is None:
                    result = None if (self.stopAfterNextTrace and not self.nextTrace) else self.getPendingEvent()
            else:
                result = self.getPendingEvent()
            if result is None:
                return None
            if result.event[0] == "msg":
                _, snd, rcv, _m = result.event
                if snd in self.isolatedActors or rcv in self.isolatedActors:
                    assert self._picked is None, "a wildcard picked a message of an actor that is not started: not restated on the device"
                    if snd == rcv:
                        raise RuntimeError("self message without prior messages!")
                    continue
                self.currentTrace.append(result)
                self.setParentEvent(result)
                return result
            self.awaitingQuiescence = True
            self.nextQuiescentPeriod = result.id
            self.quiescentMarker = result

    # ------------------------------------------------------------------ :1020-1185 with skipBacktrackComputation
    def dpor(self, trace):
        if self.dpor_budget and len(self.records) >= self.dpor_budget:       # PIN: the stop watch is a count of interleavings
            self.budget_reached = True
            return None
        while True:                                                          # getNext
            if not self.backTrack:
                self.exhausted = True
                return None
            negI, _s, (e1, e2), replayThis = heapq.heappop(self.backTrack)
            if self.isExplored((e1, e2)):
                self.skipped_explored += 1
                continue
            self.setExplored(-negI, (e1, e2))
            return list(replayThis)                                          # (:1177-1178: replayThis alone)

    # ------------------------------------------------------------------ :1193-1242 around run() / notify_quiescence
    def test(self):
        """Some(currentTrace) as a list of Uniques, or None."""
        self.nextTrace = list(self._initialTrace)
        self.origNextTraceSize = len(self.nextTrace)
        while True:
            self._rec = {"next": list(self.nextTrace), "ignored": set(), "wild": [], "alts": [], "branches": []}
            self.start_trace()                                               # (resetCallback: the ignored set starts empty)
            while True:
                nxt = self.schedule_new_message()
                if nxt is not None:
                    self.dispatch(nxt)
                    continue
                if self.awaitingQuiescence:
                    self.awaitingQuiescence = False
                    self.currentQuiescentPeriod = self.nextQuiescentPeriod
                    self.nextQuiescentPeriod = 0
                    marker = self.maybeAddGraphNode(self.quiescentMarker)
                    self.currentTrace.append(marker)
                    self.currentRoot = marker
                    self.setParentEvent(marker)
                    self.quiescentMarker = None
                    self.runExternal()
                    continue
                break
            states = (C.c_uint64 * (self.model.n_actors * self.stw))(*[w for st_ in self.state for w in st_])
            fp = int(self.oracle.lib().orc_invariant(C.byref(self.ms), states, (1 << self.model.n_actors) - 1))
            if self.looking_for is None:                  # (any violation counts: looking_for_valid = 0)
                found = fp
            else:
                found = self.looking_for if fp and ((fp ^ self.looking_for) & self.model.fp_match_mask) == 0 else 0
            h = 0xCBF29CE484222325
            for w in self.deliveries:
                h = ((h ^ w) * 0x100000001B3) & MASK64
            for a in range(self.model.n_actors):
                for w in self.state[a]:
                    h = ((h ^ w) * 0x100000001B3) & MASK64
            capped = self.messagesScheduledSoFar > self.max_messages
            flags = (T.V_VIOLATION if found else 0) | (T.V_MAXMSG if capped else 0) | min(len(self.deliveries), 0xFFFF) << 16
            self._rec["verdict"] = (flags, found, h)
            self._rec["trace"] = self.trace_entries(self.currentTrace)
            self._rec["uniques"] = list(self.currentTrace)
            self.records.append(self._rec)
            if found:
                return list(self.currentTrace)
            nxt = self.dpor(list(self.currentTrace))
            if nxt is None:
                return None
            self.nextTrace = nxt
            self.origNextTraceSize = len(nxt)


def next_trace_entries(dpor, next_trace, selector_of_rec):
    """A next trace in the device's terms (DPOR_TRACE_DTYPE; include/demi_gpu.h): selector_of_rec(rec) = (type set, policy,
    backtrack mode) of the wildcard that stands for record `rec`."""
    out = np.zeros(len(next_trace), dtype=T.DPOR_TRACE_DTYPE)
    for i, u in enumerate(next_trace):
        if isinstance(u, ProposalUnique):
            _, snd, rcv, m = u.event
            sr = (rcv << 5) | (snd << 8)
            if isinstance(m, WildCardMatch):
                out[i] = (T.wildcard_selector_key(*selector_of_rec(u.rec)), sr, 0, 0, 0, T.DPOR_KIND_WILDCARD)
            else:
                w = dpor.word_of(u)
                out[i] = (w, w & 0xFFFFFFFF, 0, 0, 0, T.DPOR_KIND_EXACT_WORD)
        else:
            kind = {"root": 0, "msg": 1, "wq": 2}[u.event[0]]
            out[i] = (dpor.key_of(u), dpor.word_of(u) & 0xFFFFFFFF if kind == 1 else 0, 0, 0, 0, kind)
    return out


def convertToEventTrace(dpor, trace, mcs):
    """DPORwHeuristicsUtil.convertToEventTrace (:1246-1268): a SpawnEvent per Start, then UniqueMsgSend + UniqueMsgEvent per
    Unique(MsgEvent) that is not the root; ids renumbered in order of appearance (the library's convention for an executed
    trace).  PIN: an external delivery's ext_idx is the Send that enqueued it - equal words in send order."""
    model = dpor.model
    dl = T.DEADLETTERS_BIG if model.n_actors > T.MAX_ACTORS else T.DEADLETTERS
    out = []
    for i, e in enumerate(mcs):               # (indices into the minimizer's externals; convertToDPORTrace keeps Start and Send)
        if int(e["kind"]) == T.EV_START:
            out.append((T.REC_SPAWN, 0, int(e["a"]), 0, 0, 0, 0, i, 0, 0))
    sends = {}
    for i, e in enumerate(mcs):
        if int(e["kind"]) == T.EV_SEND:
            sends.setdefault((int(e["a"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"])), []).append(i)
    n = 0
    for u in trace:
        if u.event[0] != "msg":
            continue
        _, snd, rcv, (mtype, p0, p1) = u.event
        n += 1
        dead = snd == dpor.DEAD
        external = dead and model.msg_class[mtype] == T.MSG_EXTERNAL
        ext_idx = sends[(rcv, mtype, p0, p1)].pop(0) if external else 255
        s = dl if dead else snd
        out.append((T.REC_MSG_SEND, s, rcv, mtype, p0, p1, 1 if external else 2 if dead else 0, ext_idx, 0, n))
        out.append((T.REC_MSG_EVENT, s, rcv, mtype, p0, p1, 0, 255, 0, n))
    return np.array(out, dtype=T.REC_EVENT_DTYPE) if out else np.zeros(0, dtype=T.REC_EVENT_DTYPE)


class ScalaWildcardDporMinimizer(ScalaWildcardMinimizer):
    """WildcardMinimizer(testScheduler = TestScheduler.DPORwHeuristics)."""

    def __init__(self, *a, dpor_budget=256, **kw):
        super().__init__(*a, **kw)
        self.dpor_budget = dpor_budget
        self.interleavings = 0            # start_trace calls over all proposals
        self.backtracked_hits = 0         # proposals that reproduced in an interleaving other than their first
        self.multi_point_interleavings = 0
        self.emptied = self.cut_by_budget = self.skipped_explored = 0
        self.dropped_ignored = 0          # PIN: ignored indices with no proposal event behind them
        self.tests = []                   # per proposal: the ScalaWildcardDPOR

    def testWithDpor(self, startTrace, present, wild):
        self.total_replays += 1                         # stats.increment_replays (DPORwHeuristics.test counts one per call)
        uniques = proposal_uniques(self.model, startTrace, present, wild)
        externals = convertToDPORTrace(self.mcs, ignoreQuiescence=False)
        d = ScalaWildcardDPOR(self.oracle, self.model, externals, uniques, self.violation.code, dpor_budget=self.dpor_budget)
        hit = d.test()
        self.tests.append(d)
        self.interleavings += len(d.records)
        self.multi_point_interleavings += sum(1 for r in d.records if len(r["alts"]) >= 2)
        self.emptied += int(d.exhausted)
        self.cut_by_budget += int(d.budget_reached)
        self.skipped_explored += d.skipped_explored
        if hit is None:
            return None, set()
        if len(d.records) > 1:
            self.backtracked_hits += 1
        return EventTrace(convertToEventTrace(d, hit, self.mcs), self.mcs), set(d.records[-1]["ignored"])

    def doMinimize(self, clusterizer, startTrace):
        minTrace = startTrace
        ev = startTrace.events
        nextTrace = clusterizer.getNextTrace(False, set())
        while nextTrace is not None:
            present, wild = nextTrace
            self.proposals.append(present)
            ret, ignoredAbsentIndices = self.testWithDpor(startTrace, present, wild)
            ignoredAbsentIds = set()
            if ret is not None:
                self.successes += 1
                if len(ret.events) <= len(minTrace.events):
                    minTrace = ret
                # adjustedTrace: the proposal's UniqueMsgEvents (:227-235); after a backtracked hit the indices are positions
                # in the hitting interleaving's own next trace - reproduced as written
                adjusted = [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0] if present[int(i)]]
                for i in ignoredAbsentIndices:
                    if i < len(adjusted):
                        ignoredAbsentIds.add(int(ev["id"][adjusted[i]]))
                    else:
                        self.dropped_ignored += 1         # PIN: `.get(i).get` would throw
            nextTrace = clusterizer.getNextTrace(ret is not None, ignoredAbsentIds)
        return minTrace
