"""Wildcard (fungible-clock) internal minimization: which deliveries can go once the others only have to match by type.

Host-side mirror of minification/wildcard_minimization/{AmbiguityResolutionStrategies, Clusterizer, OneAtATimeClusterizer,
ClockClusterizer, WildcardMinimizer}.scala with TestScheduler.STSSched (backtrack setters are no-ops).  A Clusterizer proposes
traces over the SAME original trace: deliveries of external messages stay exact, every other kept delivery becomes
MsgEvent(snd, rcv, WildCardMatch(selector)), a delivery outside the current cluster is dropped (its MsgSend stays).  On the
device (demi_replay_wildcard_*, csrc/k2_wildcard.hpp) a selector is (set of message types, policy HEAD / FIRST / LAST) and a
proposal is a presence bitmask over the recorded events, so one load serves a whole doMinimize.  The replays are launches:
the clusterizer is cloned, its upcoming proposals are enumerated assuming each fails, evaluated together, and consumed up to
the first that still triggers the violation - exactly the sequence WildcardMinimizer.doMinimize walks one replay at a time
(max_batch = 1 is that loop; every batch size gives the same result and the same stats.total_replays).

A delivery's id is the Uniq id of its UniqueMsgEvent (the `id` of the record); `sorted` sequences are sorted by it, as in the
Scala.  BeginUnignorableEvents blocks do not exist in the recorded format.  The logical-clock hooks of MessageFingerprinter are
the model's clock_increment_types / clock_field (model.py); a model without them makes ClockClusterizer degenerate as the
default fingerprinter does in the reference (no clock clusters, no timers).
"""
from typing import Dict, FrozenSet, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import _native
from . import types as T
from .capacity import aborted, decide_batch, decide_one
from .internal_minimization import countMsgEvents
from .model import Model
from .schedulers import EventTrace, MinimizationStats, SchedulerConfig, ViolationFingerprint


# ------------------------------------------------------------------ AmbiguityResolutionStrategies.scala
class AmbiguityResolutionStrategy:
    """resolve(msgSelector, pending, backtrackSetter) -> index of the selected pending message, or None.  `policy` is what the
    device knows the strategy as."""
    policy = T.WILDCARD_FIRST
    backtrack = T.WILDCARD_BACKTRACK_NONE      # which alternatives it hands to the backtrackSetter (DPORwHeuristics only)

    def resolve(self, msgSelector, pending: Sequence, backtrackSetter=None) -> Optional[int]:
        matching = [i for i, m in enumerate(pending) if msgSelector(m)]
        return matching[0] if matching else None


class SrcDstFIFOOnly(AmbiguityResolutionStrategy):
    """:18-34: if the first pending message doesn't match, give up."""
    policy = T.WILDCARD_HEAD

    def resolve(self, msgSelector, pending, backtrackSetter=None):
        return 0 if len(pending) and msgSelector(pending[0]) else None


class BackTrackStrategy(AmbiguityResolutionStrategy):
    """:45-77: the first match (the backtrack points it sets are no-ops under STSSched; under DPORwHeuristics: one per later
    match of another message value, youngest first)."""
    backtrack = T.WILDCARD_BACKTRACK_ALL


class FirstAndLastBacktrack(AmbiguityResolutionStrategy):
    """:80-107: the first match (under DPORwHeuristics: one backtrack point, for the youngest match of another message value)."""
    backtrack = T.WILDCARD_BACKTRACK_LAST_DISTINCT


class LastOnlyStrategy(AmbiguityResolutionStrategy):
    """:109-117: the last match."""
    policy = T.WILDCARD_LAST

    def resolve(self, msgSelector, pending, backtrackSetter=None):
        matching = [i for i, m in enumerate(pending) if msgSelector(m)]
        return matching[-1] if matching else None


# ------------------------------------------------------------------ the trace as the clusterizers see it
class _Deliveries:
    """The UniqueMsgEvents of a trace: record index, Uniq id, message type, payload fields, external or not."""

    def __init__(self, trace: EventTrace, model: Model):
        ev = trace.events
        self.n_rec = len(ev)
        self.idx = [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]]
        self.ids = [int(ev["id"][i]) for i in self.idx]
        assert len(set(self.ids)) == len(self.ids), "Must be UniqueMsgEvent: ids of the deliveries are not unique"
        self.types = [int(ev["msg_type"][i]) for i in self.idx]
        self.external = [model.msg_class[t] == T.MSG_EXTERNAL for t in self.types]      # EventTypes.isExternal
        self.rec_of_id = dict(zip(self.ids, self.idx))
        self.clock_inc = [t in model.clock_increment_types for t in self.types]       # causesClockIncrement
        self.clock: List[Optional[int]] = []                                           # getLogicalClock
        for i, t in zip(self.idx, self.types):
            k = model.clock_field.get(t)
            area = int(ev["p0"][i]) | int(ev["p1"][i]) << 16 | int(ev["p_hi"][i]) << 32
            self.clock.append(None if k is None else int(T.payload_fields(area, model.payloads)[k]))

    def present(self, include: Set[int]) -> np.ndarray:
        """bool[n_rec]: the trace that holds the external deliveries and the deliveries whose id is in `include`."""
        p = np.zeros(self.n_rec, dtype=bool)
        for i, d, x in zip(self.idx, self.ids, self.external):
            p[i] = x or d in include
        return p


class Clusterizer:
    """Clusterizer.scala.  getNextTrace returns the presence mask (bool[n_rec]) of the next trace, or None."""
    approximateIterations = 0

    def getNextTrace(self, violationReproducedLastRun: bool, ignoredAbsentIds: Set[int]) -> Optional[np.ndarray]:
        raise NotImplementedError

    def selectors(self) -> Tuple[np.ndarray, np.ndarray]:
        """(type_sets uint32[n_rec], policies uint8[n_rec]) of the trace's records: what a kept delivery is wildcarded to."""
        raise NotImplementedError

    def backtracks(self) -> np.ndarray:
        """uint8[n_rec]: the demi_wildcard_backtrack of every record's wildcard (the resolution strategy's; the timer wildcard
        of ClockClusterizer sets none)."""
        ts, _ = self.selectors()
        bt = np.where(ts != 0, self.resolutionStrategy.backtrack, T.WILDCARD_BACKTRACK_NONE).astype(np.uint8)
        for i, inc, x in zip(self.d.idx, self.d.clock_inc, self.d.external):
            if inc and not x and isinstance(self, ClockClusterizer):
                bt[i] = T.WILDCARD_BACKTRACK_NONE
        return bt

    def clone(self) -> "Clusterizer":
        import copy
        c = copy.copy(self)
        for k, v in self.__dict__.items():
            if isinstance(v, (_OneAtATimeIterator, _ClockClusterIterator)):
                setattr(c, k, v.clone())
        return c


class SingletonClusterizer(Clusterizer):
    """OneAtATimeClusterizer.scala: pick an event to remove, wildcard all the others."""

    def __init__(self, originalTrace: EventTrace, model: Model, resolutionStrategy: AmbiguityResolutionStrategy):
        self.d = _Deliveries(originalTrace, model)
        self.resolutionStrategy = resolutionStrategy
        self.sortedIds = sorted(i for i, x in zip(self.d.ids, self.d.external) if not x)        # getIdsToRemove
        self.allIds = frozenset(self.d.ids)                                                    # | getUnignorableIds
        self.successfullyRemoved: FrozenSet[int] = frozenset()
        self.ignoredLastRun = -1
        self.firstRun = True

    @property
    def approximateIterations(self):
        return len(self.allIds)

    def getNextTrace(self, violationReproducedLastRun, ignoredAbsentIds):
        if not self.sortedIds:
            return None
        if violationReproducedLastRun:
            self.successfullyRemoved = (self.successfullyRemoved | frozenset(ignoredAbsentIds)) | {self.ignoredLastRun}
        if not self.firstRun:
            self.ignoredLastRun = self.sortedIds[0]
            self.sortedIds = self.sortedIds[1:]
        else:
            self.firstRun = False
        currentCluster = self.allIds - (self.successfullyRemoved - {self.ignoredLastRun})
        return self.d.present(currentCluster)

    def selectors(self):
        ts = np.zeros(self.d.n_rec, dtype=np.uint32)
        po = np.zeros(self.d.n_rec, dtype=np.uint8)
        for i, t, x in zip(self.d.idx, self.d.types, self.d.external):
            if not x:
                ts[i] = 1 << t                              # the class tag
                po[i] = self.resolutionStrategy.policy
        return ts, po


class Aggressiveness:
    """ClockClusterizer.scala:12-21."""
    NONE, ALL_TIMERS_FIRST_ITR, STOP_IMMEDIATELY = 0, 1, 2


class _ClockClusterIterator:
    """ClockClusterIterator (ClockClusterizer.scala:138-228): the first iteration includes all events."""

    def __init__(self, d: _Deliveries):
        self.d = d
        self.allIds = frozenset(i for i, inc, c in zip(d.ids, d.clock_inc, d.clock) if not inc and c is not None)
        self.firstClusterRemoval = True
        self.nextClockToRemove = -1
        self.blacklist: FrozenSet[int] = frozenset()
        self.clocks: List[int] = []
        self.clocks = self.computeRemainingClocks()

    def clone(self):
        import copy
        c = copy.copy(self)
        c.clocks = list(self.clocks)
        return c

    def computeRemainingClocks(self) -> List[int]:
        lowest = self.clocks[0] if self.clocks else 0
        vals = {c for i, c in zip(self.d.ids, self.d.clock) if i not in self.blacklist and c is not None}
        return [c for c in sorted(vals) if c >= lowest]

    def _current(self) -> FrozenSet[int]:
        currentClockToRemove = -1 if self.firstClusterRemoval else self.nextClockToRemove
        out = set()
        for i, inc, c in zip(self.d.ids, self.d.clock_inc, self.d.clock):
            if inc:
                continue                                    # handled by OneAtATimeIterator
            if c is None or not (c == currentClockToRemove or i in self.blacklist):
                out.add(i)
        return frozenset(out)

    def next(self) -> FrozenSet[int]:
        if self.firstClusterRemoval:
            ret = self._current()
            self.firstClusterRemoval = False
            return ret
        self.nextClockToRemove = self.clocks[0]
        ret = self._current()
        self.clocks = self.clocks[1:]
        return ret

    def hasNext(self) -> bool:
        return self.firstClusterRemoval or bool(self.clocks)

    def producedViolation(self, previouslyIncluded, ignoredAbsents):
        self.blacklist = self.blacklist | self.inverse(previouslyIncluded)
        if ignoredAbsents:
            self.blacklist = self.blacklist | (self.allIds & frozenset(ignoredAbsents))
            self.clocks = self.computeRemainingClocks()

    def inverse(self, toInclude):
        return self.allIds - frozenset(toInclude)


class _OneAtATimeIterator:
    """OneAtATimeIterator (ClockClusterizer.scala:230-290): all timers, then all but the first, all but the second, ..."""

    def __init__(self, all_ids):
        self.all = frozenset(all_ids)
        self.toRemove = sorted(self.all)
        self.first = True
        self.blacklist: FrozenSet[int] = frozenset()

    def clone(self):
        import copy
        c = copy.copy(self)
        c.toRemove = list(self.toRemove)
        return c

    def _current(self):
        if self.first:
            return self.all - self.blacklist
        return (self.all - {self.toRemove[0]}) - self.blacklist

    def next(self):
        if self.first:
            ret = self._current()
            self.first = False
            return ret
        ret = self._current()
        self.toRemove = self.toRemove[1:]
        return ret

    def hasNext(self):
        return self.first or bool(self.toRemove)

    def producedViolation(self, previouslyIncluded, ignoredAbsents):
        self.blacklist = self.blacklist | self.inverse(previouslyIncluded) | (self.all & frozenset(ignoredAbsents))

    def reset(self):
        self.toRemove = sorted(self.all - self.blacklist)
        self.first = True

    def inverse(self, toInclude):
        return self.all - frozenset(toInclude)


class ClockClusterizer(Clusterizer):
    """ClockClusterizer.scala:23-135: cluster the deliveries by their logical clock, and for every cluster try the timers
    (the messages that cause a clock increment) one at a time."""

    def __init__(self, originalTrace: EventTrace, model: Model, resolutionStrategy: AmbiguityResolutionStrategy,
                 aggressiveness: int = Aggressiveness.ALL_TIMERS_FIRST_ITR, skipClockClusters: bool = False):
        self.d = _Deliveries(originalTrace, model)
        self.model = model
        self.resolutionStrategy = resolutionStrategy
        self.aggressiveness = aggressiveness
        self.skipClockClusters = skipClockClusters
        self.clusterIterator = _ClockClusterIterator(self.d)
        assert self.clusterIterator.hasNext()
        self.currentCluster = self.clusterIterator.next()         # start by not removing any clusters
        self.tryingFirstCluster = True
        self.timerIterator = _OneAtATimeIterator(i for i, inc in zip(self.d.ids, self.d.clock_inc) if inc)
        self.currentTimers: FrozenSet[int] = frozenset()

    @property
    def approximateIterations(self):
        if self.skipClockClusters:
            return len(self.timerIterator.toRemove)
        return len(self.clusterIterator.clocks) * len(self.timerIterator.toRemove)

    def getNextTrace(self, violationReproducedLastRun, ignoredAbsentIds):
        if violationReproducedLastRun:
            self.timerIterator.producedViolation(self.currentTimers, ignoredAbsentIds)
            self.clusterIterator.producedViolation(self.currentCluster, ignoredAbsentIds)
        if (not self.timerIterator.hasNext() or
                (self.aggressiveness == Aggressiveness.ALL_TIMERS_FIRST_ITR and violationReproducedLastRun
                 and not self.tryingFirstCluster) or
                (self.aggressiveness == Aggressiveness.STOP_IMMEDIATELY and violationReproducedLastRun)):
            self.tryingFirstCluster = False
            if not self.clusterIterator.hasNext() or self.skipClockClusters:
                return None
            self.timerIterator.reset()
            self.currentCluster = self.clusterIterator.next()
        assert self.timerIterator.hasNext()
        self.currentTimers = self.timerIterator.next()
        return self.d.present(self.currentTimers | self.currentCluster)

    def selectors(self):
        ts = np.zeros(self.d.n_rec, dtype=np.uint32)
        po = np.zeros(self.d.n_rec, dtype=np.uint8)
        inc_set = sum(1 << t for t in self.model.clock_increment_types)
        for i, t, x, inc in zip(self.d.idx, self.d.types, self.d.external, self.d.clock_inc):
            if x:
                continue
            if inc:                 # timers bypass the resolutionStrategy: lst.indexWhere(causesClockIncrement)
                ts[i], po[i] = inc_set, T.WILDCARD_FIRST
            else:
                ts[i], po[i] = 1 << t, self.resolutionStrategy.policy
        return ts, po


# ------------------------------------------------------------------ the replay oracle on the GPU
class StsWildcardOracle:
    """RunnerUtils.testWithStsSched (RunnerUtils.scala:913-943) for the traces a Clusterizer proposes: K2 with wildcard
    deliveries (demi_replay_wildcard_*).  `trace.original_externals` is the MCS: every external is kept."""

    def __init__(self, schedulerConfig: SchedulerConfig, device: int = 0, p_max: int = 64):
        if schedulerConfig.model is None or schedulerConfig.model.inv_kind == T.INV_NONE:
            raise ValueError("Must invoke setInvariant before test()")
        if int(schedulerConfig.filterKnownAbsents):
            raise ValueError("the wildcard replay is built for filterKnownAbsents = false only")
        self.schedulerConfig = schedulerConfig
        self.p_max = p_max
        self._ctx = _native.Context(device)
        self._ctx.model_load(schedulerConfig.model.to_struct())
        if getattr(schedulerConfig.model, "compiled_only", False):
            self._ctx.model_specialize()
        self._trace = None
        self.launches = 0
        self.batches: List[int] = []

    def _limits(self, fp: ViolationFingerprint, p_max=None) -> T.Limits:
        return T.Limits(0, 0, p_max or self.p_max, 1, fp.code, 1 if self.schedulerConfig.populate_all_actors else 0, 0, 0)

    def load(self, trace: EventTrace, type_sets, policies):
        self._ctx.replay_load(trace.original_externals, trace.events)
        self._ctx.replay_wildcard_load(type_sets, policies)
        self._trace = trace

    def _counted(self, launch):               # `launch` with every call of it counted
        def run(*args):
            self.launches += 1
            return launch(*args)
        return run

    def test_batch(self, presents: Sequence[np.ndarray], violation: ViolationFingerprint, masks=None) -> List[bool]:
        """masks (uint64[n, 4], optional): the subsequence of the LOADED externals every candidate keeps - the trace stays
        loaded with its own externals, so that the records' ext_idx stay aligned."""
        presents = np.asarray(presents, dtype=bool).reshape(len(presents), -1)
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        self.batches.append(len(presents))
        sub = lambda a, idx: a if a is None or idx is None else a[idx]
        v, _ = decide_batch(self._counted(lambda l, idx: self._ctx.replay_wildcard_batch(sub(presents, idx), l, masks=sub(masks, idx))),
                            self._limits(violation), aborted, "a wildcard candidate's replay exceeds the engine's capacities")
        return [bool(f & T.V_VIOLATION) for f in v["flags"]]

    def test_candidates(self, masks, drops, violation: ViolationFingerprint, base_present=None) -> np.ndarray:
        """One WildcardTestOracle.test per row of masks (demi_replay_wildcard_candidates): WILDCARD_CANDIDATE_DTYPE records.
        A candidate that is unknown because of a capacity is evaluated again with the largest pending set."""
        masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        self.batches.append(len(masks))
        r, again = decide_batch(self._counted(lambda l, idx: self._ctx.replay_wildcard_candidates(masks if idx is None else masks[idx], drops, l,
                                                                                                  base_present=base_present)),
                                self._limits(violation), lambda r: (r["flags"] & T.WC_UNKNOWN) != 0,
                                "a wildcard candidate's proposal exceeds the engine's capacities")
        if again:
            self.retried = getattr(self, "retried", 0) + again
        return r

    def executed(self, present: np.ndarray, violation: ViolationFingerprint, mask=None):
        """test() of one candidate: (executed trace, record indices of the present deliveries that were ignored as absent)
        iff it triggers the violation, else None.  mask: as in test_batch."""
        v, kept, rec = decide_one(self._counted(lambda l: self._ctx.replay_wildcard_get_trace(present, l, mask=mask)), self._limits(violation))
        if not (int(v.flags) & T.V_VIOLATION):
            return None
        ev = self._trace.events
        ignored = {int(i) for i in np.nonzero((ev["kind"] == T.REC_MSG_EVENT) & np.asarray(present, dtype=bool) & (kept == 0))[0]}
        return EventTrace(rec, self._trace.original_externals, self._trace.ext_areas), ignored

    def minimize_native(self, mcs: np.ndarray, trace: EventTrace, violation: ViolationFingerprint, clusteringStrategy: str,
                        resolutionStrategy: AmbiguityResolutionStrategy, skipClockClusters: bool = False,
                        stats: Optional[MinimizationStats] = None, max_batch: int = 1 << 14) -> Tuple[MinimizationStats, EventTrace]:
        """WildcardMinimizer(...).minimize() as one call of the library (demi_minimize_wildcards).  Of `resolutionStrategy` only
        the policy is used; the clock hooks are the model's.  The library lowers the selectors itself."""
        codes = {ClusteringStrategy.ClockClusterizer: T.CLUSTER_CLOCK, ClusteringStrategy.SingletonClusterizer: T.CLUSTER_SINGLETON,
                 ClusteringStrategy.ClockThenSingleton: T.CLUSTER_CLOCK_THEN_SINGLETON}
        if clusteringStrategy not in codes:
            raise ValueError("unknown clustering strategy %r" % (clusteringStrategy,))
        model = self.schedulerConfig.model
        stats = stats or MinimizationStats()
        areas = trace.ext_areas if trace.ext_areas is not None and len(trace.ext_areas) == len(mcs) else None
        self._ctx.replay_load(mcs, trace.events)
        self._trace = None            # the call replaces the context's loaded execution (also when it raises)
        par = T.WcminParams(codes[clusteringStrategy], resolutionStrategy.policy, skipClockClusters, max(1, int(max_batch)),
                            model.clock_increment_types, model.clock_field)
        events, sizes, batches, st = self._ctx.minimize_wildcards(self._limits(violation), par)
        stats.increment_replays(int(st.total_replays))
        self.launches += int(st.launches)
        self.batches.extend(batches)
        self.native_stats, self.native_sizes, self.native_batches = st, sizes, batches
        return stats, EventTrace(events, mcs, areas)

    def shutdown(self):
        self._ctx.close()


# ------------------------------------------------------------------ the DPOR oracle on the GPU
class TestScheduler:
    """WildcardMinimizer.scala's TestScheduler enumeration."""
    STSSched, DPORwHeuristics = "STSSched", "DPORwHeuristics"


def convertToEventTrace(model: Model, trace: np.ndarray, mcs: np.ndarray) -> np.ndarray:
    """DPORwHeuristicsUtil.convertToEventTrace (DPORwHeuristics.scala:1246-1268) of an executed DPOR trace (DPOR_TRACE_DTYPE):
    a Spawn record per Start of `mcs`, then MsgSend + MsgEvent per delivered entry, ids 1, 2, ... in order of appearance.
    Pinned: the ext_idx of an external delivery is the Send that enqueued it - equal words from deadLetters to one receiver are
    delivered in send order.  Tables whose message words fit a trace entry only (not DEMI_MODEL_WIDE)."""
    if model.wide:
        raise ValueError("convertToEventTrace: a trace entry of a DEMI_MODEL_WIDE table does not hold the whole payload area")
    out = []
    sends: Dict[Tuple[int, int, int, int], List[int]] = {}
    for i, e in enumerate(mcs):
        if int(e["kind"]) == T.EV_START:
            out.append((T.REC_SPAWN, 0, int(e["a"]), 0, 0, 0, 0, i, 0, 0))
        elif int(e["kind"]) == T.EV_SEND:
            sends.setdefault((int(e["a"]), int(e["msg_type"]), int(e["p0"]), int(e["p1"])), []).append(i)
    n = 0
    for e in trace:
        if int(e["kind"]) != T.DPOR_KIND_DELIVERY:
            continue
        w = int(e["word"])
        mtype, rcv, snd, p0, p1 = w & 31, (w >> 5) & 7, (w >> 8) & 15, (w >> 16) & 255, w >> 24
        n += 1
        dead = snd == T.DEADLETTERS
        external = dead and model.msg_class[mtype] == T.MSG_EXTERNAL
        ext_idx = sends[(rcv, mtype, p0, p1)].pop(0) if external else 255
        out.append((T.REC_MSG_SEND, snd, rcv, mtype, p0, p1, 1 if external else 2 if dead else 0, ext_idx, 0, n))
        out.append((T.REC_MSG_EVENT, snd, rcv, mtype, p0, p1, 0, 255, 0, n))
    return np.array(out, dtype=T.REC_EVENT_DTYPE) if out else np.zeros(0, dtype=T.REC_EVENT_DTYPE)


class DporWildcardOracle:
    """WildcardMinimizer.testWithDpor (WildcardMinimizer.scala:67-114) for the traces a Clusterizer proposes: one call of
    demi_wildcard_dpor_test per proposal - K3 with wildcard entries (csrc/k3_wildcard.hpp) around the backtrack queue of
    csrc/wcdpor_host.hpp.  A proposal is lowered to its UniqueMsgEvents: a wildcarded delivery to a DPOR_KIND_WILDCARD entry
    (type set, policy, backtrack mode), the exact delivery of an external message to a DPOR_KIND_EXACT_WORD entry.
    dpor_budget: interleavings per proposal (0 = unbounded); batch: queue heads per launch."""

    def __init__(self, schedulerConfig: SchedulerConfig, device: int = 0, p_max: int = 64, dpor_budget: int = 256, batch: int = 64,
                 max_alts: int = 0, specialize: bool = False):
        if schedulerConfig.model is None or schedulerConfig.model.inv_kind == T.INV_NONE:
            raise ValueError("Must invoke setInvariant before test()")
        self.schedulerConfig = schedulerConfig
        self.p_max, self.dpor_budget, self.batch, self.max_alts = p_max, dpor_budget, max(1, int(batch)), max_alts
        self._ctx = _native.Context(device)
        self._ctx.model_load(schedulerConfig.model.to_struct())
        if specialize or getattr(schedulerConfig.model, "compiled_only", False):
            self._ctx.model_specialize()
        self._trace = None
        self.launches = self.interleavings = self.speculated = 0
        self.results: List[T.WcdporResult] = []

    def load(self, trace: EventTrace, type_sets, policies, backtracks):
        from .incremental_ddmin import _dpor_trace_indices, convertToDPORTrace
        mcs = trace.original_externals
        areas = None
        if trace.ext_areas is not None and len(trace.ext_areas) == len(mcs):
            areas = np.asarray(trace.ext_areas)[_dpor_trace_indices(mcs, False)]
        self._ctx.dpor_load(convertToDPORTrace(mcs, ignoreQuiescence=False), areas=areas)
        self._trace = trace
        self._sel = (np.asarray(type_sets, dtype=np.uint32), np.asarray(policies, dtype=np.uint8), np.asarray(backtracks, dtype=np.uint8))

    def present_records(self, present) -> List[int]:
        """The proposal's UniqueMsgEvents, as record indices (what an ignored index counts in, WildcardMinimizer.scala:227-235)."""
        ev = self._trace.events
        return [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0] if present[int(i)]]

    def lower(self, present) -> np.ndarray:
        ev = self._trace.events
        model = self.schedulerConfig.model
        ts, po, bt = self._sel
        recs = self.present_records(present)
        out = np.zeros(len(recs), dtype=T.DPOR_TRACE_DTYPE)
        for k, i in enumerate(recs):
            snd, rcv = int(ev["snd"][i]), int(ev["rcv"][i])
            if int(ts[i]):
                out[k] = (T.wildcard_selector_key(ts[i], po[i], bt[i]), (rcv << 5) | (snd << 8), 0, 0, 0, T.DPOR_KIND_WILDCARD)
            else:
                area = int(ev["p0"][i]) | int(ev["p1"][i]) << 16 | int(ev["p_hi"][i]) << 32
                head = int(ev["msg_type"][i]) | (rcv << 5) | (snd << 8)
                w = head | area << 16 if model.wide else head | int(ev["p0"][i]) << 16 | int(ev["p1"][i]) << 24
                out[k] = (w, w & 0xFFFFFFFF, 0, 0, 0, T.DPOR_KIND_EXACT_WORD)
        return out

    def test_raw(self, present, violation: ViolationFingerprint, dpor_budget=None, batch=None):
        """(the hit's executed DPOR trace or None, its ignored positions, WcdporResult)."""
        init = self.lower(present)
        par = T.DporParams(0, len(init), 1, violation.code, self.p_max, 0, 1)
        trace, ignored, res = self._ctx.wildcard_dpor_test(init, par, dpor_budget=self.dpor_budget if dpor_budget is None else dpor_budget,
                                                           batch=self.batch if batch is None else batch, max_alts=self.max_alts)
        self.launches += int(res.launches)
        self.interleavings += int(res.interleavings)
        self.speculated += int(res.speculated)
        self.results.append(res)
        return trace, ignored, res

    def test(self, present, violation: ViolationFingerprint):
        """testWithDpor: (EventTrace, ignored positions) iff an interleaving triggers the violation, else None."""
        trace, ignored, _ = self.test_raw(present, violation)
        if trace is None:
            return None
        mcs = self._trace.original_externals
        return EventTrace(convertToEventTrace(self.schedulerConfig.model, trace, mcs), mcs, self._trace.ext_areas), ignored

    def shutdown(self):
        self._ctx.close()


# ------------------------------------------------------------------ WildcardMinimizer.scala
class ClusteringStrategy:
    ClockClusterizer, SingletonClusterizer, ClockThenSingleton = "ClockClusterizer", "SingletonClusterizer", "ClockThenSingleton"


class WildcardMinimizer:
    """WildcardMinimizer.scala:44-242 with TestScheduler.STSSched.  `oracle`: a StsWildcardOracle (created, and shut down, here
    when None).  `max_batch` bounds how many of the clusterizer's upcoming proposals are replayed per launch.  native: minimize()
    is ONE call of the library (demi_minimize_wildcards: same trace, same stats.total_replays, internal_sizes and batches; the
    oracle must be a StsWildcardOracle)."""

    def __init__(self, schedulerConfig: SchedulerConfig, mcs: np.ndarray, trace: EventTrace, violation: ViolationFingerprint,
                 skipClockClusters: bool = False, resolutionStrategy: Optional[AmbiguityResolutionStrategy] = None,
                 clusteringStrategy: str = ClusteringStrategy.ClockClusterizer, stats: Optional[MinimizationStats] = None,
                 max_batch: int = 1 << 14, oracle=None, device: int = 0, p_max: int = 64, native: bool = False,
                 testScheduler: str = TestScheduler.STSSched, dpor_budget: int = 256, batch: int = 64):
        if testScheduler not in (TestScheduler.STSSched, TestScheduler.DPORwHeuristics):
            raise ValueError("unknown test scheduler %r" % (testScheduler,))
        if testScheduler == TestScheduler.DPORwHeuristics and native:
            raise ValueError("native=True is demi_minimize_wildcards, the STSSched loop: not built for TestScheduler.DPORwHeuristics")
        self.testScheduler, self.dpor_budget, self.batch = testScheduler, dpor_budget, batch
        self.dropped_ignored = 0                       # DPOR branch: ignored indices with no proposal event behind them
        self.schedulerConfig = schedulerConfig
        self.native = native
        self.mcs = mcs
        # (the payload areas of a DEMI_MODEL_PAYLOADS table's externals stay with the trace: `mcs` are its externals)
        self.ext_areas = trace.ext_areas if trace.ext_areas is not None and len(trace.ext_areas) == len(mcs) else None
        self.trace = EventTrace(trace.events, mcs, self.ext_areas)
        self.violation = violation
        self.skipClockClusters = skipClockClusters
        self.resolutionStrategy = resolutionStrategy if resolutionStrategy is not None else BackTrackStrategy()
        self.clusteringStrategy = clusteringStrategy
        self._stats = stats or MinimizationStats()
        self.max_batch = max(1, int(max_batch))
        self.oracle = oracle
        self._device, self._p_max = device, p_max
        self.proposals: List[np.ndarray] = []          # every trace the sequential loop tested, in order (presence masks)
        self.internal_sizes: List[int] = []            # record_internal_size after every (sequential) replay
        self.speculative_replays = 0
        self.batches: List[int] = []

    def minimize(self) -> Tuple[MinimizationStats, EventTrace]:
        model = self.schedulerConfig.model
        aggressiveness = Aggressiveness.STOP_IMMEDIATELY if self.skipClockClusters else Aggressiveness.ALL_TIMERS_FIRST_ITR
        own = self.oracle is None
        dpor = self.testScheduler == TestScheduler.DPORwHeuristics
        if own and dpor:
            self.oracle = DporWildcardOracle(self.schedulerConfig, device=self._device, p_max=self._p_max, dpor_budget=self.dpor_budget,
                                             batch=self.batch)
        elif own:
            self.oracle = StsWildcardOracle(self.schedulerConfig, device=self._device, p_max=self._p_max)
        doMinimize = self.doMinimizeDpor if dpor else self.doMinimize
        try:
            if self.native:
                _, minTrace = self.oracle.minimize_native(self.mcs, self.trace, self.violation, self.clusteringStrategy,
                                                          self.resolutionStrategy, skipClockClusters=self.skipClockClusters,
                                                          stats=self._stats, max_batch=self.max_batch)
                self.internal_sizes.extend(self.oracle.native_sizes)
                self.batches.extend(self.oracle.native_batches)
                self.speculative_replays += sum(self.oracle.native_batches)
                return self._stats, minTrace
            if self.clusteringStrategy in (ClusteringStrategy.ClockClusterizer, ClusteringStrategy.ClockThenSingleton):
                clusterizer = ClockClusterizer(self.trace, model, self.resolutionStrategy, aggressiveness=aggressiveness,
                                               skipClockClusters=self.skipClockClusters)
            else:
                clusterizer = SingletonClusterizer(self.trace, model, self.resolutionStrategy)
            minTrace = doMinimize(clusterizer, self.trace)
            if self.clusteringStrategy == ClusteringStrategy.ClockThenSingleton:
                minTrace = doMinimize(SingletonClusterizer(minTrace, model, self.resolutionStrategy), minTrace)
            if not self.skipClockClusters:
                self.internal_sizes.append(countMsgEvents(minTrace))          # fencepost
            return self._stats, minTrace
        finally:
            if own:
                self.oracle.shutdown()
                self.oracle = None

    def doMinimize(self, clusterizer: Clusterizer, startTrace: EventTrace) -> EventTrace:
        minTrace = startTrace
        d = clusterizer.d
        id_of_rec = {i: k for k, i in d.rec_of_id.items()}
        self.oracle.load(startTrace, *clusterizer.selectors())
        last = (False, frozenset())                     # what the next getNextTrace is told about the last run
        while True:
            # the clusterizer's upcoming proposals, each assuming the one before it failed
            spec = clusterizer.clone()
            cands: List[np.ndarray] = []
            args = last
            while len(cands) < self.max_batch:
                p = spec.getNextTrace(*args)
                if p is None:
                    break
                cands.append(p)
                args = (False, frozenset())
            if not cands:
                assert clusterizer.getNextTrace(*last) is None
                break
            results = self.oracle.test_batch(cands, self.violation)
            self.speculative_replays += len(cands)
            self.batches.append(len(cands))
            j = next((k for k, r in enumerate(results) if r), None)
            consumed = len(cands) if j is None else j + 1
            args = last
            for k in range(consumed):                   # bring the real clusterizer to where the sequential loop would be
                p = clusterizer.getNextTrace(*args)
                assert p is not None and (p == cands[k]).all()
                self.proposals.append(p)
                if not self.skipClockClusters:
                    self.internal_sizes.append(countMsgEvents(minTrace))
                args = (False, frozenset())
            self._stats.increment_replays(consumed)
            if j is None:
                last = (False, frozenset())
                continue
            got = self.oracle.executed(cands[j], self.violation)
            assert got is not None, "batched and single replay of the same candidate disagree"
            ret, ignoredAbsentIndices = got
            ret = EventTrace(ret.events, self.mcs, self.ext_areas)
            if len(ret.events) <= len(minTrace.events):
                minTrace = ret
            last = (True, frozenset(id_of_rec[i] for i in ignoredAbsentIndices))
        return minTrace


    def doMinimizeDpor(self, clusterizer: Clusterizer, startTrace: EventTrace) -> EventTrace:
        """doMinimize's DPORwHeuristics branch (:190-241): one testWithDpor per proposal; the proposals depend on each other's
        outcome AND every one is an exploration of its own, so they are consulted one at a time."""
        minTrace = startTrace
        ev = startTrace.events
        self.oracle.load(startTrace, *clusterizer.selectors(), clusterizer.backtracks())
        nextTrace = clusterizer.getNextTrace(False, frozenset())
        while nextTrace is not None:
            self.proposals.append(nextTrace)
            if not self.skipClockClusters:
                self.internal_sizes.append(countMsgEvents(minTrace))
            self._stats.increment_replays(1)            # (DPORwHeuristics.test counts one replay per call)
            got = self.oracle.test(nextTrace, self.violation)
            ignoredAbsentIds = set()
            if got is not None:
                ret, ignoredAbsentIndices = got
                ret = EventTrace(ret.events, self.mcs, self.ext_areas)
                if len(ret.events) <= len(minTrace.events):
                    minTrace = ret
                # (:227-235) the indices count in the proposal's UniqueMsgEvents; after a backtracked hit they are positions of
                # the hitting interleaving's own next trace - as written.  Pinned: one with no event behind it is dropped
                adjusted = self.oracle.present_records(nextTrace) if hasattr(self.oracle, "present_records") else \
                    [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0] if nextTrace[int(i)]]
                for i in ignoredAbsentIndices:
                    if i < len(adjusted):
                        ignoredAbsentIds.add(int(ev["id"][adjusted[i]]))
                    else:
                        self.dropped_ignored += 1
            nextTrace = clusterizer.getNextTrace(got is not None, frozenset(ignoredAbsentIds))
        return minTrace


def wildcardMinimize(schedulerConfig: SchedulerConfig, mcs: np.ndarray, trace: EventTrace, violation: ViolationFingerprint,
                     **kw) -> Tuple[MinimizationStats, EventTrace]:
    return WildcardMinimizer(schedulerConfig, mcs, trace, violation, **kw).minimize()


# ------------------------------------------------------------------ WildcardTestOracle.scala
class WildcardTestOracle:
    """WildcardTestOracle.scala:11-61 with TestScheduler.STSSched: the TestOracle of RunnerUtils.wildcardDDMin.  test(events)
    runs WildcardMinimizer(skipClockClusters = true) on the subsequence `events` of originalTrace's externals (indices into
    originalTrace.original_externals).  Its ClockClusterizer (STOP_IMMEDIATELY) proposes the trace with every timer and then
    the trace without the j-th timer in id order, and the minimizer stops at the first proposal that reproduces: the proposals
    do not depend on each other's outcome, so a consultation - and a whole DDMin frontier of them - is one launch
    (StsWildcardOracle.test_candidates, demi_replay_wildcard_candidates), reduced to (first_hit, executed length) per candidate.
    `oracle`: a StsWildcardOracle or a stand-in with load / test_candidates / executed (created, and shut down, here when None)."""

    def __init__(self, schedulerConfig: SchedulerConfig, originalTrace: EventTrace,
                 resolutionStrategy: Optional[AmbiguityResolutionStrategy] = None, oracle=None, device: int = 0, p_max: int = 64):
        self.schedulerConfig = schedulerConfig
        self.originalTrace = originalTrace
        self.resolutionStrategy = resolutionStrategy if resolutionStrategy is not None else BackTrackStrategy()
        self._own = oracle is None
        self.oracle = oracle if oracle is not None else StsWildcardOracle(schedulerConfig, device=device, p_max=p_max)
        clusterizer = ClockClusterizer(originalTrace, schedulerConfig.model, self.resolutionStrategy,
                                       aggressiveness=Aggressiveness.STOP_IMMEDIATELY, skipClockClusters=True)
        d = clusterizer.d
        # proposal 0: every delivery (the first clock cluster removes nothing); proposal j: without the j-th timer in id order
        assert d.present(clusterizer.currentCluster | clusterizer.timerIterator.all)[d.idx].all()
        self.drops = np.array([d.rec_of_id[i] for i in clusterizer.timerIterator.toRemove], dtype=np.uint32)
        self.selectors = clusterizer.selectors()
        self.oracle.load(originalTrace, *self.selectors)
        self._min: Optional[Tuple[Tuple[int, ...], int, int]] = None      # (events, first_hit, executed length) of minTrace
        self._min_trace: Optional[EventTrace] = None
        self.records: Dict[Tuple[int, ...], np.void] = {}                # every candidate evaluated so far
        self.first_hits: List[Optional[int]] = []                        # per test() call, in order
        self.violation: Optional[ViolationFingerprint] = None

    def getName(self) -> str:
        return "WildcardTestOracle"

    def present_of(self, first_hit: int) -> np.ndarray:
        p = np.ones(len(self.originalTrace.events), dtype=bool)
        if first_hit:
            p[int(self.drops[first_hit - 1])] = False
        return p

    def evaluate(self, cands: Sequence[Sequence[int]], violation: ViolationFingerprint) -> List[np.void]:
        from .minification import events_to_masks
        cands = [tuple(int(e) for e in c) for c in cands]
        todo = [c for c in dict.fromkeys(cands) if c not in self.records]
        if todo:
            r = self.oracle.test_candidates(events_to_masks(todo), self.drops, violation)
            for c, x in zip(todo, r):
                self.records[c] = x.copy()
        return [self.records[c] for c in cands]

    def test_batch(self, cands, violation: ViolationFingerprint, stats=None) -> List[bool]:
        """Does test() answer Some(trace) for each candidate: reproduced, and not longer than the original (WildcardMinimizer.scala:217)."""
        return [bool(int(r["flags"]) & T.WC_REPRODUCES) and not int(r["flags"]) & T.WC_LONGER for r in self.evaluate(cands, violation)]

    def executed_trace(self, events: Sequence[int], first_hit: int, violation: ViolationFingerprint) -> EventTrace:
        from .minification import events_to_mask
        got = self.oracle.executed(self.present_of(first_hit), violation, mask=events_to_mask(tuple(events)))
        assert got is not None, "the candidates launch and the single replay of the same proposal disagree"
        ev = got[0].events.copy()                 # setOriginalExternalEvents(events): ext_idx renumbered to the subsequence
        remap = np.full(256, 255, dtype=np.uint8)
        remap[list(events)] = np.arange(len(events), dtype=np.uint8)
        ev["ext_idx"] = remap[ev["ext_idx"]]
        areas = self.originalTrace.ext_areas
        return EventTrace(ev, self.originalTrace.original_externals[list(events)].copy(),
                          None if areas is None else np.asarray(areas)[list(events)].copy())

    def test(self, events, violation: ViolationFingerprint, stats: Optional[MinimizationStats] = None, fetch: bool = True):
        """Some(trace) / None as the Scala; fetch=False answers True in place of the trace (DDMin only asks whether it is None)."""
        events = tuple(int(e) for e in events)
        self.violation = violation
        r = self.evaluate([events], violation)[0]
        hit = bool(int(r["flags"]) & T.WC_REPRODUCES)
        first_hit = int(r["first_hit"]) if hit else None
        self.first_hits.append(first_hit)
        if stats is not None:
            stats.increment_replays(first_hit + 1 if hit else 1 + len(self.drops))
        if not hit or int(r["flags"]) & T.WC_LONGER:
            return None                                  # minimize() returned originalTrace itself
        n = int(r["executed_len"])
        if n < (self._min[2] if self._min is not None else len(self.originalTrace.events)):
            self._min, self._min_trace = (events, first_hit, n), None
        return self.executed_trace(events, first_hit, violation) if fetch else True

    @property
    def externalsForMinTrace(self) -> Tuple[int, ...]:
        return self._min[0] if self._min is not None else ()

    @property
    def minTrace(self) -> EventTrace:
        if self._min is None:
            return self.originalTrace
        if self._min_trace is None:
            self._min_trace = self.executed_trace(self._min[0], self._min[1], self.violation)
        return self._min_trace

    def shutdown(self):
        if self._own:
            self.oracle.shutdown()
