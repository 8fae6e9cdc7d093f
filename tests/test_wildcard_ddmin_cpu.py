"""CPU suite: RunnerUtils.wildcardDDMin (RunnerUtils.scala:709-767) and WildcardTestOracle.test (WildcardTestOracle.scala:33-61)
transliterated, and the demi_amd mirror's host logic (wildcard_minimization.WildcardTestOracle, runner_utils.wildcardDDMin)
against them.

The transliteration is assembled from tests/test_wildcard_transliteration_cpu.py: ScalaWildcardMinimizer(skipClockClusters =
True) whose replays take the external subsequence (run_candidate(..., subseq=...)), under the sequential DDMin.  The mirror is
held against it through a stand-in device whose every replay is the transliterated scheduler (the TransliteratedDevice
pattern), with speculation on and off.  tests/test_wildcard_ddmin_gpu.py holds the kernel and demi_wildcard_ddmin against
this file.

LENGTH CONVENTION of `ret.size <= minTrace.size` (WildcardMinimizer.scala:217): both sides are counted as the library writes
executed traces down (test_wildcard_transliteration_cpu's module docstring)."""
import numpy as np
import pytest

from demi_amd import model as M
from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.apps import raft5_config2
from demi_amd.minification import DDMin, EventDagView, UnmodifiedEventDag, events_to_mask, stsSchedDDMin
from demi_amd.runner_utils import wildcardDDMin
from demi_amd.schedulers import EventTrace, MinimizationStats, SchedulerConfig, ViolationFingerprint

from . import test_wildcard_transliteration_cpu as X
from .test_minification_cpu import OracleSTS, _violating_execution

# The workloads: (index into the violating executions of raft5_config2's 50-event trace on the raft table with election_budget = 2,
# resolution strategy) - the execution loaded with ALL the externals that were injected (DDMin has not run yet).  Chosen on the
# transliteration alone, from X.WORKLOAD_SKIPS and the executions after them (test_workload_conditions): consultations that
# reproduce with every timer (first_hit 0), only without a later one (6, 9, 14, 19), and never; (2, BackTrack) is the case in
# which no consultation reproduces at all and DDMin ends where it cannot split further.
WORKLOADS = ((0, "LastOnlyStrategy"), (2, "BackTrackStrategy"), (4, "BackTrackStrategy"), (6, "LastOnlyStrategy"), (12, "BackTrackStrategy"))

_workloads = {}
_replays = {}
_reference = {}


def workload(oracle, skip):
    """(model, EventTrace of the violating execution with all the externals that were injected, fingerprint)."""
    if skip not in _workloads:
        _, events, lim = raft5_config2()
        model = M.raft_model(5, **X.WORKLOAD_MODEL)
        vv, rec, used = _violating_execution(oracle, model, events, lim, skip)
        _workloads[skip] = (model, EventTrace(rec, used), ViolationFingerprint(vv.fingerprint))
    return _workloads[skip]


def replay(oracle, skip, strategy, subseq, present, wild=None, who="scala"):
    """run_candidate of one proposal: (verdict triple, executed trace).  Once per (workload, strategy, subsequence, presence)
    and per `who` supplied the wildcards - the transliterated clusterizer's and the mirror's selectors are never mixed."""
    key = (who, skip, strategy, tuple(subseq), np.asarray(present, dtype=bool).tobytes())
    if key not in _replays:
        model, trace, fp = workload(oracle, skip)
        if wild is None:
            wild = X.wildcards_of(*W.ClockClusterizer(trace, model, X.STRATEGIES[strategy][1](), skipClockClusters=True).selectors())
        v, _, executed, _, _ = X.run_candidate(oracle, model, trace, fp, wild, present, subseq=list(subseq))
        _replays[key] = (v, executed)
    return _replays[key]


# ====================================================================== WildcardTestOracle.scala, RunnerUtils.wildcardDDMin
class _SubsequenceMinimizer(X.ScalaWildcardMinimizer):
    """ScalaWildcardMinimizer whose `mcs` is a subsequence of the trace's externals, given by index: testWithStsSched replays
    nextTrace.subsequenceIntersection(mcs)."""

    def __init__(self, oracle, skip, strategy, subseq, trace, violation):
        model = workload(oracle, skip)[0]
        super().__init__(oracle, model, trace.original_externals, trace, violation, skipClockClusters=True,
                         resolutionStrategy=X.STRATEGIES[strategy][0]())
        self.key, self.subseq = (skip, strategy), tuple(subseq)

    def testWithSTSSched(self, startTrace, present, wild):
        self.total_replays += 1
        v, executed = replay(self.oracle, self.key[0], self.key[1], self.subseq, present, wild)
        if not (v[0] & T.V_VIOLATION):
            return None, set()
        executed = executed.copy()            # the records name their external by its index: re-based on the subsequence
        for e in executed:
            if int(e["ext_idx"]) != 255:
                e["ext_idx"] = self.subseq.index(int(e["ext_idx"]))
        return EventTrace(executed, startTrace.original_externals[list(self.subseq)]), set()      # (STOP_IMMEDIATELY: the ids are not used)


class ScalaWildcardTestOracle:
    """WildcardTestOracle.scala:11-61."""

    def __init__(self, oracle, skip, strategy, originalTrace):
        self.oracle, self.skip, self.strategy, self.originalTrace = oracle, skip, strategy, originalTrace
        self.minTrace = originalTrace
        self.externalsForMinTrace = ()
        self.first_hits = []          # (test bookkeeping) per test(): the proposal that reproduced, None if none did
        self.longer = 0               #                    reproduced, but `ret.size <= minTrace.size` failed

    def test(self, events, violation_fingerprint, stats):
        minimizer = _SubsequenceMinimizer(self.oracle, self.skip, self.strategy, events, self.originalTrace, violation_fingerprint)
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


def scala_wildcard_ddmin(oracle, skip, strategy):
    """RunnerUtils.wildcardDDMin with the externals runTheGamut hands it (WaitQuiescence stripped, :370-378).  Once per workload."""
    if (skip, strategy) in _reference:
        return _reference[(skip, strategy)]
    model, originalTrace, violation = workload(oracle, skip)
    externals = originalTrace.original_externals
    wo = ScalaWildcardTestOracle(oracle, skip, strategy, originalTrace)
    dag = UnmodifiedEventDag(externals)
    keep = tuple(i for i in dag.events if int(externals[i]["kind"]) != T.EV_WAIT_QUIESCENCE)
    stats = MinimizationStats()
    ddmin = DDMin(wo, stats=stats)
    mcs = ddmin.minimize(EventDagView(dag, keep), violation)
    consulted_hits = list(wo.first_hits)
    min_after_search = (tuple(wo.externalsForMinTrace), len(wo.minTrace.events))       # (verify_mcs below consults the oracle once more)
    if mcs.length < len(keep):
        validated = ddmin.verify_mcs(mcs, violation)
        if validated is None:
            ret = (tuple(wo.externalsForMinTrace), wo.minTrace)
        else:
            ret = (tuple(mcs.events), EventTrace(validated.events, externals[list(mcs.events)]))
    else:
        ret = (tuple(mcs.events), originalTrace)
    out = {"mcs": ret[0], "trace": ret[1], "consulted": list(ddmin.consulted), "first_hits": consulted_hits,
           "total_replays": stats.total_replays, "longer": wo.longer, "min": min_after_search}
    _reference[(skip, strategy)] = out
    return out


# ====================================================================== the mirror against the transliteration
class TransliteratedCandidatesDevice:
    """Stands in for StsWildcardOracle where WildcardTestOracle uses it (load / test_candidates / executed): every replay is a
    ScalaWildcardSTSScheduler; the reduction is the sequential loop's."""

    def __init__(self, oracle, skip, strategy):
        self.oracle, self.skip, self.strategy = oracle, skip, strategy
        self.launches = 0
        self.batches = []

    def load(self, trace, type_sets, policies):
        self.trace, self.wild = trace, X.wildcards_of(type_sets, policies)

    def test_candidates(self, masks, drops, violation, base_present=None):
        self.launches += 1
        self.batches.append(len(masks))
        out = np.zeros(len(masks), dtype=T.WILDCARD_CANDIDATE_DTYPE)
        for c, m in enumerate(masks):
            out[c] = (T.NO_HIT, 0, 0, T.NO_HIT, 0)
            for j in range(len(drops) + 1):
                present = np.ones(len(self.trace.events), dtype=bool)
                if j:
                    present[int(drops[j - 1])] = False
                v, executed = replay(self.oracle, self.skip, self.strategy, T.mask_to_events(m), present, self.wild, "mirror")
                if v[0] & T.V_VIOLATION:
                    longer = len(executed) > len(self.trace.events)
                    out[c] = (j, len(executed), T.WC_REPRODUCES | (T.WC_LONGER if longer else 0), T.NO_HIT, v[2])
                    break
        return out

    def executed(self, present, violation, mask=None):
        v, executed = replay(self.oracle, self.skip, self.strategy, T.mask_to_events(mask), present, self.wild, "mirror")
        return (EventTrace(executed, self.trace.original_externals), set()) if v[0] & T.V_VIOLATION else None

    def shutdown(self):
        pass


def assert_equals_the_transliteration(want, got, stats):
    ext, _, trace, _, record = got
    assert tuple(ext) == want["mcs"]
    assert record.consulted == [(tuple(c), p) for c, p in want["consulted"]]
    assert record.first_hits == want["first_hits"]
    assert stats.total_replays == want["total_replays"]
    assert len(trace.events) == len(want["trace"].events) and trace.events.tobytes() == want["trace"].events.tobytes()
    assert trace.original_externals.tobytes() == want["trace"].original_externals.tobytes()


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("skip,strategy", WORKLOADS)
def test_mirror_equals_the_transliteration(oracle, skip, strategy, depth):
    model, trace, fp = workload(oracle, skip)
    want = scala_wildcard_ddmin(oracle, skip, strategy)
    stats = MinimizationStats()
    dev = TransliteratedCandidatesDevice(oracle, skip, strategy)
    got = wildcardDDMin(SchedulerConfig(model=model), trace, fp, resolutionStrategy=X.STRATEGIES[strategy][1](), stats=stats,
                        speculative_depth=depth, oracle=dev)
    assert_equals_the_transliteration(want, got, stats)
    if depth:
        assert max(dev.batches) > 1 and len(dev.batches) < len(want["consulted"])      # (speculation did batch)


def test_the_oracle_proposes_what_the_clusterizer_does(oracle):
    """Proposal 0 keeps every delivery, proposal j drops the j-th timer in id order: the sequence ScalaClockClusterizer
    (skipClockClusters, STOP_IMMEDIATELY) walks while nothing reproduces."""
    model, trace, fp = workload(oracle, X.WORKLOAD_SKIPS[0])
    wo = W.WildcardTestOracle(SchedulerConfig(model=model), trace, oracle=TransliteratedCandidatesDevice(oracle, 0, "BackTrackStrategy"))
    c = X.ScalaClockClusterizer(trace, X.ScalaFingerprinter(model), X.ScalaBackTrackStrategy(), aggressiveness=X.STOP_IMMEDIATELY,
                                skipClockClusters=True)
    j, nxt = 0, c.getNextTrace(False, set())
    while nxt is not None:
        assert (nxt[0] == (wo.present_of(j) & (trace.events["kind"] == T.REC_MSG_EVENT))).all()
        j, nxt = j + 1, c.getNextTrace(False, set())
    assert j == 1 + len(wo.drops) and len(wo.drops) >= 2


def test_workload_conditions(oracle):
    """What the GPU comparison rests on, asserted on the transliteration alone: (a) a consultation whose wildcard answer differs
    from the exact STSScheduler.test answer for the same subsequence, (b) a consultation that reproduced only after a timer was
    dropped (first_hit >= 1), (c) a consultation where no proposal reproduces.  (d), an MCS strictly smaller than
    stsSchedDDMin's; how often a reproducing proposal was longer than the original is printed."""
    differs = late = none = smaller = longer = 0
    for skip, strategy in WORKLOADS:
        model, trace, fp = workload(oracle, skip)
        ref = scala_wildcard_ddmin(oracle, skip, strategy)
        sts = OracleSTS(oracle, model, trace.original_externals, trace.events, fp.code)
        for (cand, passes), hit in zip(ref["consulted"], ref["first_hits"]):
            differs += (sts.test(cand, fp, None) is None) != passes
            late += hit is not None and hit >= 1
            none += hit is None
        exact_mcs, _, _ = stsSchedDDMin(sts, trace.original_externals, fp, speculative_depth=2)
        smaller += len(ref["mcs"]) < len(exact_mcs)
        longer += ref["longer"]
    print("wildcardDDMin workloads: differs=%d first_hit>=1: %d no hit: %d smaller MCS: %d longer-than-original: %d"
          % (differs, late, none, smaller, longer))
    assert differs > 0 and late > 0 and none > 0
    assert smaller > 0         # (d) was observed on these workloads; `longer` (WildcardMinimizer.scala:217 failing) was not
