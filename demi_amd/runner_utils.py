"""The drivers either side of the hot path: RunnerUtils.fuzz (RunnerUtils.scala:62-147) and the minimization pipeline
of RunnerUtils.runTheGamut (:165-380, the stages that exist on the GPU path).  Host orchestration only: every execution,
replay and interleaving is a kernel launch through the schedulers of this package.
"""
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import types as T
from .incremental_ddmin import dpor_initial_trace
from .minification import SpeculativeDDMin
from .provenance import pruneConcurrentEvents
from .schedulers import (EventTrace, FullyRandom, MinimizationStats, RandomScheduler, ReplayException, ReplayScheduler,
                         SchedulerConfig, ViolationFingerprint)


def fuzz(generateFuzzTest: Callable[[int], np.ndarray], schedulerConfig: SchedulerConfig,
         validate_replay: Optional[Callable[[], ReplayScheduler]] = None, invariant_check_interval: int = 30,
         maxMessages: Optional[int] = None, randomizationStrategyCtor: Callable[[], object] = FullyRandom,
         computeProvenance: bool = True, violationWereLookingFor: Callable[[ViolationFingerprint], bool] = lambda f: True,
         executions_per_test: int = 4096, max_tests: int = 64, scheduler_ctor=RandomScheduler,
         provenance_device: Optional[int] = -1
         ) -> Optional[Tuple[EventTrace, ViolationFingerprint, np.ndarray, np.ndarray]]:
    """RunnerUtils.fuzz: generate a fuzz test, explore it, keep the first violation that (optionally) replays
    deterministically, then prune the deliveries outside the violation's provenance.

    The reference runs ONE random execution per generated test (`new RandomScheduler(config, 1, interval, strategy)`);
    a launch evaluates `executions_per_test` seeded interleavings of the same test and explore() reports the first
    violating one.  generateFuzzTest(i) is Fuzzer.generateFuzzTest for the i-th attempt (fuzzer.generate_fuzz_test /
    raft_trace with a seed derived from i); it may return (events, areas) - fuzzer.generate_fuzz_test_fields: the external
    Sends of a DEMI_MODEL_PAYLOADS table with all their fields -, and the execution is then loaded with those areas.  Returns (trace, violation, initialTrace, filtered) — the depGraph of the
    reference is implicit in the causal-path keys of initialTrace — or None after max_tests tests without a violation
    (the reference loops forever).  provenance_device: the GPU ProvenanceTracker runs on (demi_provenance_prune); -1 = device
    0 when the executions ran on the GPU scheduler (the default scheduler_ctor), the host class (demi_amd/provenance.py)
    for a caller-supplied scheduler; None = always the host class."""
    if provenance_device == -1:
        provenance_device = 0 if scheduler_ctor is RandomScheduler else None
    for attempt in range(max_tests):
        fuzzTest, areas = generateFuzzTest(attempt), None
        if isinstance(fuzzTest, tuple) and len(fuzzTest) == 2:
            fuzzTest, areas = fuzzTest
        fuzzTest = np.ascontiguousarray(fuzzTest, dtype=T.EXT_EVENT_DTYPE)
        sched = scheduler_ctor(schedulerConfig, executions_per_test, invariant_check_interval,
                               randomizationStrategy=randomizationStrategyCtor())
        if maxMessages is not None:
            sched.setMaxMessages(maxMessages)
        try:
            found = sched.explore(fuzzTest) if areas is None else sched.explore(fuzzTest, areas=areas)
        finally:
            sched.shutdown()
        if found is None:
            continue
        trace, violation = found
        if not violationWereLookingFor(violation):
            continue
        if validate_replay is not None:
            replayer = validate_replay()
            deterministic = True
            try:
                v = replayer.replay(trace, violation)
                if not (int(v["flags"]) & T.V_VIOLATION):          # replayer.violationAtEnd.isEmpty
                    deterministic = False
            except ReplayException:
                deterministic = False
            finally:
                replayer.shutdown()
            if not deterministic:
                continue
        initialTrace = dpor_initial_trace(trace, schedulerConfig.model)
        if not computeProvenance:
            filtered = initialTrace[:0]
        elif provenance_device is not None:
            from . import _native
            pctx = _native.Context(provenance_device)
            try:
                filtered = pruneConcurrentEvents(initialTrace, violation.affectedNodes(), ctx=pctx)
            finally:
                pctx.close()
        else:
            filtered = pruneConcurrentEvents(initialTrace, violation.affectedNodes())
        return trace, violation, initialTrace, filtered
    return None


def fuzz_campaign(fuzzer_args, schedulerConfig: SchedulerConfig,
                  validate_replay: Optional[Callable[[], ReplayScheduler]] = None, invariant_check_interval: int = 30,
                  maxMessages: Optional[int] = None, randomizationStrategyCtor: Callable[[], object] = FullyRandom,
                  computeProvenance: bool = True, violationWereLookingFor: Callable[[ViolationFingerprint], bool] = lambda f: True,
                  executions_per_test: int = 64, max_tests: int = 1024, tests_per_launch: int = 256, test_seed_base: int = 0,
                  provenance_device: Optional[int] = 0, device: int = 0, p_max: int = 64, specialize: bool = False, ctx=None,
                  in_flight: Optional[int] = None
                  ) -> Optional[Tuple[EventTrace, ViolationFingerprint, np.ndarray, np.ndarray]]:
    """fuzz() with the test axis on the device: what fuzz(lambda i: generate_fuzz_test(.., seed = test_seed_base + i), ..) returns
    for the same executions_per_test and max_tests - (trace, violation, initialTrace, filtered) or None - found by launches of
    tests_per_launch generated tests each (demi_fuzz_campaign: k_fuzz_generate, K1 with a workgroup per test, the per-test flags).

    fuzzer_args: (num_events, weights, send_generator, prefix[, postfix]) - Fuzzer's constructor arguments with the
    MessageGenerator as a fuzzer.SendGenerator, or as a fuzzer.FieldSendGenerator: generated Sends with up to six fields
    (demi_fuzz_campaign_fields), which is how a DEMI_MODEL_PAYLOADS table is fuzzed; the found execution is then recorded with
    the test's payload areas and the EventTrace carries them (ext_areas).
    ctx: a caller's _native.Context with the model loaded (and specialised, where the table needs it): it is used and NOT
    closed, so that many campaigns share one compilation of the table; `device` and `specialize` are then the caller's.  The one (test, execution) the device reports is re-run through the recording
    path (RandomScheduler.explore's own last step) for its EventTrace; replay validation, violationWereLookingFor and the
    provenance pruning are fuzz()'s, and a test they reject sends the campaign on from the test after it.  When an execution
    before the reported one was aborted on a capacity, the campaign goes on with the largest pending set (fuzz() decides such an
    execution alone with it; verdicts without an overflow do not depend on p_max); CapacityExceeded if that does not suffice.
    in_flight: 1..3 launches of every campaign call on the device at a time (demi_fuzz_campaign_pipelined; 0 = 2) - the same
    answer; None, the default, is the synchronous entry point."""
    from . import _native
    from .capacity import CapacityExceeded, is_largest, largest
    from .schedulers import SrcDstFIFO
    num_events, weights, send_gen, prefix = fuzzer_args[:4]
    postfix = fuzzer_args[4] if len(fuzzer_args) > 4 else ()
    model = schedulerConfig.model
    if model is None or model.inv_kind == T.INV_NONE:
        raise ValueError("Must invoke setInvariant before test()")
    strategy = randomizationStrategyCtor()
    exec_seed_base = strategy.seed
    mm = 0 if maxMessages is None or maxMessages >= 0x7FFFFFFF else maxMessages
    lim = T.Limits(mm, max(0, invariant_check_interval), p_max, 0, 0, 1 if schedulerConfig.populate_all_actors else 0,
                   T.STRATEGY_SRC_DST_FIFO if isinstance(strategy, SrcDstFIFO) else T.STRATEGY_FULLY_RANDOM)
    from .fuzzer import FieldSendGenerator
    with_fields = isinstance(send_gen, FieldSendGenerator)
    own_ctx = ctx is None
    if own_ctx:
        ctx = _native.Context(device)
    try:
        if own_ctx:
            ctx.model_load(model.to_struct())
            if getattr(model, "compiled_only", False) or specialize:
                ctx.model_specialize()
        start = 0
        while start < max_tests:
            res, fuzzTest, *found_areas = ctx.fuzz_campaign(num_events, weights, send_gen, prefix, lim, postfix=postfix,
                                                            executions_per_test=executions_per_test, tests_per_launch=tests_per_launch,
                                                            max_tests=max_tests - start, test_seed_base=test_seed_base + start,
                                                            exec_seed_base=exec_seed_base, in_flight=in_flight)
            areas = found_areas[0] if with_fields else None
            if res.capacity_aborts:
                # an execution aborted on a capacity has no verdict.  fuzz() decides it alone with the largest pending set; a verdict
                # does not depend on p_max unless the execution overflows, so the campaign from this test on with the largest
                # pending set answers what fuzz() answers.  Aborts that remain are beyond the engine, as they are for fuzz().
                if is_largest(lim.p_max):
                    raise CapacityExceeded("%d tests of the campaign have executions beyond p_max = %d" % (res.capacity_aborts, lim.p_max))
                lim = largest(lim)
                continue
            if not res.found:
                return None
            start += int(res.test_index) + 1
            ctx.trace_load(fuzzTest, areas)
            v, rec = ctx.random_get_trace(exec_seed_base + int(res.exec_index), lim)
            assert v.flags & T.V_VIOLATION and int(v.fingerprint) == int(res.verdict.fingerprint)
            used = T.verdict_trace_idx(v.flags)
            trace = EventTrace(rec, fuzzTest[:used], None if areas is None else areas[:used].copy())
            violation = ViolationFingerprint(int(v.fingerprint), model.fp_match_mask)
            if not violationWereLookingFor(violation):
                continue
            if validate_replay is not None:
                replayer = validate_replay()
                deterministic = True
                try:
                    rv = replayer.replay(trace, violation)
                    if not (int(rv["flags"]) & T.V_VIOLATION):
                        deterministic = False
                except ReplayException:
                    deterministic = False
                finally:
                    replayer.shutdown()
                if not deterministic:
                    continue
            initialTrace = dpor_initial_trace(trace, model)
            if not computeProvenance:
                filtered = initialTrace[:0]
            elif provenance_device is not None:
                filtered = _prune_on(provenance_device, initialTrace, violation)       # (a context of its own, as in fuzz())
            else:
                filtered = pruneConcurrentEvents(initialTrace, violation.affectedNodes())
            return trace, violation, initialTrace, filtered
        return None
    finally:
        if own_ctx:
            ctx.close()


def _prune_on(device, initialTrace, violation):
    from . import _native
    pctx = _native.Context(device)
    try:
        return pruneConcurrentEvents(initialTrace, violation.affectedNodes(), ctx=pctx)
    finally:
        pctx.close()


def wildcardDDMin(schedulerConfig: SchedulerConfig, originalTrace: EventTrace, violation: ViolationFingerprint,
                  resolutionStrategy=None, stats: Optional[MinimizationStats] = None, native: bool = False, speculative_depth: int = 0,
                  max_candidates: int = 0, sequential: bool = False, oracle=None, device: int = 0, p_max: int = 64):
    """RunnerUtils.wildcardDDMin (RunnerUtils.scala:709-767) with TestScheduler.STSSched: DDMin over the externals of
    originalTrace (WaitQuiescence stripped, as runTheGamut hands them over, :370-378) whose oracle is WildcardTestOracle.
    Returns what the Scala returns - (externals of the MCS as indices into originalTrace.original_externals, stats, validated
    trace, violation) - and, fifth, the DDMin record (consulted, first_hits, batches).

    Two modes that agree on the MCS, the consultations, their first_hits, stats.total_replays and the validated trace:
    native=False walks the decision tree here over replay_wildcard_candidates (speculative_depth levels ahead per launch;
    sequential=True, or speculative_depth = 0 with a stand-in oracle, consults one candidate at a time), native=True makes the
    one call demi_wildcard_ddmin (depth / max_candidates as in demi_ddmin_params; sequential = one consultation per launch).
    `oracle`: a stand-in for StsWildcardOracle (tests)."""
    from . import wildcard_minimization as W
    from .minification import DDMin, EventDagView, UnmodifiedEventDag
    stats = stats if stats is not None else MinimizationStats()
    externals = originalTrace.original_externals
    wo = W.WildcardTestOracle(schedulerConfig, originalTrace, resolutionStrategy=resolutionStrategy, oracle=oracle, device=device,
                              p_max=p_max)
    try:
        dag = UnmodifiedEventDag(externals)
        keep = tuple(i for i in dag.events if int(externals[i]["kind"]) != T.EV_WAIT_QUIESCENCE)
        if native:
            par = T.DdminParams(depth=1 if sequential else speculative_depth, max_candidates=1 if sequential else max_candidates,
                                check_unmodified=0, verify_mcs=1)
            mcs, consulted, batches, st, res = wo.oracle._ctx.wildcard_ddmin(wo.oracle._limits(violation), wo.drops, params=par)
            stats.total_replays = int(res.total_replays)
            record = _WildcardDdminRecord([(c, p) for c, p, _ in consulted], [h for _, _, h in consulted], batches, st, res)
            wo.violation = violation
            if len(mcs) < len(keep):
                if st.verified:
                    validated = wo.executed_trace(mcs, int(res.mcs_first_hit), violation)
                else:       # the stop-gap of :752-758: the smallest trace a consultation reproduced, as the native call kept it
                    if int(res.min_first_hit) == T.NO_HIT:
                        return (), stats, originalTrace, violation, record
                    ext = tuple(T.mask_to_events(np.array(list(res.min_externals), dtype=np.uint64)))
                    return ext, stats, wo.executed_trace(ext, int(res.min_first_hit), violation), violation, record
                return tuple(mcs), stats, validated, violation, record
            return tuple(mcs), stats, originalTrace, violation, record
        if sequential or not speculative_depth:
            ddmin = DDMin(_FetchlessOracle(wo), checkUnmodifed=False, stats=stats)
        else:
            ddmin = _WildcardSpeculativeDDMin(wo, depth=speculative_depth, checkUnmodifed=False, stats=stats)
        mcs = ddmin.minimize(EventDagView(dag, keep), violation)
        record = _WildcardDdminRecord(ddmin.consulted, list(wo.first_hits), list(getattr(ddmin, "batches", [])), None, None)
        if mcs.length < len(keep):
            validated = wo.test(mcs.events, violation, MinimizationStats())            # ddmin.verify_mcs
            if validated is None:
                return wo.externalsForMinTrace, stats, wo.minTrace, violation, record
            return tuple(mcs.events), stats, validated, violation, record
        return tuple(mcs.events), stats, originalTrace, violation, record
    finally:
        wo.shutdown()


class _FetchlessOracle:
    """DDMin only asks whether test() is None: the executed trace of a consultation is not fetched."""

    def __init__(self, wo):
        self.wo = wo

    def test(self, events, violation, stats=None):
        return self.wo.test(events, violation, stats, fetch=False)


class _WildcardDdminRecord:
    """consulted [(candidate indices, passes)], first_hits [int or None] in consultation order, candidates per launch; the
    native call's demi_ddmin_stats / demi_wildcard_ddmin_result (None for the mirror's walk)."""

    def __init__(self, consulted, first_hits, batches, st, res):
        self.consulted = [(tuple(int(i) for i in c), bool(p)) for c, p in consulted]
        self.first_hits = list(first_hits)
        self.batches = list(batches)
        self.stats, self.result = st, res


class _WildcardSpeculativeDDMin(SpeculativeDDMin):
    """SpeculativeDDMin whose consultations are WildcardTestOracle's: the frontier's candidates are evaluated in one launch,
    and the consultation itself does the oracle's bookkeeping (first_hit + 1 or 1 + T replays, minTrace)."""

    def _passes(self, events):
        events = tuple(events)
        if events not in self.oracle.records:
            todo = {events: None}
            self._frontier(*self._node, self.depth, todo)
            cands = [c for c in todo if c not in self.oracle.records]
            results = self.oracle.test_batch(cands, self.violation_fingerprint, None)
            self.speculative_replays += len(cands) * (1 + len(self.oracle.drops))
            self.batches.append(len(cands))
            for c, reproduced in zip(cands, results):
                self.cache[c] = not reproduced
        passes = self.oracle.test(events, self.violation_fingerprint, self._stats, fetch=False) is None
        self.consulted.append((events, passes))
        return passes


def run_the_gamut(schedulerConfig: SchedulerConfig, trace: EventTrace, violation: ViolationFingerprint,
                  stages: Sequence[str] = ("DDMin", "IntMin"), device: int = 0, p_max: int = 64,
                  shouldRerunDDMin: Callable[[np.ndarray], bool] = lambda externals: True, native_intmin: bool = False,
                  native_wildcards: bool = False, dpor_budget: int = 256):
    """The stages of RunnerUtils.runTheGamut (:165-380) that run on the GPU path, in the reference's order:
    stsSchedDDMin (external events), then minimizeInternals with LeftToRightOneAtATime, then - only when named in `stages` -
    "WildCardDDMinNoBacktracks" and "WildCardDDMinLastOnly" (wildcardDDMin over the current trace, :363-411, guarded by
    shouldRerunDDMin as there), then "WildcardsNoBackTracks" and "WildcardsLastOnly" (wildcard_minimization.WildcardMinimizer, ClockClusterizer),
    then "Wildcards" (the same with DPORwHeuristics as the oracle, dpor_budget interleavings per proposal).  Returns a dict with the MCS
    (indices into trace.original_externals), the verified MCS execution, the internally minimized execution and the
    replay counts of each stage.  native_intmin: the internal minimization as one native call (demi_minimize_internals); native_wildcards: each
    wildcard stage likewise (demi_minimize_wildcards)."""
    from .internal_minimization import countMsgEvents, minimizeInternals
    from .minification import stsSchedDDMin
    from .schedulers import STSScheduler
    out = {"original_externals": len(trace.original_externals), "original_deliveries": countMsgEvents(trace)}
    cur_trace, mcs = trace, tuple(range(len(trace.original_externals)))
    if "DDMin" in stages:
        sts = STSScheduler(schedulerConfig, trace, device=device, p_max=p_max)
        try:
            stats = MinimizationStats()
            mcs, ddmin, _ = stsSchedDDMin(sts, trace.original_externals, violation, stats=stats)
            verified = sts.executed_trace(mcs, violation)
        finally:
            sts.shutdown()
        out.update(mcs=mcs, ddmin_replays=stats.total_replays, verified_mcs=verified)
        if verified is not None:
            cur_trace = verified
    if "IntMin" in stages and cur_trace is not None:
        stats = MinimizationStats()
        _, minimized = minimizeInternals(schedulerConfig, cur_trace.original_externals, cur_trace, violation, stats=stats,
                                         device=device, p_max=p_max, native=native_intmin)
        out.update(intmin_replays=stats.total_replays, minimized=minimized, minimized_deliveries=countMsgEvents(minimized))
        cur_trace = minimized
    # wildcard DDMin over the externals, opt-in, as RunnerUtils.scala:363-411 places and configures it: without backtracks (the
    # default strategy), then with LastOnlyStrategy
    for stage, strategy in (("WildCardDDMinNoBacktracks", None), ("WildCardDDMinLastOnly", "LastOnlyStrategy")):
        if stage in stages and cur_trace is not None and shouldRerunDDMin(cur_trace.original_externals):
            from . import wildcard_minimization as W
            stats = MinimizationStats()
            ext, _, validated, _, _ = wildcardDDMin(schedulerConfig, cur_trace, violation, native=True, stats=stats,
                                                    resolutionStrategy=getattr(W, strategy)() if strategy else None,
                                                    device=device, p_max=p_max)
            out.setdefault("wildcard_ddmin_replays", {})[stage] = stats.total_replays
            out.setdefault("wildcard_ddmin_externals", {})[stage] = len(ext)
            if validated is not None:
                cur_trace = validated
                out.update(wildcard_ddmin_trace=cur_trace)
    # the wildcard (fungible-clock) stages, opt-in, as RunnerUtils.scala:412-440 configures them: STSSched as the oracle, the
    # default resolution strategy (BackTrackStrategy, its backtrack points no-ops) and then LastOnlyStrategy
    for stage, strategy in (("WildcardsNoBackTracks", None), ("WildcardsLastOnly", "LastOnlyStrategy")):
        if stage in stages and cur_trace is not None:
            from . import wildcard_minimization as W
            stats = MinimizationStats()
            _, cur_trace = W.WildcardMinimizer(schedulerConfig, cur_trace.original_externals, cur_trace, violation, stats=stats,
                                               resolutionStrategy=getattr(W, strategy)() if strategy else None,
                                               device=device, p_max=p_max, native=native_wildcards).minimize()
            out.setdefault("wildcard_replays", {})[stage] = stats.total_replays
            out.update(wildcard_minimized=cur_trace, wildcard_deliveries=countMsgEvents(cur_trace))
    # "Wildcards" (RunnerUtils.scala:441-454), opt-in: the same minimizer with fungClocksScheduler = DPORwHeuristics as its oracle -
    # the default resolution strategy's backtrack points are explored (wildcard_minimization.DporWildcardOracle).  The
    # reference's timeBudgetSeconds is dpor_budget here, interleavings per proposal.
    if "Wildcards" in stages and cur_trace is not None:
        from . import wildcard_minimization as W
        stats = MinimizationStats()
        _, cur_trace = W.WildcardMinimizer(schedulerConfig, cur_trace.original_externals, cur_trace, violation, stats=stats,
                                           testScheduler=W.TestScheduler.DPORwHeuristics, dpor_budget=dpor_budget,
                                           device=device, p_max=p_max).minimize()
        out.setdefault("wildcard_replays", {})["Wildcards"] = stats.total_replays
        out.update(wildcard_minimized=cur_trace, wildcard_deliveries=countMsgEvents(cur_trace))
    return out
