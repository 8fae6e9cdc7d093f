"""CPU suite: the wildcard minimizers and the DPOR-based minimizers on tables whose messages carry more than two fields
(DEMI_MODEL_PAYLOADS) and on DEMI_MODEL_ARRAY tables.

  * the (type, area) transliteration of tests/wildcard_payload_cases.py against the oracle, with exact selectors;
  * what the GPU comparison rests on (tests/test_wildcard_payloads_gpu.py), asserted on the transliteration alone;
  * the host mirror (wildcard_minimization.WildcardMinimizer / WildcardTestOracle, runner_utils.wildcardDDMin) against it;
  * ResumableDPOR / editDistanceDporDDMin with the payload areas of the externals, over the oracle backend;
  * the two wildcard modules compiled for gfx950 without a device: no stack frame, no spilled vector register."""
import os
import subprocess
import sys

import numpy as np
import pytest

from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.dpor import ArvindDistanceOrdering, DPORwHeuristics
from demi_amd.incremental_ddmin import ResumableDPOR, dpor_initial_trace, editDistanceDporDDMin
from demi_amd.runner_utils import wildcardDDMin
from demi_amd.schedulers import EventTrace, MinimizationStats, SchedulerConfig

from . import test_wildcard_transliteration_cpu as X
from . import wildcard_payload_cases as Pc
from .test_wildcard_ddmin_cpu import assert_equals_the_transliteration

NO_SKIP = 0xFFFFFFFF


@pytest.mark.parametrize("table", sorted(Pc.WORKLOADS))
def test_exact_selectors_equal_the_oracles_removal_replay(oracle, table):
    """Every selector 0, presence all ones or one delivery cleared: oracle.sts_removal_batch / sts_removal_kept - verdict flags,
    fingerprint, hash, kept marks.  (What anchors the subclass to something that is not itself.)"""
    checked = 0
    for spec in Pc.WORKLOADS[table]:
        model, trace, fp = Pc.get(oracle, spec)
        ev, n = trace.events, len(trace.events)
        lim = T.Limits(0, 0, Pc.P_MAX, 1, fp.code, 0)
        dels = [int(i) for i in np.nonzero(ev["kind"] == T.REC_MSG_EVENT)[0]]
        skips = [NO_SKIP] + dels[::5]
        want = oracle.sts_removal_batch(model, trace.original_externals, ev, skips, lim)
        assert not (want["flags"] & (T.V_PENDING_OVF | T.V_QUEUE_OVF)).any()
        lowered = (ev["kind"] != T.REC_MSG_SEND) | ((ev["flags"] & 1) != 0)
        for k, skip in enumerate(skips):
            present = np.ones(n, dtype=bool)
            if skip != NO_SKIP:
                present[skip] = False
            v, kept, executed, _, _ = Pc.run_candidate(oracle, model, trace, fp, [None] * n, present)
            assert v == (int(want["flags"][k]), int(want["fingerprint"][k]), int(want["hash"][k])), (spec[2], skip)
            if k % 4 == 0:
                ov, okept = oracle.sts_removal_kept(model, trace.original_externals, ev, skip, lim)
                assert (kept[lowered] == np.asarray(okept)[lowered]).all()
            checked += 1
        assert (want["flags"] & T.V_VIOLATION).any() and not (want["flags"] & T.V_VIOLATION).all()
    assert checked >= 15


def test_workload_conditions(oracle):
    """Over the pinned workloads, on the transliteration alone: (a) an ambiguous replay; (b) a replay that delivers a message whose
    AREA differs from every recorded delivery's in a field of index >= 2; (c) reproducing and non-reproducing candidates under
    each policy; (d) a clock cluster removed by ClockClusterizer; (e) no replay with more than 128 pending messages, so p_max =
    128 is sufficient: no candidate is excluded from a comparison and no overflow flag may appear."""
    ambiguous = through_p_hi = 0
    cluster_removed = False
    max_pending = 0
    outcomes = {s: set() for s in ("SrcDstFIFOOnly", "BackTrackStrategy", "LastOnlyStrategy")}       # HEAD, FIRST, LAST
    for table in sorted(Pc.WORKLOADS):
        for spec in Pc.WORKLOADS[table]:
            model, trace, fp = Pc.get(oracle, spec)
            for strategy in outcomes:
                ref = Pc.AreaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=X.STRATEGIES[strategy][0](),
                                               clusteringStrategy="ClockThenSingleton")
                ref.minimize()
                ambiguous += ref.ambiguous
                through_p_hi += ref.left_through_p_hi
                max_pending = max(max_pending, ref.max_pending)
                cluster_removed |= len(ref.clock_values) >= 2 and bool(ref.removed_clusters_that_reproduced)
                outcomes[strategy] |= ({True} if ref.successes else set()) | ({False} if ref.successes < ref.total_replays else set())
    ddmin = Pc.ddmin_reference(oracle)
    assert any(h is not None and h >= 1 for h in ddmin["first_hits"]) and any(h is None for h in ddmin["first_hits"])
    assert len(ddmin["mcs"]) < len(Pc.ddmin_workload(oracle)[1].original_externals) <= 20
    print("payload wildcard workloads: ambiguous=%d through p_hi=%d max pending=%d" % (ambiguous, through_p_hi, max_pending))
    assert ambiguous > 0 and through_p_hi > 0 and cluster_removed and max_pending <= 128
    assert all(o == {True, False} for o in outcomes.values()), outcomes


@pytest.mark.parametrize("clustering", ["ClockClusterizer", "ClockThenSingleton"])
@pytest.mark.parametrize("table", sorted(Pc.WORKLOADS))
def test_mirror_proposes_and_returns_what_the_transliteration_does(oracle, table, clustering):
    spec = Pc.WORKLOADS[table][0]
    model, trace, fp = Pc.get(oracle, spec)
    for strategy in ("LastOnlyStrategy", "BackTrackStrategy"):
        ref = Pc.AreaWildcardMinimizer(oracle, model, trace.original_externals, trace, fp, resolutionStrategy=X.STRATEGIES[strategy][0](),
                                       clusteringStrategy=clustering)
        want = ref.minimize()
        stats = MinimizationStats()
        m = W.WildcardMinimizer(SchedulerConfig(model=model), trace.original_externals, trace, fp, resolutionStrategy=X.STRATEGIES[strategy][1](),
                                clusteringStrategy=clustering, stats=stats, oracle=Pc.AreaTransliteratedDevice(oracle, model))
        _, got = m.minimize()
        assert len(m.proposals) == len(ref.proposals) and all((a == b).all() for a, b in zip(m.proposals, ref.proposals))
        assert stats.total_replays == ref.total_replays
        assert len(got.events) == len(want.events) and got.events.tobytes() == want.events.tobytes()


class _CandidatesDevice:
    """Stands in for StsWildcardOracle where WildcardTestOracle uses it: every replay is an AreaWildcardSTSScheduler."""

    def __init__(self, oracle, model):
        self.oracle, self.model, self.memo = oracle, model, {}
        self.launches, self.batches = 0, []

    def load(self, trace, type_sets, policies):
        self.trace, self.wild = trace, X.wildcards_of(type_sets, policies)

    def _replay(self, mask, present, violation):
        sub = tuple(T.mask_to_events(mask))
        key = (sub, present.tobytes())
        if key not in self.memo:
            v, _, executed, _, _ = Pc.run_candidate(self.oracle, self.model, self.trace, violation, self.wild, present, subseq=list(sub))
            self.memo[key] = (v, executed)
        return self.memo[key]

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
                v, executed = self._replay(m, present, violation)
                if v[0] & T.V_VIOLATION:
                    out[c] = (j, len(executed), T.WC_REPRODUCES | (T.WC_LONGER if len(executed) > len(self.trace.events) else 0), T.NO_HIT, v[2])
                    break
        return out

    def executed(self, present, violation, mask=None):
        v, executed = self._replay(mask, np.asarray(present, dtype=bool), violation)
        return (EventTrace(executed, self.trace.original_externals, self.trace.ext_areas), set()) if v[0] & T.V_VIOLATION else None

    def shutdown(self):
        pass


@pytest.mark.parametrize("depth", [0, 2])
def test_wildcard_ddmin_mirror_equals_the_transliteration(oracle, depth):
    model, trace, fp, strategy = Pc.ddmin_workload(oracle)
    want = Pc.ddmin_reference(oracle)
    stats = MinimizationStats()
    got = wildcardDDMin(SchedulerConfig(model=model), trace, fp, resolutionStrategy=X.STRATEGIES[strategy][1](), stats=stats,
                        speculative_depth=depth, oracle=_CandidatesDevice(oracle, model))
    assert_equals_the_transliteration(want, got, stats)


# ====================================================================== the DPOR-based minimizers with payload areas
def _dpor_run(oracle, model, trace, fp, with_areas, log=None):
    t = trace if with_areas else EventTrace(trace.events, trace.original_externals)
    return editDistanceDporDDMin(SchedulerConfig(model=model), t, fp, stopAtSize=1, maxMaxDistance=4, batch=8,
                                 backend=Pc.oracle_backend_with_areas(oracle, log))


def test_edit_distance_dpor_ddmin_hands_every_consultation_its_areas(oracle):
    """The ledger table: the invariant is decided by the fourth field of one external Deposit.  With trace.ext_areas every
    consultation's backend call gets the areas of exactly the externals it is given, and the MCS holds the Send that carries the
    memo; without areas the fields past the second are 0, the unmodified trace does not violate and nothing reproduces."""
    model, events, areas = Pc.ledger_workload()
    trace, fp = Pc.ledger_execution(oracle, model, events, areas)
    memo_send = next(i for i in range(len(events)) if T.payload_fields(int(areas[i]), 5)[3] == 0x1A5)
    log = []
    mcs, ddmin, verified, _ = _dpor_run(oracle, model, trace, fp, True, log)
    assert verified is not None and memo_send in mcs and len(mcs) < len(events)
    # (the Sends are pairwise different events, so an event names its area)
    area_of_event = {events[i].tobytes(): int(areas[i]) for i in range(len(events))}
    assert len({events[i].tobytes() for i in range(Pc.LEDGER_ACTORS, len(events))}) == Pc.LEDGER_SENDS
    assert log and any(len(ext) < len(events) for ext, _ in log)
    for ext, ar in log:
        assert ar is not None and len(ar) == len(ext) and [int(x) for x in ar] == [area_of_event[e.tobytes()] for e in ext]
    # ... and the gather itself, on ResumableDPOR: the areas of the kept events of the subsequence, in order
    seen = []

    class _Probe:
        def setMaxDistance(self, d):
            pass

        def test(self, ext, fp_, stats, areas=None):
            seen.append((ext.copy(), None if areas is None else np.array(areas)))

        def shutdown(self):
            pass
    sub = (0, 2, memo_send, len(events) - 1)
    ResumableDPOR(_Probe, events, True, areas=areas).test(sub, fp)
    assert (seen[0][0] == events[list(sub)]).all() and (seen[0][1] == areas[list(sub)]).all()
    with pytest.raises(ValueError, match="payload areas"):
        ResumableDPOR(_Probe, events, True, areas=areas[:3])
    # without areas: another answer (this difference is what makes the GPU test meaningful)
    full = tuple(range(len(events)))
    d = DPORwHeuristics(SchedulerConfig(model=model), prioritizePendingUponDivergence=True, backtrackHeuristic=ArvindDistanceOrdering(),
                        batch=8, backend=Pc.oracle_backend_with_areas(oracle))
    init = dpor_initial_trace(trace, model)
    d.setMaxMessagesToSchedule(len(init)); d.setInitialTrace(init); d.backtrackHeuristic.init(d, init); d.setMaxDistance(4)
    assert d.test(events[list(full)], fp) is None                       # the unmodified trace does not violate without its areas
    d2 = DPORwHeuristics(SchedulerConfig(model=model), prioritizePendingUponDivergence=True, backtrackHeuristic=ArvindDistanceOrdering(),
                         batch=8, backend=Pc.oracle_backend_with_areas(oracle))
    d2.setMaxMessagesToSchedule(len(init)); d2.setInitialTrace(init); d2.backtrackHeuristic.init(d2, init); d2.setMaxDistance(4)
    assert d2.test(events[list(full)], fp, areas=areas) is not None
    with pytest.raises(ValueError, match="payload areas"):
        d2.explore(events, fp, areas=areas[:2])
    mcs0, _, verified0, _ = _dpor_run(oracle, model, trace, fp, False)
    assert verified0 is None and tuple(mcs0) != tuple(mcs)


def test_a_backend_without_the_keyword_keeps_working(oracle):
    """Existing backends take (model, externals, prefixes, params, shared): without areas the keyword is not passed."""
    model, events, areas = Pc.ledger_workload()
    calls = []

    def backend(model_, externals, prefixes, params, shared=None):
        calls.append(len(prefixes))
        return oracle.dpor_batch(model_, externals, prefixes, params, shared)
    d = DPORwHeuristics(SchedulerConfig(model=model), depth_bound=20, stopIfViolationFound=False, batch=8, backend=backend)
    d.explore(events, max_interleavings=16)
    assert calls


def test_minimizers_carry_ext_areas_of_the_externals_they_keep(oracle):
    from demi_amd.internal_minimization import executed_trace
    model, events, areas = Pc.ledger_workload()
    trace, fp = Pc.ledger_execution(oracle, model, events, areas)
    kept = np.ones(len(trace.events), dtype=np.uint8)
    sub = (0, 1, 3, 4)
    t = executed_trace(trace, kept, subseq=sub)
    assert (t.ext_areas == areas[list(sub)]).all() and (t.original_externals == events[list(sub)]).all()
    assert executed_trace(trace, kept).ext_areas is trace.ext_areas
    assert executed_trace(EventTrace(trace.events, events), kept, subseq=sub).ext_areas is None
    m = W.WildcardMinimizer(SchedulerConfig(model=model), events, trace, fp, oracle=Pc.AreaTransliteratedDevice(oracle, model))
    assert m.trace.ext_areas is trace.ext_areas
    _, out = m.minimize()
    assert (out.ext_areas == areas).all() and len(out.original_externals) == len(areas)


# ====================================================================== device-free compilation
_SPEC = ("import sys; sys.path.insert(0, %r)\n"
         "from demi_amd import _native, model as M\n"
         "m = {'real5': lambda: M.raft_model(5, election_budget=2, log_cap=8, real_fields=True),\n"
         "     'narrow': lambda: M.raft_model(5), 'wide': lambda: M.raft_model(5, term0=1000, loglen0=300)}[%r]()\n"
         "try:\n"
         "    print('CHECK', _native.specialize_check(m.to_struct()))\n"
         "except _native.DemiError as e:\n"
         "    print('ERR', e)\n")


@pytest.mark.parametrize("table", ["real5", "narrow", "wide"])
def test_wildcard_modules_compile_for_gfx950_without_scratch(tmp_path, table):
    """specialize_check of the real-field table compiles modules 18 and 19 (k2_replay_wildcard, k2_replay_wildcard_candidates) for
    gfx950: no private segment, no spilled vector register (the check of tests/test_fuzz_campaign_cpu.py for modules 20 / 21).
    The narrow and the wide raft5 table still dump both."""
    from .test_jit_cpu import ROOT, _meta_values
    env = dict(os.environ, DEMI_EXPERIMENT="1", DEMI_JIT_DUMP=str(tmp_path / "img"))
    env.pop("DEMI_SPECIALIZE_CHECK_TESTS", None)
    out = subprocess.run([sys.executable, "-c", _SPEC % (ROOT, table)], env=env, capture_output=True, text=True, timeout=280)
    if "hiprtc not found" in out.stdout:
        pytest.skip("no hiprtc in this environment")
    assert "CHECK" in out.stdout and "k2_replay_wildcardE" in out.stdout and "k2_replay_wildcard_candidates" in out.stdout, out.stdout + out.stderr[-2000:]
    for k in (18, 19):
        image = open(str(tmp_path / "img") + ".%d" % k, "rb").read()
        sizes = _meta_values(image, ".private_segment_fixed_size")
        assert sizes and all(v == 0 for v in sizes), (k, sizes)
        assert all(v == 0 for v in _meta_values(image, ".vgpr_spill_count")), k
