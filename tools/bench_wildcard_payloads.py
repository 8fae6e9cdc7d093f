#!/usr/bin/env python
"""Wildcard minimization on tables whose messages carry more than two fields, on one GPU:

  * one WildcardMinimizer pass (ClockThenSingleton, LastOnlyStrategy) batched (max_batch 16384) against the reference's loop
    shape (max_batch 1), on the workloads of tests/wildcard_payload_cases.py;
  * one demi_wildcard_ddmin call batched against depth = 1, max_candidates = 1;
  * the time of demi_model_specialize and of the first wildcard launch (which compiles the two wildcard modules lazily).

DEMI_EXPERIMENT=1 DEMI_K2_VERBOSE=1 ... --shapes: only the first part, every launch printing its LDS bytes and resident workgroups
per CU under the table's name."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demi_amd import _native, types as T                                   # noqa: E402
from demi_amd import wildcard_minimization as W                            # noqa: E402
from demi_amd.runner_utils import wildcardDDMin                            # noqa: E402
from demi_amd.schedulers import MinimizationStats, SchedulerConfig         # noqa: E402
from oracle import oracle_py as oracle                                     # noqa: E402
from tests import wildcard_payload_cases as Pc                             # noqa: E402

P_MAX = 128


def minimizer(name, model, trace, fp):
    cfg = SchedulerConfig(model=model)
    dev = W.StsWildcardOracle(cfg, p_max=P_MAX)          # one context (the table compiled once) for both loop shapes
    try:
        row = []
        for max_batch in (16384, 1, 16384, 1):
            stats = MinimizationStats()
            dev.launches, dev.batches = 0, []
            t0 = time.perf_counter()
            m = W.WildcardMinimizer(cfg, trace.original_externals, trace, fp, resolutionStrategy=W.LastOnlyStrategy(),
                                    clusteringStrategy=W.ClusteringStrategy.ClockThenSingleton, stats=stats, max_batch=max_batch, oracle=dev)
            _, out = m.minimize()
            row.append((max_batch, (time.perf_counter() - t0) * 1e3, dev.launches, stats.total_replays, m.speculative_replays,
                        int((out.events["kind"] == T.REC_MSG_EVENT).sum())))
        print("%s | %d externals, %d deliveries |" % (name, len(trace.original_externals), int((trace.events["kind"] == T.REC_MSG_EVENT).sum())),
              " | ".join("max_batch %d: %.1f ms, %d launches, %d sequential replays, %d replayed -> %d deliveries" % r for r in row[2:]),
              "| (first pass, with the lazy compilation: %.1f ms)" % row[0][1])
    finally:
        dev.shutdown()


def ddmin():
    model, trace, fp, strategy = Pc.ddmin_workload(oracle)
    cfg = SchedulerConfig(model=model)
    for kw, label in ((dict(), "batched"), (dict(sequential=True), "depth 1, max_candidates 1"), (dict(), "batched"),
                      (dict(sequential=True), "depth 1, max_candidates 1")):
        stats = MinimizationStats()
        t0 = time.perf_counter()
        got = wildcardDDMin(cfg, trace, fp, resolutionStrategy=getattr(W, strategy)(), stats=stats, p_max=P_MAX, native=True, **kw)
        dt = (time.perf_counter() - t0) * 1e3
        st = got[4].stats
        print("wildcardDDMin real5, %d externals, %s: %.1f ms whole call (context, compilation, load included), %d consultations, %d launches, "
              "%d replays -> MCS of %d" % (len(trace.original_externals), label, dt, st.consultations, st.launches, stats.total_replays, len(got[0])))
    # the native call alone on a loaded context
    wo = W.WildcardTestOracle(cfg, trace, resolutionStrategy=getattr(W, strategy)(), p_max=P_MAX)
    try:
        ctx, lim = wo.oracle._ctx, wo.oracle._limits(fp)
        for par, label in ((T.DdminParams(check_unmodified=0, verify_mcs=1), "batched"),
                           (T.DdminParams(depth=1, max_candidates=1, check_unmodified=0, verify_mcs=1), "depth 1, max_candidates 1")):
            ctx.wildcard_ddmin(lim, wo.drops, params=par)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                _, _, batches, st, _ = ctx.wildcard_ddmin(lim, wo.drops, params=par)
                ts.append((time.perf_counter() - t0) * 1e3)
            print("demi_wildcard_ddmin alone, %s: median %.2f ms (min %.2f .. max %.2f), %d launches" % (label, float(np.median(ts)), min(ts), max(ts), st.launches))
    finally:
        wo.shutdown()


def specialise():
    for name, spec in (("real5", Pc.WORKLOADS["real5"][0]), ("real3", Pc.WORKLOADS["real3"][0]), ("array5", Pc.WORKLOADS["array5"][0])):
        model, trace, fp = Pc.get(oracle, spec)
        print("table %s (%d externals loaded):" % (name, len(trace.original_externals)), file=sys.stderr, flush=True)
        ctx = _native.Context(0)
        try:
            ctx.model_load(model.to_struct())
            t0 = time.perf_counter()
            ctx.model_specialize()
            t_spec = time.perf_counter() - t0
            ctx.replay_load(trace.original_externals, trace.events)
            n = len(trace.events)
            ctx.replay_wildcard_load(np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8))
            lim = T.Limits(0, 0, P_MAX, 1, fp.code, 0, 0, 0)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                ctx.replay_wildcard_batch(np.ones((64, n), dtype=bool), lim)
                ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.replay_wildcard_candidates(np.full((4, 4), ~np.uint64(0), dtype=np.uint64), [], lim)
            t_cand = time.perf_counter() - t0
            print("%s: demi_model_specialize %.2f s; first wildcard launch (compiles module 18) %.2f s, then %.2f ms; first candidates "
                  "launch (module 19) %.2f s" % (name, t_spec, ts[0], ts[-1] * 1e3, t_cand))
        finally:
            ctx.close()


if __name__ == "__main__":
    specialise()
    if "--shapes" in sys.argv:          # (with DEMI_EXPERIMENT=1 DEMI_K2_VERBOSE=1: the launch shapes per table, nothing else)
        sys.exit(0)
    for name in ("real5", "real3", "array5"):
        for spec in Pc.WORKLOADS[name][:2]:
            model, trace, fp = Pc.get(oracle, spec)
            minimizer("%s %s #%d" % (name, spec[0], spec[2]), model, trace, fp)
    ddmin()
