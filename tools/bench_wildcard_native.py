#!/usr/bin/env python
"""WildcardMinimizer as one native call (demi_minimize_wildcards) against the Python loop, on one GPU, on the
six workloads of profiles/wildcard_payloads.txt (tests/wildcard_payload_cases.py): ClockThenSingleton, LastOnlyStrategy, p_max 128.

  * per workload and loop shape (max_batch 16384 and 1): the Python loop and the native call on the same context, the first pass
    (which compiles the wildcard modules lazily) apart, then median and min..max of --repeat further passes; launches, sequential
    replays and replays run;
  * where the native call's time sits: one demi_replay_wildcard_round of 64 proposals against one demi_replay_wildcard_batch of
    the same rows (the launch and its read-back), and the call's time per launch.

On a tree without the native call (--python-only) only the Python loop is timed: the parent's figures, taken in the same job."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demi_amd import types as T                                            # noqa: E402
from demi_amd import wildcard_minimization as W                            # noqa: E402
from demi_amd.schedulers import MinimizationStats, SchedulerConfig         # noqa: E402
from oracle import oracle_py as oracle                                     # noqa: E402
from tests import wildcard_payload_cases as Pc                             # noqa: E402

P_MAX = 128


def summary(ts):
    return "median %.2f ms (min %.2f .. max %.2f of %d)" % (float(np.median(ts)), min(ts), max(ts), len(ts))


def one_pass(cfg, dev, trace, fp, max_batch, native):
    stats = MinimizationStats()
    dev.launches, dev.batches = 0, []
    kw = dict(native=True) if native else {}
    t0 = time.perf_counter()
    m = W.WildcardMinimizer(cfg, trace.original_externals, trace, fp, resolutionStrategy=W.LastOnlyStrategy(),
                            clusteringStrategy=W.ClusteringStrategy.ClockThenSingleton, stats=stats, max_batch=max_batch, oracle=dev, **kw)
    _, out = m.minimize()
    dt = (time.perf_counter() - t0) * 1e3
    return dt, dev.launches, stats.total_replays, m.speculative_replays, out


def workload(name, model, trace, fp, repeat, python_only):
    cfg = SchedulerConfig(model=model)
    dev = W.StsWildcardOracle(cfg, p_max=P_MAX)          # one context (the table compiled once) for every loop shape
    try:
        print("%s | %d externals, %d deliveries" % (name, len(trace.original_externals), int((trace.events["kind"] == T.REC_MSG_EVENT).sum())))
        for native in ((False,) if python_only else (False, True)):
            for max_batch in (16384, 1):
                first = one_pass(cfg, dev, trace, fp, max_batch, native)
                runs = [one_pass(cfg, dev, trace, fp, max_batch, native) for _ in range(repeat)]
                dt, launches, seq, run, out = runs[-1]
                extra = ""
                if native:
                    st = dev.native_stats
                    run = int(st.replays_run)
                    extra = ", %d rounds, %d adoptions, %.3f ms per launch" % (st.rounds, st.adoptions, float(np.median([r[0] for r in runs])) / max(1, launches))
                print("  %-6s max_batch %5d: %s, %d launches, %d sequential replays, %d replayed -> %d deliveries%s (first pass %.1f ms)"
                      % ("native" if native else "python", max_batch, summary([r[0] for r in runs]), launches, seq, run,
                         int((out.events["kind"] == T.REC_MSG_EVENT).sum()), extra, first[0]))
        if not python_only:
            # one round against one batch of the same 64 rows, selectors of the ClockClusterizer loaded
            c = W.ClockClusterizer(trace, model, W.LastOnlyStrategy())
            rows = []
            p = c.getNextTrace(False, frozenset())
            while p is not None and len(rows) < 64:
                rows.append(p)
                p = c.getNextTrace(False, frozenset())
            rows = np.array([rows[k % len(rows)] for k in range(64)])
            dev.load(trace, *c.selectors())
            lim = dev._limits(fp)
            tb, tr = [], []
            for _ in range(repeat + 1):
                t0 = time.perf_counter(); dev._ctx.replay_wildcard_batch(rows, lim); tb.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); dev._ctx.replay_wildcard_round(rows, lim); tr.append((time.perf_counter() - t0) * 1e3)
            print("  64 proposals: demi_replay_wildcard_batch %s; demi_replay_wildcard_round %s" % (summary(tb[1:]), summary(tr[1:])))
    finally:
        dev.shutdown()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--python-only", action="store_true", help="time only the Python loop (a tree without demi_minimize_wildcards)")
    args = ap.parse_args()
    for name in ("real5", "real3", "array5"):
        for spec in Pc.WORKLOADS[name][:2]:
            model, trace, fp = Pc.get(oracle, spec)
            workload("%s %s #%d" % (name, spec[0], spec[2]), model, trace, fp, max(5, args.repeat), args.python_only)
