#!/usr/bin/env python
"""The "Wildcards" stage - WildcardMinimizer with DPORwHeuristics as its oracle - on one GPU: one pass per
test workload (tests/test_wildcard_transliteration_cpu.py raft5_workload, election budget 2; ClockClusterizer, BackTrackStrategy,
p_max 128, dpor_budget 16)

  * in the reference's loop shape (batch = 1: one interleaving per launch) and with the speculative frontier (batch = 64),
  * interpreted and specialised (the first pass, which compiles the module lazily, apart),

with launches, committed and speculated interleavings and ms per pass.  Writes profiles/wildcard_dpor.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from demi_amd import types as T                                            # noqa: E402
from demi_amd import wildcard_minimization as W                            # noqa: E402
from demi_amd.schedulers import MinimizationStats, SchedulerConfig         # noqa: E402
from oracle import oracle_py as oracle                                     # noqa: E402
from tests import test_wildcard_transliteration_cpu as X                   # noqa: E402

P_MAX, BUDGET = 128, 16


def one_pass(cfg, dev, trace, fp, batch):
    dev.launches = dev.interleavings = dev.speculated = 0
    dev.batch = batch
    stats = MinimizationStats()
    t0 = time.perf_counter()
    m = W.WildcardMinimizer(cfg, trace.original_externals, trace, fp, stats=stats, oracle=dev, testScheduler=W.TestScheduler.DPORwHeuristics)
    _, out = m.minimize()
    dt = (time.perf_counter() - t0) * 1e3
    return dt, stats.total_replays, dev.launches, dev.interleavings, dev.speculated, int((out.events["kind"] == T.REC_MSG_EVENT).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wildcard_dpor.txt"))
    a = ap.parse_args()
    oracle.build()
    lines = ["tools/bench_wildcard_dpor.py: one Wildcards pass per workload, ClockClusterizer, BackTrackStrategy, p_max %d, dpor_budget %d" % (P_MAX, BUDGET)]
    for skip in X.WORKLOAD_SKIPS:
        model, trace, fp = X.raft5_workload(oracle, skip, **X.WORKLOAD_MODEL)
        cfg = SchedulerConfig(model=model)
        lines.append("raft5 workload %d | %d externals, %d deliveries" % (skip, len(trace.original_externals), int((trace.events["kind"] == T.REC_MSG_EVENT).sum())))
        for specialise in (False, True):
            dev = W.DporWildcardOracle(cfg, p_max=P_MAX, dpor_budget=BUDGET, specialize=specialise)
            try:
                for batch in (1, 64):
                    first = one_pass(cfg, dev, trace, fp, batch)
                    runs = [one_pass(cfg, dev, trace, fp, batch) for _ in range(a.repeat)]
                    ts = [r[0] for r in runs]
                    _, proposals, launches, committed, speculated, left = runs[-1]
                    lines.append("  %-11s batch %2d: median %.1f ms (min %.1f .. max %.1f of %d; first pass %.1f ms), %d proposals, %d launches, "
                                 "%d committed + %d speculated interleavings, %.3f ms per launch -> %d deliveries"
                                 % ("specialised" if specialise else "interpreted", batch, float(np.median(ts)), min(ts), max(ts), len(ts), first[0],
                                    proposals, launches, committed, speculated, float(np.median(ts)) / max(1, launches), left))
            finally:
                dev.shutdown()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
