"""Internal-event minimization of config 4's verified MCS execution: the Python loop around demi_replay_removal_batch /
demi_replay_get_kept (minimizeInternals(native=False)) against the one native call (native=True: demi_minimize_internals),
DESIGN section 4.

The workload of tools/bench_k2k3.py: config 4's first violating execution, DDMin, the verified MCS execution.  Both removal
strategies; one warm-up of each path, then five repetitions of each, interleaved, on one replay oracle (one context: model load and
kernel selection are outside the timing for both); medians.  For the native path also rounds, launches and replays_run.

    python tools/bench_intmin.py [--out profiles/intmin_native.txt] [--reps 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from demi_amd import _native, internal_minimization as IM, types as T          # noqa: E402
from demi_amd.apps import SEED_BASE, raft5_config4                              # noqa: E402
from demi_amd.minification import stsSchedDDMin                                 # noqa: E402
from demi_amd.schedulers import EventTrace, STSScheduler, SchedulerConfig, ViolationFingerprint   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    model, events, lim = raft5_config4()
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct()); ctx.trace_load(events)
    v = ctx.random_explore(4000, lim, seed_base=SEED_BASE)
    i = int(np.nonzero(v["flags"] & T.V_VIOLATION)[0][0])
    vv, rec = ctx.random_get_trace(SEED_BASE + i, lim)
    ctx.close()
    used = events[:T.verdict_trace_idx(vv.flags)]
    fp = ViolationFingerprint(vv.fingerprint)
    cfg = SchedulerConfig(model=model)
    sts = STSScheduler(cfg, EventTrace(rec, used), p_max=128)
    mcs, _, _ = stsSchedDDMin(sts, used, fp, speculative_depth=4)
    verified = sts.executed_trace(mcs, fp)
    sts.shutdown()
    say("# internal minimization, config 4's verified MCS execution: %d externals, %d recorded events, %d deliveries; %d repetitions after one warm-up"
        % (len(verified.original_externals), len(verified.events), IM.countMsgEvents(verified), a.reps))
    for name in ("LeftToRightOneAtATime", "SrcDstFIFORemoval"):
        orc = IM.StsRemovalOracle(cfg, p_max=128)
        ctor = lambda: getattr(IM, name)(verified, model)                        # noqa: E731

        def run(native):
            t = time.perf_counter()
            st, tr = IM.minimizeInternals(cfg, verified.original_externals, verified, fp, removalStrategyCtor=ctor, oracle=orc, native=native)
            return time.perf_counter() - t, st, tr
        (_, s0, t0), (_, s1, t1) = run(False), run(True)                         # warm-up; the two paths agree
        assert t0.events.tobytes() == t1.events.tobytes() and s0.total_replays == s1.total_replays
        py, nat = [], []
        for _ in range(a.reps):
            py.append(run(False)[0])
            nat.append(run(True)[0])
        ns = orc.native_stats
        mp, mn = statistics.median(py), statistics.median(nat)
        say("%s: %d -> %d deliveries, %d sequential replays | python loop median %.3f ms (min %.3f, max %.3f) | native median %.3f ms "
            "(min %.3f, max %.3f): rounds %d, launches %d, replays_run %d, adoptions %d | python / native = %.2f"
            % (name, IM.countMsgEvents(verified), IM.countMsgEvents(t1), s1.total_replays, mp * 1e3, min(py) * 1e3, max(py) * 1e3, mn * 1e3,
               min(nat) * 1e3, max(nat) * 1e3, ns.rounds, ns.launches, ns.replays_run, ns.adoptions, mp / mn))
        orc.shutdown()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
