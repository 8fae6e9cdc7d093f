"""Campaign rate of demi_fuzz_campaign_pipelined against the synchronous demi_fuzz_campaign, DESIGN section 0.16.

Config 2's table without its seeded bug (nothing violates: every launch of the campaign runs), 50-event tests (10-event prefix + 40
generated), section 0.8's three shapes (executions per test / tests per launch: 1 / 2048, 64 / 1024, 4096 / 128), table interpreted
and specialised.  Per shape the synchronous campaign (in_flight=None: unchanged code) is interleaved with in_flight = 1, 2, 3 in
this one process, two rounds; the spread between the synchronous path's two rounds is the margin for "not slower".  Reported: ms
per launch, tests/s, launches_discarded.

This process creates no stream but the library's own; GPU_MAX_HW_QUEUES is set to 8 before the runtime starts when the caller
has not set it (the library's two streams must not share a hardware queue).

    python tools/bench_fuzz_pipeline.py [--out profiles/fuzz_pipeline.txt] [--launches 8]
"""
import argparse
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
os.environ.setdefault("DEMI_NO_TORCH", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from demi_amd import _native, fuzzer as F, types as T          # noqa: E402
from demi_amd.model import M_BOOTSTRAP, raft_model             # noqa: E402

TEST_SEED, NUM_EVENTS = 0xF0220000, 40
SHAPES = [(1, 2048), (64, 1024), (4096, 128)]                  # executions per test, tests per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=8)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    model = raft_model(5, buggy=False)
    prefix = [F.start(i) for i in range(5)] + [F.send(i, M_BOOTSTRAP) for i in range(5)]
    args = (NUM_EVENTS, F.FuzzerWeights(), F.raft_send_generator(), prefix)
    lim = T.Limits(200, 30, 64, 0, 0, 0)
    say("# demi_fuzz_campaign_pipelined vs demi_fuzz_campaign: raft5 table (no seeded bug), %d-event tests, %d launches per campaign, "
        "GPU_MAX_HW_QUEUES=%s, no stream but the library's" % (len(prefix) + NUM_EVENTS, a.launches, os.environ["GPU_MAX_HW_QUEUES"]))
    for specialize in (False, True):
        ctx = _native.Context(0)
        ctx.model_load(model.to_struct())
        if specialize:
            ctx.model_specialize()
        for epc, tpl in SHAPES:
            n = tpl * a.launches
            kw = dict(executions_per_test=epc, tests_per_launch=tpl, max_tests=n, test_seed_base=TEST_SEED)
            for in_flight in (None, 3):                      # warm-up: buffers, the compiled kernels
                ctx.fuzz_campaign(*args, lim, in_flight=in_flight, **dict(kw, max_tests=min(n, 2 * tpl)))
            sync = []
            for rnd in range(2):
                for in_flight in (None, 1, 2, 3):
                    t0 = time.perf_counter()
                    res, ev = ctx.fuzz_campaign(*args, lim, in_flight=in_flight, **kw)
                    dt = time.perf_counter() - t0
                    assert not res.found and res.launches == a.launches and res.tests_run == n
                    disc = ctx.fuzz_pipeline_stats.launches_discarded if in_flight else 0
                    if in_flight is None:
                        sync.append(dt)
                    say("specialize=%d epc=%d tests_per_launch=%d round=%d in_flight=%s  %.3f ms per launch  %.1f tests/s  %.3e executions/s  "
                        "discarded=%d  vs synchronous (this round) %.3f" % (specialize, epc, tpl, rnd, in_flight, 1e3 * dt / a.launches, n / dt,
                                                                            n * epc / dt, disc, sync[rnd] / dt))
            say("specialize=%d epc=%d  synchronous rounds %.3f / %.3f ms per launch: spread %.1f%%"
                % (specialize, epc, 1e3 * sync[0] / a.launches, 1e3 * sync[1] / a.launches, 100 * abs(sync[0] - sync[1]) / min(sync)))
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
