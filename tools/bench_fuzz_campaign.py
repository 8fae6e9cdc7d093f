"""Campaign rate of runner_utils.fuzz_campaign against fuzz()'s shape (one launch per test, Python generation), DESIGN section 0.8.

Config 2's table without its seeded bug (nothing violates: both drivers run every test), 50-event tests (10-event prefix + 40
generated), executions per test 1 / 64 / 4096, the same test and execution seeds for both drivers, the two interleaved, two rounds.
Then what share of a campaign launch is k_fuzz_generate and what share is K1 (each timed alone over the same tests).

    python tools/bench_fuzz_campaign.py [--out profiles/fuzz_campaign.txt] [--specialize]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from demi_amd import _native, fuzzer as F, types as T          # noqa: E402
from demi_amd.model import M_BOOTSTRAP, raft_model             # noqa: E402
from demi_amd.runner_utils import fuzz, fuzz_campaign           # noqa: E402
from demi_amd.schedulers import SchedulerConfig                 # noqa: E402

TEST_SEED, NUM_EVENTS = 0xF0220000, 40
#        executions per test, tests of the campaign, tests per launch, tests of the one-launch-per-test driver
SHAPES = [(1, 8192, 2048, 128), (64, 2048, 1024, 128), (4096, 256, 128, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--specialize", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    model = raft_model(5, buggy=False)
    sc = SchedulerConfig(model=model)
    prefix = [F.start(i) for i in range(5)] + [F.send(i, M_BOOTSTRAP) for i in range(5)]
    w, gen = F.FuzzerWeights(), F.raft_send_generator()
    args = (NUM_EVENTS, w, gen, prefix)
    kw = dict(maxMessages=200, invariant_check_interval=30)
    say("# fuzz_campaign vs fuzz(): raft5 table (no seeded bug), %d-event tests, specialize=%s" % (len(prefix) + NUM_EVENTS, a.specialize))
    fuzz_campaign(args, sc, executions_per_test=1, max_tests=64, tests_per_launch=64, test_seed_base=TEST_SEED, specialize=a.specialize, **kw)   # warm-up
    for epc, n_camp, tpl, n_one in SHAPES:
        for rnd in range(2):
            t0 = time.perf_counter()
            r = fuzz(lambda i: F.events_to_array(F.generate_fuzz_test(NUM_EVENTS, w, gen, prefix, TEST_SEED + i)), sc,
                     executions_per_test=epc, max_tests=n_one, **kw)
            t1 = time.perf_counter()
            c = fuzz_campaign(args, sc, executions_per_test=epc, max_tests=n_camp, tests_per_launch=tpl, test_seed_base=TEST_SEED,
                              specialize=a.specialize, **kw)
            t2 = time.perf_counter()
            assert r is None and c is None
            one, camp = n_one / (t1 - t0), n_camp / (t2 - t1)
            say("epc=%d round=%d  fuzz(): %d tests %.3f s = %.1f tests/s %.3e executions/s | fuzz_campaign: %d tests (%d per launch) %.3f s = "
                "%.1f tests/s %.3e executions/s | ratio %.1f" % (epc, rnd, n_one, t1 - t0, one, one * epc, n_camp, tpl, t2 - t1, camp, camp * epc, camp / one))
    # the two halves of a campaign launch, each alone
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    if a.specialize:
        ctx.model_specialize()
    lim = T.Limits(200, 30, 64, 0, 0, 0)
    for epc, _, tpl, _ in SHAPES:
        ctx.fuzz_generate(tpl, NUM_EVENTS, w, gen, prefix, seed_base=TEST_SEED, copy_out=False)
        ctx.random_explore_tests(None, epc, lim, n_tests=tpl)
        reps = 10
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.fuzz_generate(tpl, NUM_EVENTS, w, gen, prefix, seed_base=TEST_SEED, copy_out=False)
        t1 = time.perf_counter()
        for _ in range(reps):
            ctx.random_explore_tests(None, epc, lim, n_tests=tpl)
        t2 = time.perf_counter()
        g, k = (t1 - t0) / reps, (t2 - t1) / reps
        say("epc=%d tests_per_launch=%d  fuzz_generate %.3f ms (%.1f%%)  random_explore_tests %.3f ms (%.1f%%; verdicts copied out)"
            % (epc, tpl, g * 1e3, 100 * g / (g + k), k * 1e3, 100 * k / (g + k)))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
