"""Campaign rate on a DEMI_MODEL_PAYLOADS table: raft_model(5, log_cap=8, real_fields=True) without its seeded
bug (nothing violates: every test runs), 50-event tests (10-event prefix + 40 generated ClientCommands with all five fields
described), ONE specialised context for everything.

Per shape (executions per test 1 and 4096): the campaign (Context.fuzz_campaign with a FieldSendGenerator: demi_fuzz_campaign_fields)
against the loop a user of such a table had before - a mirror-generated test (fuzzer.generate_fuzz_test_fields), trace_load(events,
areas), random_explore - on the same test and execution seeds, the two interleaved, two rounds.  Then the two halves of a campaign
launch, each timed alone over the same tests: k_fuzz_generate_fields (events and areas) and K1 with a workgroup per test.

    python tools/bench_fuzz_campaign_fields.py [--out profiles/fuzz_campaign_fields.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from demi_amd import _native, fuzzer as F, types as T          # noqa: E402
from demi_amd.model import M_BOOTSTRAP, M_CLIENT, raft_model    # noqa: E402

TEST_SEED, NUM_EVENTS = 0xF0220000, 40
#        executions per test, tests of the campaign, tests per launch, tests of the one-launch-per-test loop
SHAPES = [(1, 8192, 2048, 128), (4096, 256, 128, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tiny", action="store_true", help="a few tests per shape: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    shapes = [(1, 8, 4, 2), (8, 4, 2, 2)] if a.tiny else SHAPES
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    model = raft_model(5, buggy=False, log_cap=8, real_fields=True)
    prefix = [F.start(i) for i in range(5)] + [F.send(i, M_BOOTSTRAP) for i in range(5)]
    w = F.FuzzerWeights()
    gen = F.FieldSendGenerator([(M_CLIENT, F.RANDOM_ALIVE, [F.COUNTER, F.CONST(0), F.RANDOM(13), F.RANDOM(200), F.CONST(511)])], model)
    lim = T.Limits(200, 30, 64, 0, 0, 0)
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    t0 = time.perf_counter()
    ctx.model_specialize()
    ctx.fuzz_campaign(NUM_EVENTS, w, gen, prefix, lim, executions_per_test=1, tests_per_launch=64, max_tests=64, test_seed_base=TEST_SEED)   # warm-up
    ctx.trace_load(*_mirror(gen, w, prefix, 0))
    ctx.random_explore(64, lim, seed_base=0)
    say("# fuzz_campaign (FieldSendGenerator) vs the host loop: raft5 with akka-raft's field sets (DEMI_MODEL_PAYLOADS(5), log_cap 8, no seeded "
        "bug), %d-event tests; compiling K1, K1 TESTS and the warm-up: %.2f s, once" % (len(prefix) + NUM_EVENTS, time.perf_counter() - t0))
    for epc, n_camp, tpl, n_one in shapes:
        for rnd in range(2):
            t0 = time.perf_counter()
            hits = 0
            for i in range(n_one):
                ev, ar = _mirror(gen, w, prefix, i)
                ctx.trace_load(ev, ar)
                hits += int((ctx.random_explore(epc, lim, seed_base=0)["flags"] & T.V_VIOLATION).any())
            t1 = time.perf_counter()
            res, _, _ = ctx.fuzz_campaign(NUM_EVENTS, w, gen, prefix, lim, executions_per_test=epc, tests_per_launch=tpl, max_tests=n_camp,
                                          test_seed_base=TEST_SEED)
            t2 = time.perf_counter()
            assert hits == 0 and not res.found and res.tests_run == n_camp
            one, camp = n_one / (t1 - t0), n_camp / (t2 - t1)
            say("epc=%d round=%d  host loop: %d tests %.3f s = %.1f tests/s %.3e executions/s | fuzz_campaign: %d tests (%d per launch) %.3f s = "
                "%.1f tests/s %.3e executions/s (%d tests with an execution beyond p_max) | ratio %.1f"
                % (epc, rnd, n_one, t1 - t0, one, one * epc, n_camp, tpl, t2 - t1, camp, camp * epc, res.capacity_aborts, camp / one))
    # the two halves of a campaign launch, each alone
    for epc, _, tpl, _ in shapes:
        ctx.fuzz_generate(tpl, NUM_EVENTS, w, gen, prefix, seed_base=TEST_SEED, copy_out=False)
        ctx.random_explore_tests(None, epc, lim, n_tests=tpl, with_areas=True)
        reps = 10
        t0 = time.perf_counter()
        for _ in range(reps):
            ctx.fuzz_generate(tpl, NUM_EVENTS, w, gen, prefix, seed_base=TEST_SEED, copy_out=False)
        t1 = time.perf_counter()
        for _ in range(reps):
            ctx.random_explore_tests(None, epc, lim, n_tests=tpl, with_areas=True)
        t2 = time.perf_counter()
        g, k = (t1 - t0) / reps, (t2 - t1) / reps
        say("epc=%d tests_per_launch=%d  fuzz_generate (fields: events and areas) %.3f ms (%.1f%%)  random_explore_tests %.3f ms (%.1f%%; verdicts copied out)"
            % (epc, tpl, g * 1e3, 100 * g / (g + k), k * 1e3, 100 * k / (g + k)))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _mirror(gen, w, prefix, i):
    import numpy as np
    ev, ar = F.generate_fuzz_test_fields(NUM_EVENTS, w, gen, prefix, TEST_SEED + i)
    return F.events_to_array(ev), np.array(ar, dtype=np.uint64)


if __name__ == "__main__":
    main()
