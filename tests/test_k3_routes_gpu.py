"""Every route of the K3 host path once, small: the same exploration of apps.raft5_dpor_config3 (batch 64, 300 interleavings -
rounds smaller than, equal to and larger than one launch's width, the budget cutting the last round; interpreter only) through
each branch of demi_dpor_explore, and one demi_dpor_batch call with shared lengths.  What each route returns - verdicts, prefix
lengths, rounds, and the counters of demi_dpor_stats that say how often and how much the host talked to the device - is held
against tests/golden/k3_routes.json, recorded from the commit before the host path's launch, layout and growth code became one
function each: a copy of that code that drifts changes a launch count or a byte count here before it changes a
verdict anywhere."""
import hashlib
import json
import os

import numpy as np
import pytest

from demi_amd import types as T
from demi_amd.apps import raft5_dpor_config3

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k3_routes.json")
COUNTERS = ("launches", "interleavings", "executed", "fetches", "h2d_bytes", "d2h_bytes")
KNOBS = ("DEMI_DPOR_HOST_QUEUE", "DEMI_DPOR_HOST_BOOKKEEPING")
# route -> (exploration order, backtrack ordering, the knob that selects it)
ROUTES = {
    "rounds_device_queue": (T.DPOR_ORDER_ROUNDS, T.DPOR_ORDERING_DEFAULT, None),
    "rounds_host_queue": (T.DPOR_ORDER_ROUNDS, T.DPOR_ORDERING_DEFAULT, "DEMI_DPOR_HOST_QUEUE"),
    "rounds_host_bookkeeping": (T.DPOR_ORDER_ROUNDS, T.DPOR_ORDERING_DEFAULT, "DEMI_DPOR_HOST_BOOKKEEPING"),
    "reference_resident": (T.DPOR_ORDER_REFERENCE, T.DPOR_ORDERING_DEFAULT, None),
    "reference_host_bookkeeping": (T.DPOR_ORDER_REFERENCE, T.DPOR_ORDERING_DEFAULT, "DEMI_DPOR_HOST_BOOKKEEPING"),
    "ordered_arvind": (T.DPOR_ORDER_ROUNDS, T.DPOR_ORDERING_ARVIND, None),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def first_trace(ctx, par):
    """the trace of the first interleaving (empty next trace): ArvindDistanceOrdering's original trace, and what the batch cuts"""
    _, traces, _ = ctx.dpor_batch([np.zeros(0, dtype=T.DPOR_TRACE_DTYPE)], par)
    return traces[0]


def run_route(ctx, name):
    """One route on a context with the workload loaded -> what the golden file holds for it."""
    _, _, par = raft5_dpor_config3()
    for k in KNOBS:
        os.environ.pop(k, None)
    if name == "batch_shared_len":
        tr = first_trace(ctx, par)
        n = len(tr)
        cuts = [0, 1, n // 3, n // 2, n - 1]
        shared = [0, 0, n // 3, n // 4, n - 2]
        v, traces, pairs = ctx.dpor_batch([tr[:c] for c in cuts], par, shared)
        return {"verdicts": sha(v), "flags": [int(x) for x in v["flags"]], "trace_len": [len(t) for t in traces],
                "n_pairs": [len(p) for p in pairs], "traces": [sha(t) for t in traces], "pairs": [sha(p) for p in pairs]}
    order, ordering, knob = ROUTES[name]
    ctx.dpor_set_traces(first_trace(ctx, par) if ordering == T.DPOR_ORDERING_ARVIND else None, None)
    if knob:
        os.environ[knob] = "1"
    try:
        v, plen, rounds, _, st = ctx.dpor_explore(par, T.DporSearch(64, 300, 0, 1, order, 0, ordering))
    finally:
        if knob:
            del os.environ[knob]
        ctx.dpor_set_traces(None, None)
    out = {"verdicts": sha(v), "n_verdicts": len(v), "violating": int(np.count_nonzero(v["flags"] & T.V_VIOLATION)),
           "prefix_len": [int(x) for x in plen], "rounds": [int(x) for x in rounds]}
    out.update({c: int(getattr(st, c)) for c in COUNTERS})
    return out


@pytest.fixture(scope="module")
def routes_ctx():
    from demi_amd import _native
    model, ev, _ = raft5_dpor_config3()
    ctx = _native.Context(0)
    ctx.model_load(model.to_struct())
    ctx.dpor_load(ev)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(ROUTES) + ["batch_shared_len"])
def test_every_route_of_the_k3_host_path_returns_what_it_returned_before(routes_ctx, golden, name, monkeypatch):
    monkeypatch.setenv("DEMI_EXPERIMENT", "1")
    got = run_route(routes_ctx, name)
    want = golden["routes"][name]
    unstable = set(golden["unstable"].get(name, []))
    assert unstable <= set(COUNTERS)                       # (only counters may be left out, never a verdict, a length or a round)
    assert set(got) == set(want) | unstable
    for k in want:
        assert got[k] == want[k], (name, k, got[k], want[k])
    if name != "batch_shared_len":
        # (the budget cuts the last round; the REFERENCE order also runs interleavings its commit does not take)
        assert got["n_verdicts"] == got["interleavings"] == len(got["prefix_len"]) == 300 and sum(got["rounds"]) == got["executed"]
