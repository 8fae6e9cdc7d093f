"""GPU suite: the payload areas of a DEMI_MODEL_PAYLOADS table's external Sends through the DPOR-based minimizers -
demi_edit_distance_dpor_ddmin (areas staged with demi_ext_payload_areas are the areas of its externals: kept for the call,
gathered for every subsequence it consults), DPORwHeuristics.test(areas=) and editDistanceDporDDMin(trace with ext_areas) on its
three paths - against the Python loop over the CPU oracle given the same areas per subsequence.  The workload is the ledger
table of tests/test_payloads_gpu.py: the invariant is decided by the fourth field of one external Send."""
import numpy as np
import pytest

from demi_amd import _native
from demi_amd import types as T
from demi_amd.dpor import ArvindDistanceOrdering, DPORwHeuristics
from demi_amd.incremental_ddmin import dpor_initial_trace, editDistanceDporDDMin
from demi_amd.schedulers import EventTrace, SchedulerConfig

from . import wildcard_payload_cases as Pc

pytestmark = pytest.mark.gpu

KW = dict(stopAtSize=1, maxMaxDistance=4, batch=8)
_ref = {}


def _workload(oracle):
    if "w" not in _ref:
        model, events, areas = Pc.ledger_workload()
        trace, fp = Pc.ledger_execution(oracle, model, events, areas)
        _ref["w"] = (model, events, areas, trace, fp)
    return _ref["w"]


def _oracle_loop(oracle, with_areas):
    """editDistanceDporDDMin's Python loop over the oracle backend, once per flavour."""
    if with_areas not in _ref:
        model, events, areas, trace, fp = _workload(oracle)
        t = trace if with_areas else EventTrace(trace.events, events)
        _ref[with_areas] = editDistanceDporDDMin(SchedulerConfig(model=model), t, fp, backend=Pc.oracle_backend_with_areas(oracle), **KW)
    return _ref[with_areas]


def _native_call(ctx, model, events, trace, fp, areas):
    init = dpor_initial_trace(trace, model)
    par = T.DporParams(0, len(init), 1, fp.code, 64, 4096, 1)
    ip = T.IncDdminParams(max_max_distance=KW["maxMaxDistance"], stop_at_size=KW["stopAtSize"], check_unmodified=0, ignore_quiescence=1,
                          verify_mcs=1, batch=KW["batch"])
    return ctx.edit_distance_dpor_ddmin(events, init, par, ip, areas=areas)


def _same(native, loop):
    mcs, consulted, passes, vtrace, st = native
    w_mcs, w_dd, w_verified, _ = loop
    assert tuple(mcs) == tuple(w_mcs) and passes == w_dd.distances
    assert [(tuple(c), p, d) for c, p, d in consulted] == [(tuple(c), p, d) for c, p, d in w_dd.consulted_all]
    assert int(st.replays) == w_dd._stats.total_replays
    assert (vtrace is not None) == (w_verified is not None)
    if w_verified is not None:
        assert len(vtrace) == len(w_verified) and (vtrace["key"] == w_verified["key"]).all() and (vtrace["word"] == w_verified["word"]).all()


def test_staged_areas_reach_every_consultation_of_the_native_ddmin(oracle):
    model, events, areas, trace, fp = _workload(oracle)
    want, without = _oracle_loop(oracle, True), _oracle_loop(oracle, False)
    assert want[2] is not None and tuple(want[0]) != tuple(without[0])          # (the areas decide the answer: asserted on the oracle)
    ctx = _native.Context(0)
    try:
        ctx.model_load(model.to_struct())
        ctx.model_specialize()
        _same(_native_call(ctx, model, events, trace, fp, areas), want)
        # staged through the C entry point itself, not the keyword: the same
        ctx.ext_payload_areas(areas)
        _same(_native_call(ctx, model, events, trace, fp, None), want)
        # nothing staged (the call above consumed them): P0 / P1 of every Send, fields 2 and up zero
        _same(_native_call(ctx, model, events, trace, fp, None), without)
        # a count mismatch is refused by name, with both numbers, and leaves nothing staged
        with pytest.raises(_native.DemiError, match=r"staged %d areas for the %d external events" % (len(events) - 2, len(events))):
            _native_call(ctx, model, events, trace, fp, areas[:-2])
        _same(_native_call(ctx, model, events, trace, fp, None), without)
    finally:
        ctx.close()


def test_dpor_test_with_areas_on_the_device_equals_the_oracle_backend(oracle):
    model, events, areas, trace, fp = _workload(oracle)
    init = dpor_initial_trace(trace, model)
    sub = [i for i in range(len(events)) if i != 2]           # (a subsequence: the gathered areas, not a prefix of them)
    answers = []
    for backend, native in ((Pc.oracle_backend_with_areas(oracle), False), (None, False), (None, True)):
        for ar in (areas[sub], None):
            h = ArvindDistanceOrdering()
            d = DPORwHeuristics(SchedulerConfig(model=model), prioritizePendingUponDivergence=True, backtrackHeuristic=h, batch=8,
                                backend=backend, native=native)
            d.setMaxMessagesToSchedule(len(init)); d.setInitialTrace(init); h.init(d, init); d.setMaxDistance(4)
            try:
                got = d.test(events[sub], fp, areas=ar)
            finally:
                d.shutdown()
            answers.append(None if got is None else (got["key"].tobytes(), got["word"].tobytes()))
    assert answers[0] is not None and answers[1] is None
    assert answers[2:4] == answers[0:2] and answers[4:6] == answers[0:2]


@pytest.mark.parametrize("path", ["python_loop", "native", "native_loop"])
def test_edit_distance_dpor_ddmin_with_ext_areas_on_its_three_paths(oracle, path):
    """(a case per path: every DPORwHeuristics instance of the first two compiles the table for its own context)"""
    model, events, areas, trace, fp = _workload(oracle)
    want = _oracle_loop(oracle, True)
    cfg = SchedulerConfig(model=model)
    if path == "native_loop":
        n_mcs, n_dd, n_verified, _ = editDistanceDporDDMin(cfg, trace, fp, native_loop=True, **KW)
        assert tuple(n_mcs) == tuple(want[0]) and n_dd.distances == want[1].distances
        assert n_dd.consulted_all == [(tuple(c), p, d) for c, p, d in want[1].consulted_all]
        assert n_dd._stats.total_replays == want[1]._stats.total_replays
        assert n_verified is not None and (n_verified["key"] == want[2]["key"]).all()
        return
    mcs, dd, verified, _ = editDistanceDporDDMin(cfg, trace, fp, native=(path == "native"), **KW)
    assert tuple(mcs) == tuple(want[0]) and dd.consulted_all == want[1].consulted_all and dd.distances == want[1].distances
    assert dd._stats.total_replays == want[1]._stats.total_replays
    assert verified is not None and (verified["key"] == want[2]["key"]).all()
