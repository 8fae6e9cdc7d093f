"""What tests/test_wildcard_dpor_cpu.py and tests/test_wildcard_dpor_gpu.py share: the hand-made table and the comparison of a
K3W launch with the transliteration's interleavings."""
import numpy as np

from demi_amd import model as M
from demi_amd import types as T
from demi_amd.fuzzer import events_to_array, send, start
from demi_amd.model import Asm, build_model

from . import test_wildcard_transliteration_cpu as X
from . import wildcard_dpor_transliteration as D

GO, WMSG = 0, 1
BACKTRACK_OF = {"SrcDstFIFOOnly": T.WILDCARD_BACKTRACK_NONE, "BackTrackStrategy": T.WILDCARD_BACKTRACK_ALL,
                "FirstAndLastBacktrack": T.WILDCARD_BACKTRACK_LAST_DISTINCT, "LastOnlyStrategy": T.WILDCARD_BACKTRACK_NONE}


def first_writer_model(n_payloads=2, wide=False):
    """Three actors.  Go makes actor 0 send W(1), W(2), ... W(n) to actor 1, which keeps the payload of the FIRST W it gets; the
    invariant fails only if that is 2 - so only if W(2) is delivered before W(1).  Actor 2 takes no part."""
    msgs = [("Go", T.MSG_EXTERNAL), ("W", T.MSG_INTERNAL)]
    go = Asm().mov(M.T1, 1)
    for k in range(1, n_payloads + 1):
        go = go.mov(M.T0, k).send(WMSG, M.T1, M.T0)
    h = {(0, "Go"): go, (0, "W"): Asm().skipnz(M.F[1], "seen").mov(M.F[0], M.P0).label("seen").add(M.F[1], M.F[1], 1)}
    return build_model("firstwriter", 3, msgs, h, [[0] * 8] * 3, (T.INV_NEVER, 0, 2, 0), wide=wide)


def first_writer_externals(gos=1):
    """gos: how many Go(g) are sent (g = 0, 1, ...: distinct messages, so the W's of each are nodes of their own)."""
    return events_to_array([start(a) for a in range(3)] + [send(0, GO, g) for g in range(gos)])


def first_writer_uniques(strategy, n_payloads=2, gos=1):
    """The proposal: the exact delivery of every Go, then one class-tag wildcard per W."""
    strat = X.STRATEGIES[strategy][0]()
    return [D.ProposalUnique(("msg", T.DEADLETTERS, 0, (GO, g, 0)), g) for g in range(gos)] + \
           [D.ProposalUnique(("msg", 0, 1, X.class_tag_wildcard(WMSG, strat)), gos + k) for k in range(n_payloads * gos)]


def first_writer_selector(strategy):
    mirror = X.STRATEGIES[strategy][1]()
    return lambda rec: (1 << WMSG, mirror.policy, BACKTRACK_OF[strategy])


def first_writer_test(oracle, strategy, n_payloads=2, dpor_budget=0, wide=False, gos=1):
    d = D.ScalaWildcardDPOR(oracle, first_writer_model(n_payloads, wide), first_writer_externals(gos), first_writer_uniques(strategy, n_payloads, gos),
                            None, dpor_budget=dpor_budget)
    return d, d.test()


def selector_of(clusterizer_mirror):
    ts, po = clusterizer_mirror.selectors()
    bt = clusterizer_mirror.backtracks()
    return lambda rec: (int(ts[rec]), int(po[rec]), int(bt[rec]))


def compare_launch(ctx, dpor, records, selector, par, max_alts=64):
    """The interleavings `records` of the transliteration `dpor` through demi_dpor_wildcard_batch in ONE launch: verdict triple,
    trace entries, ignored positions, picked-by-wildcard marks and alternative records in order, bit for bit."""
    nexts = [D.next_trace_entries(dpor, r["next"], selector) for r in records]
    v, traces, ignored, wild, alts = ctx.dpor_wildcard_batch(nexts, par, stop_after_next_trace=True, max_alts=max_alts)
    assert not (v["flags"] & (T.V_PENDING_OVF | T.V_QUEUE_OVF | T.V_TRACE_OVF | T.V_ALTS_OVF | T.V_SELFMSG)).any()
    for k, r in enumerate(records):
        assert (int(v["flags"][k]), int(v["fingerprint"][k]), int(v["hash"][k])) == r["verdict"], (k, r["verdict"])
        assert len(traces[k]) == len(r["trace"]) and traces[k].tobytes() == r["trace"].tobytes(), k
        assert ignored[k] == sorted(r["ignored"]), k
        assert wild[k] == sorted(r["wild"]), k
        want = np.array([(key, word, tl, pos, par_) for key, word, tl, pos, par_ in r["alts"]], dtype=T.DPOR_WILD_ALT_DTYPE) \
            if r["alts"] else np.zeros(0, dtype=T.DPOR_WILD_ALT_DTYPE)
        assert len(alts[k]) == len(want) and alts[k].tobytes() == want.tobytes(), (k, alts[k], want)
    return v
