"""CPU suite of the fuzz campaign for messages with more than two fields: the host mirror alone (fuzzer.FieldSendGenerator and
generate_fuzz_test_fields, the mirror of k_fuzz_generate_fields) and the conditions the GPU suite's cases must contain, asserted
on the mirror and the oracle."""
import ctypes

import numpy as np
import pytest

from demi_amd import fuzzer as F, model as M, types as T

from . import fuzz_campaign_cases as FC
from . import fuzz_fields_cases as FF


def _as_fields(gen, model):
    """a SendGenerator's alternatives as two-field alternatives of a FieldSendGenerator"""
    return F.FieldSendGenerator([(m, t, [p0, p1]) for m, t, p0, p1 in gen.alternatives], model)


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("name", [c.name for c in FC.CONFIGS])
def test_two_field_alternatives_yield_the_old_generators_events(name, explicit):
    """(a) the draw order with two fields per alternative is SendGenerator's: every configuration and seed set of the campaign's
    own suite, event for event; a table without DEMI_MODEL_PAYLOADS has no areas"""
    cfg = {c.name: c for c in FC.CONFIGS}[name]
    seeds = FC.explicit_seeds() if explicit else [FC.SEED_BASE + i for i in range(FC.N_TESTS)]
    want = FC.mirror_tests(name, explicit)
    gen = _as_fields(cfg.gen(), M.raft_model(cfg.n_actors))
    for i, s in enumerate(seeds):
        ev, ar = F.generate_fuzz_test_fields(cfg.num_events, cfg.weights, gen, cfg.prefix, s, cfg.postfix)
        assert tuple(ev) == want[i], (name, i)
        assert len(ar) == len(ev) and not any(ar)


def test_hand_packed_areas_for_every_field_count():
    """(b) known answers: one generated Send per field count, its area packed by hand at the table's width"""
    class Rng:
        def next_int(self, bound):
            return bound - 1
    for npay, w in ((3, 16), (4, 12), (5, 9), (6, 8)):
        model = FF.pay_table(npay)
        assert F.model_field_layout(model) == (npay, w) == (model.payloads, T.payload_bits(npay))
        top = (1 << w) - 1
        fields = [F.CONST(5), F.CONST(top), F.RANDOM(13), F.CONST(1), F.COUNTER, F.RANDOM(200)][:npay]
        vals = [5, top, 12, 1, 1, 199][:npay]
        g = F.FieldSendGenerator([(0, F.FIXED(3), fields)], model)
        assert g(Rng(), None) == F.send(3, 0, 5, top) and g.sent == [vals]
        by_hand = 0
        for k, v in enumerate(vals):
            by_hand |= v << (k * w)
        assert g.area(vals) == by_hand == T.pay_area(vals, npay)
        assert [T.payload_fields(by_hand, npay)[k] for k in range(npay)] == vals
        # the neighbours of the field at 2^W - 1 keep their bits; an alternative shorter than the table leaves the rest 0
        assert (by_hand >> w) & top == top and by_hand & top == 5 and (by_hand >> (2 * w)) & top == 12
        short = F.FieldSendGenerator([(0, F.FIXED(3), fields[:2])], model)
        short(Rng(), None)
        assert short.area(short.sent[0]) == 5 | (top << w)
    # without DEMI_MODEL_PAYLOADS: 8 bits (narrow) or 16 (wide), two fields, no area
    assert F.model_field_layout(M.raft_model(5)) == (2, 8) and F.model_field_layout(M.raft_model(5, term0=1000, loglen0=300)) == (2, 16)
    g = F.FieldSendGenerator([(M.M_CLIENT, F.FIXED(0), [F.CONST(7), F.CONST(9)])], M.raft_model(5))
    g(Rng(), None)
    assert g.area(g.sent[0]) == 0


def test_draw_order_counter_and_struct():
    """alternative (only when there is more than one), target, then the fields in order; the counter restarts with every test"""
    class Rng:
        def __init__(self):
            self.asked = []

        def next_int(self, bound):
            self.asked.append(bound)
            return bound - 1

    class Alive:
        def __init__(self, rng, n):
            self.rng, self.n = rng, n

        def __len__(self):
            return self.n

        def get_random(self):
            return 1 + self.rng.next_int(self.n)

    model = FF.pay_table(6)
    g = F.FieldSendGenerator([(0, F.FIXED(0), [F.CONST(1)]),
                              (0, F.RANDOM_ALIVE, [F.RANDOM(7), F.CONST(2), F.RANDOM(200), F.COUNTER, F.RANDOM(3), F.RANDOM(11)])], model)
    r = Rng()
    assert g(r, Alive(r, 3)) == F.send(3, 0, 6, 2) and r.asked == [2, 3, 7, 200, 3, 11] and g.sent == [[6, 2, 199, 1, 2, 10]]
    r.asked.clear()
    g(r, Alive(r, 0))
    assert r.asked == [2, 7, 200, 3, 11] and g.sent[1][3] == 2                              # nobody alive: actor 0, no draw
    r2 = Rng()
    assert g(r2, Alive(r2, 3)) and g.sent == [[6, 2, 199, 1, 2, 10]]                        # another test's generator: from 1 again
    s = g.to_struct()
    assert s.nbytes == 296 == ctypes.sizeof(T.FuzzFieldGen) and F.FIELD_ALT_DTYPE.itemsize == 36 == ctypes.sizeof(T.FuzzFieldAlt)
    a1 = s["alts"][0][1]
    assert int(s["n_alts"][0]) == 2 and int(a1["n_fields"]) == 6 and a1["kind"].tolist() == [2, 0, 2, 1, 2, 2] and int(a1["arg"][2]) == 200
    assert int(s["alts"][0][0]["n_fields"]) == 1 and not s["alts"][0][2:].tobytes().strip(b"\0")


def test_areas_are_zero_off_the_sends_and_prefix_sends_get_their_p0_p1():
    """(c) over the GPU suite's generator tests: an area only where a Send is; a Send of the prefix / postfix has the area
    trace_load makes of P0 / P1 with nothing staged (each masked to the table's width); generated Sends unpack to their fields"""
    for npay in (3, 4, 5, 6):
        cfg, w = FF.GenConfig(npay), T.payload_bits(npay)
        top = (1 << w) - 1
        assert cfg.stride == T.MAX_EXT_EVENTS == 255
        kinds = set()
        for explicit in (False, True):
            for ev, ar in FF.mirror_tests(npay, explicit):
                assert len(ev) == len(ar) <= 255
                n_sends = sum(1 for e in ev if e[0] == T.EV_SEND)
                assert n_sends < 256                     # (COUNTER never reaches its mask: a test holds fewer than 256 Sends)
                for i, (e, a) in enumerate(zip(ev, ar)):
                    if e[0] != T.EV_SEND:
                        assert a == 0
                        continue
                    f = T.payload_fields(a, npay)
                    if i < len(cfg.prefix) or e == cfg.postfix[0]:
                        assert a == (e[4] & top) | ((e[5] & top) << w) and a != 0
                    else:
                        assert (f[0], f[1]) == (e[4], e[5])
                        if e[1] == 1 and len([x for x in f if x]) <= 2 and f[1] < 7:
                            kinds.add(2)
                        if f[1] == top:
                            kinds.add(npay)
                            assert f[2] < 13 and (npay < 4 or f[3] < 200) and (npay < 5 or f[4] == top) and (npay < 6 or 1 <= f[5] <= n_sends)
                assert ar[len(cfg.prefix) - 1] == (0xABCD & top) | ((0x1234 & top) << w)
        assert kinds == {2, npay}
        assert max(len(ev) for ev, _ in FF.mirror_tests(npay)) == 255             # a test that fills its row
    assert FF.N_TESTS == 65


def test_the_crafted_seeds_reject_a_draw_inside_a_field():
    for npay in (3, 4, 5, 6):
        seed = FF.field_rejecting_seed(npay)
        assert set(FF.rejected_bounds(FF.GenConfig(npay), seed)) & set(FF.FIELD_BOUNDS)
        assert seed in FF.gen_seeds(npay, True)
        # (the counting generator changes nothing)
        cfg = FF.GenConfig(npay)
        ev, ar = F.generate_fuzz_test_fields(cfg.num_events, cfg.weights, cfg.gen(), cfg.prefix, seed, cfg.postfix)
        assert (tuple(ev), tuple(ar)) == FF.mirror_tests(npay, True)[FF.N_TESTS // 2]


def test_the_mirrors_refusals():
    """(d) what the C side refuses by name, the mirror refuses too"""
    narrow, wide3, wide6 = M.raft_model(5), FF.pay_table(3), FF.pay_table(6)
    ok = (0, F.FIXED(0), [F.CONST(0)] * 2)
    for model, bad in ((narrow, []), (narrow, [ok] * 9),
                       (narrow, [(0, F.FIXED(0), [F.CONST(0)] * 3)]),                    # three fields without DEMI_MODEL_PAYLOADS
                       (wide3, [(0, F.FIXED(0), [F.CONST(0)] * 4)]),                     # more fields than the table has
                       (wide6, [(0, F.FIXED(0), [F.CONST(0)] * 7)]),
                       (wide6, [(0, F.FIXED(0), [F.CONST(0), F.CONST(256)])]),           # W = 8
                       (narrow, [(0, F.FIXED(0), [F.CONST(256)])]),
                       (FF.pay_table(4), [(0, F.FIXED(0), [F.CONST(0), F.CONST(0), F.CONST(1 << 12)])]),
                       (wide3, [(0, F.FIXED(0), [F.RANDOM(0)])]), (wide3, [(0, F.FIXED(0), [F.RANDOM(257)])]),
                       (wide3, [(0, F.FIXED(0), [(3, 0)])]), (wide3, [(0, (2, 0), [])]), (wide3, [(32, F.FIXED(0), [])])):
        with pytest.raises(ValueError):
            F.FieldSendGenerator(bad, model)
    F.FieldSendGenerator([(0, F.FIXED(0), [F.CONST(255), F.RANDOM(256)] * 3)], wide6)
    F.FieldSendGenerator([(0, F.FIXED(0), [F.CONST(4095)] * 4)], FF.pay_table(4))
    F.FieldSendGenerator([(0, F.FIXED(0), [])], narrow)                                   # no field described: all of them 0


def test_the_k1_cases_hold_what_the_gpu_suite_relies_on():
    for case in FF.K1_CASES.values():
        tests = case.tests()
        assert len({len(e) for e, _ in tests}) == 3                                       # three lengths: a wrong row stride shows
        assert all(any(int(a) >> (2 * 9) for a in ar) for _, ar in tests)                 # fields >= 2 on the wire in every test
        for strategy in (T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO):
            with_areas, without = case.oracle(strategy, 70), case.oracle(strategy, 70, False)
            assert all(a.tobytes() != b.tobytes() for a, b in zip(with_areas, without))   # ... and part of every verdict
            assert len({int(h) for v in with_areas for h in v["hash"]}) > 3                # (the executions are not all one)
    # the ledger's violation is the memo in field 3: with the areas some executions of a test violate, without them none does
    for strategy in (T.STRATEGY_FULLY_RANDOM, T.STRATEGY_SRC_DST_FIFO):
        viol = [int((v["flags"] & T.V_VIOLATION).sum()) for v in FF.LEDGER.oracle(strategy, 70)]
        assert any(0 < n < 70 for n in viol) and any(n > 0 for n in viol)
        assert not any((v["flags"] & T.V_VIOLATION).any() for v in FF.LEDGER.oracle(strategy, 70, False))


def test_the_campaign_case_has_its_property_under_the_oracle():
    """(e) tests 0 .. k - 1 clean, test k violating first in execution e, k beyond the first launch of four tests - and no
    violation at all when the areas are left out"""
    assert FF.campaign_first_violation(12) == (FF.CAMPAIGN_TEST, FF.CAMPAIGN_EXEC) == (5, 1)
    assert FF.campaign_first_violation(12, T.STRATEGY_SRC_DST_FIFO) == (5, 2)
    assert FF.CAMPAIGN_TEST >= 4
    from oracle import oracle_py as O
    ev, ar = FF.campaign_test(FF.CAMPAIGN_TEST)
    assert any((int(a) >> 27) & 0x1FF == FF.MEMO for a in ar)
    O.set_ext_areas(None)
    v = O.random_explore(FF.ledger_model(), ev, FF.CAMPAIGN_EPC, seed_base=0, limits=FF.campaign_limits())
    assert not (v["flags"] & T.V_VIOLATION).any()


def test_the_fields_kernel_keeps_the_alternative_out_of_scratch(tmp_path):
    """k_fuzz_generate_fields compiled for gfx950 (device only, no GPU): the alternative is selected by value and its fields are
    unrolled, so there is no stack frame and no spilled vector register; the sets are the LDS columns of k_fuzz_generate"""
    import os
    import subprocess
    from .test_jit_cpu import ROOT, _meta_values
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    src = tmp_path / "fzf.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include "%s/include/demi_gpu.h"\n#include "%s/demi_amd/csrc/k_fuzz.hpp"\n'
                   'template __global__ void demi::k_fuzz_generate_fields<0>(const demi::FuzzFieldArgs);\n' % (ROOT, ROOT))
    obj = tmp_path / "fzf.co"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                           str(src), "-o", str(obj)], timeout=280)
    image = obj.read_bytes()
    assert b"k_fuzz_generate_fields" in image
    assert _meta_values(image, ".private_segment_fixed_size") == [0, 0]
    assert _meta_values(image, ".vgpr_spill_count") == [0, 0]
    assert _meta_values(image, ".group_segment_fixed_size") == [256 * 64] * 2
