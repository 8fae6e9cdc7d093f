"""CPU suite: the boundary of demi_replay_batch_submit / _wait - the header's prototypes against the argument types the ctypes
binding declares, and the JNI shim against the Scala adapter's @native declarations, name by name in both directions."""
import ctypes as C
import os
import re

from demi_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _prototype(header, name):
    """the parameter list of `int name(...);` in the header: [(C type without const, parameter name)], comments dropped"""
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, "include/demi_gpu.h does not declare %s" % name
    params = []
    for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        p = " ".join(p.replace("const", " ").replace("*", " * ").split())
        ctype, pname = p.rsplit(" ", 1)
        params.append((ctype.replace(" *", "*").replace("* ", "*"), pname))
    return params


def test_the_binding_declares_the_headers_argument_types():
    import __graft_entry__ as g
    g.build()
    from demi_amd import _native
    L = _native.lib()
    header = _read("include", "demi_gpu.h")
    # what the binding passes for each C type of these two prototypes (buffers as addresses, as for every other entry point)
    ctype_of = {"demi_ctx*": C.c_void_p, "uint64_t*": None, "uint64_t": C.c_uint64, "demi_limits*": C.POINTER(T.Limits),
                "uint32_t": C.c_uint32, "uint32_t*": C.POINTER(C.c_uint32), "demi_verdict*": C.c_void_p, "demi_violation*": C.c_void_p}
    want = {"demi_replay_batch_submit": [("demi_ctx*", "ctx"), ("uint64_t*", "masks"), ("uint64_t", "n"), ("demi_limits*", "limits"),
                                         ("uint32_t", "flag_mask"), ("uint32_t", "want_verdicts"), ("uint32_t*", "ticket")],
            "demi_replay_batch_wait": [("demi_ctx*", "ctx"), ("uint32_t", "ticket"), ("demi_verdict*", "out"), ("demi_violation*", "flagged"),
                                       ("uint32_t", "cap"), ("uint64_t*", "n_flagged"), ("uint64_t*", "first_index")]}
    for name, params in want.items():
        assert _prototype(header, name) == params
        assert name in _native.EXPORTS and hasattr(L, name)
        bound = getattr(L, name).argtypes
        assert len(bound) == len(params)
        for (ctype, pname), b in zip(params, bound):
            if ctype == "uint64_t*":           # masks: an address; the two counters: references to c_uint64
                assert b is (C.c_void_p if pname == "masks" else C.POINTER(C.c_uint64)), (name, pname)
            else:
                assert b is ctype_of[ctype], (name, pname)
    # the pair mirrors K1's: the same parameters behind the first two of the submit, the same wait
    k1s, k1w = _prototype(header, "demi_random_explore_submit"), _prototype(header, "demi_random_explore_wait")
    assert k1s[2:] == want["demi_replay_batch_submit"][2:] and k1w == want["demi_replay_batch_wait"]
    assert re.search(r"#define\s+DEMI_ABI_VERSION\s+5u?\s", header)          # additive: the generation of the struct layouts stays
    # ... and the Python methods exist with the documented parameters
    import inspect
    assert list(inspect.signature(_native.Context.replay_batch_submit).parameters) == ["self", "masks", "limits", "flag_mask", "want_verdicts"]
    assert list(inspect.signature(_native.Context.replay_batch_wait).parameters) == ["self", "ticket", "out", "cap"]


def test_every_native_declaration_has_its_jni_export_and_the_reverse():
    scala = _read("scala", "akka", "dispatch", "verification", "gpu", "DemiGpu.scala")
    shim = _read("jni", "demi_jni.c")
    natives = re.findall(r"@native\s+def\s+(\w+)", scala)
    exports = re.findall(r"JNIEXPORT\s+\w+\s+JNICALL\s+FN\((\w+)\)", shim)
    assert len(natives) > 20 and len(set(natives)) == len(natives) and len(set(exports)) == len(exports)
    assert sorted(natives) == sorted(exports)
    for name in ("replayBatchSubmit", "replayBatchWait", "randomExploreSubmit", "randomExploreWait"):
        assert name in natives
    # the shim's two new functions call the two new entry points
    for fn, entry in (("replayBatchSubmit", "demi_replay_batch_submit"), ("replayBatchWait", "demi_replay_batch_wait")):
        body = shim[shim.index("FN(%s)" % fn):]
        body = body[:body.index("\nJNIEXPORT")]
        assert entry + "(" in body
