"""ctypes binding of libdemi_gpu.so (the C ABI of include/demi_gpu.h).

There is no fallback: if the shared library is missing or no MI355X is visible, the product path
raises.  Build with `python -c "import __graft_entry__ as g; g.build()"` or `make -C demi_amd/csrc`.
"""
import ctypes as C
import os

from . import types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdemi_gpu.so")

EXPORTS = ["demi_ctx_create", "demi_ctx_destroy", "demi_last_error", "demi_version", "demi_model_load",
           "demi_trace_load", "demi_random_explore", "demi_random_explore_dev", "demi_random_get_trace", "demi_collect_violations_dev",
           "demi_replay_load", "demi_replay_batch", "demi_replay_batch_dev", "demi_dpor_load", "demi_dpor_batch", "demi_dpor_explore", "demi_random_explore_violations", "demi_random_get_trace_carried",
           "demi_replay_removal_batch", "demi_replay_get_kept", "demi_replay_recorded_len", "demi_ddmin", "demi_dpor_set_traces", "demi_model_specialize", "demi_model_is_specialized", "demi_model_code_id",
           "demi_specialize_check", "demi_specialize_source", "demi_specialize_source_k1", "demi_provenance_prune", "demi_device_probe", "demi_device_probe_mix", "demi_calib_rw", "demi_random_explore_flagged", "demi_collect_flagged_dev", "demi_random_explore_submit", "demi_random_explore_wait", "demi_trace_len",
           "demi_comm_unique_id", "demi_comm_create", "demi_comm_create_host", "demi_comm_destroy", "demi_comm_rank",
           "demi_comm_allgather_dev", "demi_random_explore_sharded", "demi_replay_batch_sharded", "demi_abi_version", "demi_replay_externals_len", "demi_edit_distance_dpor_ddmin", "demi_dpor_explored", "demi_random_ddmin", "demi_random_explore_candidates", "demi_ext_payload_areas",
           "demi_replay_wildcard_load", "demi_replay_wildcard_batch", "demi_replay_wildcard_get_trace",
           "demi_replay_wildcard_candidates", "demi_wildcard_ddmin",
           "demi_fuzz_stride", "demi_fuzz_generate", "demi_random_explore_tests", "demi_fuzz_campaign",
           "demi_fuzz_generate_fields", "demi_random_explore_tests_areas", "demi_fuzz_campaign_fields",
           "demi_fuzz_launch_summary", "demi_fuzz_launch_summary_row", "demi_fuzz_campaign_pipelined",
           "demi_replay_removal_round", "demi_minimize_internals", "demi_replay_wildcard_round", "demi_minimize_wildcards",
           "demi_replay_batch_submit", "demi_replay_batch_wait",
           "demi_dpor_wildcard_batch", "demi_wildcard_dpor_test"]

_lib = None
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)     # demi_allgather_fn


class DemiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("demi_gpu error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libdemi_gpu.so is not built (%s); run __graft_entry__.build()" % LIB_PATH)
    if not os.environ.get("DEMI_NO_TORCH"):
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; loading it first makes
        # libdemi_gpu.so bind to the same runtime, so torch tensors / streams and our kernels share a
        # device context (loading the system runtime first leaves torch with "No HIP GPUs").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    L.demi_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.demi_ctx_destroy.argtypes = [C.c_void_p]
    L.demi_ctx_destroy.restype = None
    L.demi_last_error.argtypes = [C.c_void_p]
    L.demi_last_error.restype = C.c_char_p
    L.demi_version.restype = C.c_char_p
    L.demi_abi_version.argtypes = []
    L.demi_abi_version.restype = C.c_uint32
    if L.demi_abi_version() != T.ABI_VERSION:       # (struct layouts of another generation of include/demi_gpu.h)
        raise ImportError("libdemi_gpu.so has ABI generation %d, this binding was written for %d: rebuild (__graft_entry__.build())"
                          % (L.demi_abi_version(), T.ABI_VERSION))
    L.demi_replay_externals_len.argtypes = [C.c_void_p]
    L.demi_replay_externals_len.restype = C.c_uint32
    L.demi_trace_len.argtypes = [C.c_void_p]
    L.demi_trace_len.restype = C.c_uint32
    L.demi_model_load.argtypes = [C.c_void_p, C.POINTER(T.ModelStruct)]
    L.demi_model_specialize.argtypes = [C.c_void_p, C.c_int]
    L.demi_model_is_specialized.argtypes = [C.c_void_p]
    L.demi_model_code_id.argtypes = [C.c_void_p]
    L.demi_model_code_id.restype = C.c_uint64
    L.demi_specialize_check.argtypes = [C.POINTER(T.ModelStruct), C.c_char_p, C.c_size_t]
    L.demi_specialize_check.restype = C.c_long
    L.demi_dpor_set_traces.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.demi_dpor_set_traces.restype = C.c_int
    L.demi_ddmin.argtypes = [C.c_void_p, C.POINTER(T.Limits), C.POINTER(T.DdminParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(T.DdminStats)]
    L.demi_ddmin.restype = C.c_int
    L.demi_edit_distance_dpor_ddmin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(T.DporParams),
                                                C.POINTER(T.IncDdminParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                C.c_void_p, C.POINTER(T.IncDdminStats)]
    L.demi_edit_distance_dpor_ddmin.restype = C.c_int
    L.demi_specialize_source.argtypes = [C.POINTER(T.ModelStruct), C.c_char_p, C.c_size_t]
    L.demi_specialize_source.restype = C.c_long
    L.demi_specialize_source_k1.argtypes = [C.POINTER(T.ModelStruct), C.c_char_p, C.c_size_t]
    L.demi_specialize_source_k1.restype = C.c_long
    L.demi_trace_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.demi_ext_payload_areas.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.demi_random_explore.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_void_p]
    L.demi_random_explore_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(T.Limits),
                                          C.c_void_p, C.c_void_p]
    L.demi_random_get_trace.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.POINTER(T.Verdict),
                                        C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.demi_random_get_trace_carried.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(T.Limits), C.POINTER(T.Verdict),
                                                C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.demi_collect_violations_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_void_p]
    L.demi_replay_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.demi_replay_recorded_len.argtypes = [C.c_void_p]
    L.demi_replay_recorded_len.restype = C.c_uint32
    L.demi_replay_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_void_p]
    L.demi_replay_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_void_p, C.c_void_p]
    L.demi_replay_removal_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_void_p]
    L.demi_replay_wildcard_load.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.demi_replay_wildcard_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_void_p]
    L.demi_replay_wildcard_get_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(T.Limits), C.POINTER(T.Verdict),
                                                 C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.demi_replay_wildcard_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(T.Limits),
                                                  C.c_void_p, C.c_void_p]
    L.demi_wildcard_ddmin.argtypes = [C.c_void_p, C.POINTER(T.Limits), C.POINTER(T.DdminParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.POINTER(T.DdminStats), C.POINTER(T.WildcardDdminResult)]
    L.demi_replay_get_kept.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(T.Limits), C.POINTER(T.Verdict),
                                       C.c_void_p]
    L.demi_dpor_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.demi_dpor_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(T.DporParams),
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.demi_dpor_wildcard_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(T.DporParams), C.c_uint32,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.demi_wildcard_dpor_test.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(T.DporParams), C.POINTER(T.WcdporParams),
                                          C.c_void_p, C.POINTER(T.WcdporResult)]
    L.demi_dpor_explore.argtypes = [C.c_void_p, C.POINTER(T.DporParams), C.POINTER(T.DporSearch), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(T.DporStats)]
    L.demi_random_explore_candidates.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(T.Limits), C.c_void_p, C.c_void_p]
    L.demi_random_ddmin.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.POINTER(T.RandomDdminParams), C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(T.DdminStats)]
    L.demi_dpor_explored.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p,
                                     C.POINTER(C.c_uint32)]
    L.demi_random_explore_violations.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(T.Limits), C.c_void_p,
                                                 C.c_uint32, C.POINTER(C.c_uint64)]
    L.demi_random_explore_flagged.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(T.Limits), C.c_uint32, C.c_void_p,
                                              C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.demi_random_explore_submit.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(T.Limits), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.demi_random_explore_wait.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]
    L.demi_replay_batch_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.demi_replay_batch_wait.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]
    L.demi_collect_flagged_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32,
                                           C.c_void_p, C.c_void_p]
    L.demi_comm_unique_id.argtypes = [C.c_void_p]
    L.demi_comm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.demi_comm_create_host.argtypes = [C.c_void_p, C.c_int, C.c_int, ALLGATHER_FN, C.c_void_p]
    L.demi_comm_destroy.argtypes = [C.c_void_p]
    L.demi_comm_rank.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.demi_comm_allgather_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.demi_random_explore_sharded.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(T.Limits), C.c_void_p, C.c_uint32,
                                              C.POINTER(C.c_uint64)]
    L.demi_replay_batch_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(T.Limits), C.c_void_p]
    L.demi_device_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(T.ProbeResult)]
    L.demi_provenance_prune.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    L.demi_device_probe_mix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(T.ProbeResult)]
    L.demi_calib_rw.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32]
    L.demi_fuzz_stride.argtypes = [C.POINTER(T.FuzzParams)]
    L.demi_fuzz_stride.restype = C.c_uint32
    L.demi_fuzz_generate.argtypes = [C.c_void_p, C.POINTER(T.FuzzParams), C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.demi_random_explore_tests.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(T.Limits),
                                            C.c_void_p, C.c_void_p]
    L.demi_fuzz_campaign.argtypes = [C.c_void_p, C.POINTER(T.FuzzParams), C.POINTER(T.FuzzCampaignParams), C.POINTER(T.Limits), C.c_void_p,
                                     C.c_uint32, C.POINTER(T.FuzzCampaignResult)]
    L.demi_fuzz_generate_fields.argtypes = [C.c_void_p, C.POINTER(T.FuzzParams), C.POINTER(T.FuzzFieldGen), C.c_uint64, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.demi_random_explore_tests_areas.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  C.POINTER(T.Limits), C.c_void_p, C.c_void_p]
    L.demi_fuzz_campaign_fields.argtypes = [C.c_void_p, C.POINTER(T.FuzzParams), C.POINTER(T.FuzzFieldGen), C.POINTER(T.FuzzCampaignParams),
                                            C.POINTER(T.Limits), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(T.FuzzCampaignResult)]
    L.demi_fuzz_launch_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(T.FuzzSummary)]
    L.demi_fuzz_launch_summary_row.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.demi_fuzz_campaign_pipelined.argtypes = [C.c_void_p, C.POINTER(T.FuzzParams), C.POINTER(T.FuzzFieldGen), C.POINTER(T.FuzzCampaignParams),
                                               C.POINTER(T.FuzzPipelineParams), C.POINTER(T.Limits), C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.POINTER(T.FuzzCampaignResult), C.POINTER(T.FuzzPipelineStats)]
    L.demi_replay_removal_round.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(T.Limits), C.c_void_p,
                                            C.POINTER(T.RemovalRoundResult)]
    L.demi_minimize_internals.argtypes = [C.c_void_p, C.POINTER(T.Limits), C.POINTER(T.IntminParams), C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(T.IntminStats)]
    L.demi_replay_wildcard_round.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(T.Limits), C.c_void_p,
                                             C.POINTER(T.WildcardRoundResult)]
    L.demi_minimize_wildcards.argtypes = [C.c_void_p, C.POINTER(T.Limits), C.POINTER(T.WcminParams), C.c_void_p, C.c_uint32,
                                          C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(T.WcminStats)]
    # every export has its argument types declared: an undeclared one would silently truncate pointers to 32 bits
    for name in EXPORTS:
        fn = getattr(L, name)
        assert fn.argtypes is not None or name in ("demi_version",), "no argtypes for %s" % name
    _lib = L
    return L


def specialize_check(model_struct):
    """Generate + compile the specialised K1 kernel for a model without a device: (code size, kernel name)."""
    log = C.create_string_buffer(4096)
    n = lib().demi_specialize_check(C.byref(model_struct), log, len(log))
    if n < 0:
        raise DemiError(n, log.value.decode(errors="replace"))
    return int(n), log.value.decode()


def specialize_source(model_struct, k1=False, fx_commute=False):
    """The C++ the specialiser generates for the model's handlers (k1: the RandomScheduler kernel's flavour, with the
    table's effect-slot schedule when it has one).
    fx_commute (k1 only): True = the schedule demi_model_specialize compiles by default, in which a timer-set row may sit below
    a send that precedes it (jit.hpp fx_schedule); False = the schedule whose slot order is every path's program order - what
    the library's switch DEMI_JIT_NO_FX_COMMUTE selects and what a table gets whose commuted schedule is not exact.  The C
    entry point follows the switch; this wrapper sets it for the call, so that a caller reads one or the other by name."""
    saved = {k: os.environ.get(k) for k in ("DEMI_EXPERIMENT", "DEMI_JIT_NO_FX_COMMUTE")}
    try:
        if k1 and not fx_commute:
            os.environ["DEMI_EXPERIMENT"] = "1"
            os.environ["DEMI_JIT_NO_FX_COMMUTE"] = "1"
        elif k1:
            os.environ.pop("DEMI_JIT_NO_FX_COMMUTE", None)
        buf = C.create_string_buffer(1 << 20)
        n = (lib().demi_specialize_source_k1 if k1 else lib().demi_specialize_source)(C.byref(model_struct), buf, len(buf))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if n < 0:
        raise DemiError(n, buf.value.decode(errors="replace"))
    return buf.value.decode()


class Context:
    """demi_ctx: one per host thread, owns the device copies of the model and the trace."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().demi_ctx_create(device, C.byref(self._h))
        if rc != 0:
            raise DemiError(rc, "demi_ctx_create failed (no MI355X visible? the GPU path has no CPU fallback)")
        self.device = device

    def close(self):
        if self._h:
            lib().demi_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise DemiError(rc, lib().demi_last_error(self._h).decode())

    def model_load(self, model_struct):
        self._check(lib().demi_model_load(self._h, C.byref(model_struct)))

    def model_specialize(self, enable=True):
        """Compile the loaded table to native code (hiprtc) for the following random_explore launches."""
        self._check(lib().demi_model_specialize(self._h, 1 if enable else 0))

    def is_specialized(self):
        return bool(lib().demi_model_is_specialized(self._h))

    def code_id(self):
        """64-bit identity of the compiled K1 of the loaded model (0: interpreted)."""
        return int(lib().demi_model_code_id(self._h))

    def ext_payload_areas(self, areas):
        """demi_ext_payload_areas: the 48-bit payload areas (T.pay_area) of the external events of the NEXT trace_load / dpor_load -
        a DEMI_MODEL_PAYLOADS table's external Sends with all their fields.  None forgets a staged array."""
        import numpy as np
        if areas is None:
            self._check(lib().demi_ext_payload_areas(self._h, None, 0))
            return
        a = np.ascontiguousarray(areas, dtype=np.uint64)
        self._check(lib().demi_ext_payload_areas(self._h, a.ctypes.data if len(a) else None, len(a)))

    def trace_load(self, events, areas=None):
        import numpy as np
        ev = np.ascontiguousarray(events, dtype=T.EXT_EVENT_DTYPE)
        if areas is not None:
            self.ext_payload_areas(areas)
        self._check(lib().demi_trace_load(self._h, ev.ctypes.data if len(ev) else None, len(ev)))

    def random_explore(self, n, limits, seed_base=0, seeds=None):
        import numpy as np
        out = np.zeros(n, dtype=T.VERDICT_DTYPE)
        sp = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            k = max(1, int(limits.executions_per_instance))           # carried-generator mode: one seed per instance
            assert len(seeds) == (n + k - 1) // k
            sp = seeds.ctypes.data
        self._check(lib().demi_random_explore(self._h, C.c_uint64(seed_base), sp, n, C.byref(limits),
                                              out.ctypes.data if n else None))
        return out

    def random_explore_violations(self, n, limits, seed_base=0, cap=1 << 16):
        """n schedules; only the violating ones come back (VIOLATION_DTYPE, sorted by index) + their count."""
        import numpy as np
        out = np.zeros(cap, dtype=T.VIOLATION_DTYPE)
        cnt = C.c_uint64(0)
        self._check(lib().demi_random_explore_violations(self._h, C.c_uint64(seed_base), n, C.byref(limits),
                                                         out.ctypes.data, cap, C.byref(cnt)))
        return out[:min(cnt.value, cap)].copy(), int(cnt.value)

    def random_explore_flagged(self, n, limits, flag_mask, seed_base=0, cap=1 << 16):
        """n schedules; the entries whose verdict flags intersect flag_mask (sorted by index), their count and the lowest
        such index (exact even when the list is truncated to `cap`)."""
        import numpy as np
        out = np.zeros(cap, dtype=T.VIOLATION_DTYPE)
        cnt, first = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().demi_random_explore_flagged(self._h, C.c_uint64(seed_base), n, C.byref(limits), flag_mask,
                                                      out.ctypes.data, cap, C.byref(cnt), C.byref(first)))
        return out[:min(cnt.value, cap)].copy(), int(cnt.value), int(first.value)

    def random_explore_submit(self, n, limits, seed_base=0, flag_mask=0, want_verdicts=False):
        """explore() in pieces, up to three outstanding: enqueue n executions on a stream of the context's own; returns the ticket.
        want_verdicts: every verdict travels to the library's pinned memory behind the call (random_explore_wait(out=...))."""
        t = C.c_uint32(0)
        self._check(lib().demi_random_explore_submit(self._h, C.c_uint64(seed_base), n, C.byref(limits), flag_mask,
                                                     1 if want_verdicts else 0, C.byref(t)))
        return int(t.value)

    def random_explore_wait(self, ticket, out=None, cap=1 << 16):
        """-> (flagged entries sorted by index, their exact count, the lowest flagged index or 2^64 - 1); out: a VERDICT_DTYPE
        array of the call's n entries to receive every verdict, or None"""
        import numpy as np
        fl = np.zeros(cap, dtype=T.VIOLATION_DTYPE)
        cnt, first = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().demi_random_explore_wait(self._h, ticket, out.ctypes.data if out is not None else None, fl.ctypes.data, cap,
                                                   C.byref(cnt), C.byref(first)))
        return fl[:min(cnt.value, cap)].copy(), int(cnt.value), int(first.value)

    def random_explore_dev(self, n, limits, d_out_ptr, seed_base=0, d_seeds_ptr=None, stream=None):
        self._check(lib().demi_random_explore_dev(self._h, C.c_uint64(seed_base), d_seeds_ptr, n, C.byref(limits),
                                                  d_out_ptr, stream))

    def collect_violations_dev(self, d_verdicts_ptr, n, index_base, d_out_ptr, cap, d_count_ptr, stream=None):
        self._check(lib().demi_collect_violations_dev(self._h, d_verdicts_ptr, n, C.c_uint64(index_base), d_out_ptr,
                                                      cap, d_count_ptr, stream))

    def replay_load(self, original_externals, original_trace):
        import numpy as np
        ev = np.ascontiguousarray(original_externals, dtype=T.EXT_EVENT_DTYPE)
        rec = T.rec_events(original_trace)
        self._check(lib().demi_replay_load(self._h, ev.ctypes.data if len(ev) else None, len(ev),
                                           rec.ctypes.data if len(rec) else None, len(rec)))

    def replay_batch(self, masks, limits):
        """masks: uint64[n, 4] (bit i of the 256-bit row = external event i kept)."""
        import numpy as np
        masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(len(masks), dtype=T.VERDICT_DTYPE)
        self._check(lib().demi_replay_batch(self._h, masks.ctypes.data if len(masks) else None, len(masks),
                                            C.byref(limits), out.ctypes.data if len(masks) else None))
        return out

    def replay_batch_submit(self, masks, limits, flag_mask=0, want_verdicts=False):
        """replay_batch() in pieces, up to three outstanding: enqueue the candidates `masks` (uint64[n, 4]; copied before this returns)
        on a stream of the context's own; returns the ticket.  want_verdicts: every verdict travels to the library's pinned memory
        behind the call (replay_batch_wait(out=...))."""
        import numpy as np
        masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        t = C.c_uint32(0)
        self._check(lib().demi_replay_batch_submit(self._h, masks.ctypes.data if len(masks) else None, len(masks), C.byref(limits),
                                                   flag_mask, 1 if want_verdicts else 0, C.byref(t)))
        return int(t.value)

    def replay_batch_wait(self, ticket, out=None, cap=1 << 16):
        """-> (flagged entries sorted by index - the candidate's number within the call -, their exact count, the lowest flagged
        index or 2^64 - 1); out: a VERDICT_DTYPE array of the call's n entries to receive every verdict, or None"""
        import numpy as np
        fl = np.zeros(cap, dtype=T.VIOLATION_DTYPE)
        cnt, first = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().demi_replay_batch_wait(self._h, ticket, out.ctypes.data if out is not None else None, fl.ctypes.data, cap,
                                                 C.byref(cnt), C.byref(first)))
        return fl[:min(cnt.value, cap)].copy(), int(cnt.value), int(first.value)

    def replay_batch_dev(self, d_masks_ptr, n, limits, d_out_ptr, stream=None):
        """Device-resident form: masks [n][4] u64 and verdicts [n] stay in HBM; enqueued on `stream`, not synchronised."""
        self._check(lib().demi_replay_batch_dev(self._h, C.c_void_p(d_masks_ptr), C.c_uint64(n), C.byref(limits),
                                                C.c_void_p(d_out_ptr), stream))

    def replay_removal_batch(self, skips, limits, masks=None):
        """One STSScheduler.test per entry of skips: the loaded trace minus the delivery at that recorded-event
        index (0xFFFFFFFF = nothing removed); masks (uint64[n, 4]) default to every external kept."""
        import numpy as np
        skips = np.ascontiguousarray(skips, dtype=np.uint32)
        out = np.zeros(len(skips), dtype=T.VERDICT_DTYPE)
        if len(skips) == 0:
            return out
        mp = None
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
            if len(masks) != len(skips):
                raise ValueError("one mask per removal candidate")
            mp = masks.ctypes.data
        self._check(lib().demi_replay_removal_batch(self._h, mp, skips.ctypes.data, len(skips), C.byref(limits),
                                                    out.ctypes.data))
        return out

    def ddmin(self, limits, params=None, conjoined=None, cap=4096):
        """RunnerUtils.stsSchedDDMin on the loaded replay, natively (demi_ddmin): (mcs indices, [(candidate indices, passes)] in
        consultation order, candidates per launch, stats)."""
        import numpy as np
        params = params or T.DdminParams()
        mcs = np.zeros(4, dtype=np.uint64)
        consulted = np.zeros((cap, 4), dtype=np.uint64)
        passed = np.zeros(cap, dtype=np.uint8)
        batches = np.zeros(cap, dtype=np.uint32)
        st = T.DdminStats()
        conj = np.ascontiguousarray(conjoined, dtype=np.uint8) if conjoined is not None else None
        self._check(lib().demi_ddmin(self._h, C.byref(limits), C.byref(params), conj.ctypes.data if conj is not None else None,
                                     mcs.ctypes.data, consulted.ctypes.data, passed.ctypes.data, cap, batches.ctypes.data, cap,
                                     C.byref(st)))
        return T.mask_to_events(mcs), [(T.mask_to_events(consulted[i]), bool(passed[i])) for i in range(min(cap, st.consultations))], \
            [int(b) for b in batches[:st.launches]], st

    def random_explore_candidates(self, masks, executions, limits, seed_base=0):
        """K1 over candidate subsequences of the loaded trace: (verdicts [n_cand, executions], flags [n_cand])."""
        import numpy as np
        m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        v = np.zeros((len(m), executions), dtype=T.VERDICT_DTYPE)
        f = np.zeros(len(m), dtype=np.uint32)
        self._check(lib().demi_random_explore_candidates(self._h, C.c_uint64(seed_base), m.ctypes.data, len(m), executions, C.byref(limits),
                                                         v.ctypes.data, f.ctypes.data))
        return v, f

    @staticmethod
    def fuzz_params(num_events, weights, send_gen, prefix, postfix=()):
        """demi_fuzz_params for Fuzzer(num_events, weights, send_gen, prefix, postfix): (struct, the arrays it points into - keep
        them alive as long as the struct).  send_gen: fuzzer.SendGenerator (a FieldSendGenerator travels beside the struct, as
        field_gen_struct makes it: `gen` stays zero); prefix / postfix: event tuples or EXT_EVENT_DTYPE."""
        import numpy as np
        from . import fuzzer as F

        def arr(ev):
            if isinstance(ev, np.ndarray):
                return np.ascontiguousarray(ev, dtype=T.EXT_EVENT_DTYPE)
            return F.events_to_array(list(ev))
        pre, post = arr(prefix), arr(postfix)
        par = T.FuzzParams()
        par.num_events, par.n_prefix, par.n_postfix = num_events, len(pre), len(post)
        par.prefix = pre.ctypes.data if len(pre) else None
        par.postfix = post.ctypes.data if len(post) else None
        total, *cum = F.fuzz_thresholds(weights)
        par.total_mass = total
        for i in range(4):
            par.cum[i] = cum[i]
        if not isinstance(send_gen, F.FieldSendGenerator):
            C.memmove(C.byref(par.gen), send_gen.to_struct().ctypes.data, C.sizeof(T.FuzzSendGen))
        return par, (pre, post)

    @staticmethod
    def field_gen_struct(field_gen):
        """demi_fuzz_field_gen of a fuzzer.FieldSendGenerator"""
        fg = T.FuzzFieldGen()
        C.memmove(C.byref(fg), field_gen.to_struct().ctypes.data, C.sizeof(T.FuzzFieldGen))
        return fg

    def fuzz_generate(self, n_tests, num_events, weights, send_gen, prefix, postfix=(), seed_base=0, seeds=None, copy_out=True):
        """demi_fuzz_generate: n_tests tests of Fuzzer(num_events, weights, send_gen, prefix, postfix), test i under
        java.util.Random(seed_base + i) or seeds[i]; they stay resident for random_explore_tests(None, ..).  Returns
        (events [n_tests, stride], n_ev [n_tests], n_batches [n_tests]); copy_out=False leaves the events on the device (None).
        With a fuzzer.FieldSendGenerator (demi_fuzz_generate_fields) the payload areas [n_tests, stride] come beside the events:
        (events, areas, n_ev, n_batches), and stay resident with them."""
        import numpy as np
        from . import fuzzer as F
        par, keep = self.fuzz_params(num_events, weights, send_gen, prefix, postfix)
        stride = int(lib().demi_fuzz_stride(C.byref(par)))
        ev = np.zeros((n_tests, stride), dtype=T.EXT_EVENT_DTYPE) if copy_out and stride <= T.MAX_EXT_EVENTS else None     # (a longer stride is refused by the call)
        n_ev = np.zeros(n_tests, dtype=np.uint32)
        n_b = np.zeros(n_tests, dtype=np.uint32)
        sp = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            assert len(seeds) == n_tests
            sp = seeds.ctypes.data
        if isinstance(send_gen, F.FieldSendGenerator):
            fg = self.field_gen_struct(send_gen)
            ar = np.zeros((n_tests, stride), dtype=np.uint64) if ev is not None else None
            self._check(lib().demi_fuzz_generate_fields(self._h, C.byref(par), C.byref(fg), C.c_uint64(seed_base), sp, n_tests,
                                                        ev.ctypes.data if ev is not None and n_tests else None,
                                                        ar.ctypes.data if ar is not None and n_tests else None, n_ev.ctypes.data, n_b.ctypes.data))
            del keep
            return ev, ar, n_ev, n_b
        self._check(lib().demi_fuzz_generate(self._h, C.byref(par), C.c_uint64(seed_base), sp, n_tests,
                                             ev.ctypes.data if ev is not None and n_tests else None, n_ev.ctypes.data, n_b.ctypes.data))
        del keep
        return ev, n_ev, n_b

    def random_explore_tests(self, tests, executions, limits, seed_base=0, n_ev=None, n_tests=None, areas=None, with_areas=None):
        """K1 with a workgroup per test: (verdicts [n_tests, executions], flags [n_tests]).  tests: [n_tests, stride] events with
        their lengths n_ev (a list of event arrays is packed), or None for the first n_tests tests fuzz_generate left resident.
        areas: the tests' payload areas, shaped like `tests` (a list of per-test arrays is packed with them) - the call then goes
        through demi_random_explore_tests_areas, which takes a DEMI_MODEL_PAYLOADS table; with_areas=True asks for that entry point
        without areas (host tests: the areas are made of P0 / P1; None: the resident tests' own)."""
        import numpy as np
        if with_areas is None:
            with_areas = areas is not None
        ap = None
        if tests is None:
            assert n_tests is not None and areas is None
            tp, np_, stride = None, None, 0
        else:
            if not isinstance(tests, np.ndarray):
                lens = [len(t) for t in tests]
                packed = np.zeros((len(tests), max(lens + [1])), dtype=T.EXT_EVENT_DTYPE)
                for i, t in enumerate(tests):
                    packed[i, :lens[i]] = np.asarray(t, dtype=T.EXT_EVENT_DTYPE)
                if areas is not None:
                    pa = np.zeros(packed.shape, dtype=np.uint64)
                    for i, a in enumerate(areas):
                        if len(a) != lens[i]:
                            raise ValueError("random_explore_tests: test %d has %d events and %d areas" % (i, lens[i], len(a)))
                        pa[i, :lens[i]] = np.asarray(a, dtype=np.uint64)
                    areas = pa
                tests, n_ev = packed, lens
            if n_ev is None:
                raise ValueError("random_explore_tests: an array of tests needs n_ev, the length of every test")
            tests = np.ascontiguousarray(tests, dtype=T.EXT_EVENT_DTYPE)
            n_ev = np.ascontiguousarray(n_ev, dtype=np.uint32)
            if tests.ndim != 2 or n_ev.shape != (tests.shape[0],):
                raise ValueError("random_explore_tests: tests is [n_tests, stride] and n_ev [n_tests]")
            n_tests, stride = tests.shape
            tp, np_ = tests.ctypes.data, n_ev.ctypes.data
            if areas is not None:
                areas = np.ascontiguousarray(areas, dtype=np.uint64)
                if areas.shape != tests.shape:
                    raise ValueError("random_explore_tests: areas is [n_tests, stride] like tests")
                ap = areas.ctypes.data
        v = np.zeros((n_tests, executions), dtype=T.VERDICT_DTYPE)
        f = np.zeros(n_tests, dtype=np.uint32)
        if with_areas:
            self._check(lib().demi_random_explore_tests_areas(self._h, C.c_uint64(seed_base), tp, ap, np_, stride, n_tests, executions,
                                                              C.byref(limits), v.ctypes.data, f.ctypes.data))
            return v, f
        self._check(lib().demi_random_explore_tests(self._h, C.c_uint64(seed_base), tp, np_, stride, n_tests, executions, C.byref(limits),
                                                    v.ctypes.data, f.ctypes.data))
        return v, f

    def fuzz_launch_summary(self, n_tests, executions, flags=None, verdicts=None, row=False):
        """demi_fuzz_launch_summary: the T.FuzzSummary of a launch's flags [n_tests] and verdicts [n_tests, executions] (both, or
        neither: the results the last random_explore_tests(None, ..) left on the device).  row=True: (summary, the hit test's events or
        None, its payload areas or None) - demi_fuzz_launch_summary_row."""
        import numpy as np
        fp = vp = None
        if flags is not None:
            flags = np.ascontiguousarray(flags, dtype=np.uint32)
            assert flags.shape == (n_tests,)
            fp = flags.ctypes.data
        if verdicts is not None:
            verdicts = np.ascontiguousarray(verdicts, dtype=T.VERDICT_DTYPE)
            assert verdicts.size == n_tests * executions
            vp = verdicts.ctypes.data
        s = T.FuzzSummary()
        self._check(lib().demi_fuzz_launch_summary(self._h, fp, vp, n_tests, executions, C.byref(s)))
        if not row:
            return s
        if s.first_hit >= n_tests:
            return s, None, None
        ev = np.zeros(T.MAX_EXT_EVENTS, dtype=T.EXT_EVENT_DTYPE)
        ar = np.zeros(T.MAX_EXT_EVENTS, dtype=np.uint64)
        self._check(lib().demi_fuzz_launch_summary_row(self._h, ev.ctypes.data, ar.ctypes.data, T.MAX_EXT_EVENTS))
        return s, ev[:s.n_events].copy(), ar[:s.n_events].copy()

    def fuzz_campaign(self, num_events, weights, send_gen, prefix, limits, postfix=(), executions_per_test=1, tests_per_launch=256,
                      max_tests=1024, test_seed_base=0, exec_seed_base=0, in_flight=None, cap=None):
        """demi_fuzz_campaign: (result struct, the violating test's events or None).  With a fuzzer.FieldSendGenerator
        (demi_fuzz_campaign_fields): (result struct, events or None, their payload areas or None).
        in_flight=1..3 (0 = 2): demi_fuzz_campaign_pipelined, that many launches on the device at a time - the same answers; its
        T.FuzzPipelineStats is left in self.fuzz_pipeline_stats.  None: the synchronous entry points.  cap: the events the output
        holds (default: the largest test)."""
        import numpy as np
        from . import fuzzer as F
        par, keep = self.fuzz_params(num_events, weights, send_gen, prefix, postfix)
        cp = T.FuzzCampaignParams(test_seed_base=test_seed_base, exec_seed_base=exec_seed_base, executions_per_test=executions_per_test,
                                  tests_per_launch=tests_per_launch, max_tests=max_tests)
        res = T.FuzzCampaignResult()
        cap = T.MAX_EXT_EVENTS if cap is None else cap
        ev = np.zeros(max(cap, 1), dtype=T.EXT_EVENT_DTYPE)
        if in_flight is not None:
            fields = isinstance(send_gen, F.FieldSendGenerator)
            fg = self.field_gen_struct(send_gen) if fields else None
            ar = np.zeros(max(cap, 1), dtype=np.uint64)
            pp = T.FuzzPipelineParams(in_flight=in_flight)
            self.fuzz_pipeline_stats = st = T.FuzzPipelineStats()
            self._check(lib().demi_fuzz_campaign_pipelined(self._h, C.byref(par), C.byref(fg) if fields else None, C.byref(cp), C.byref(pp),
                                                           C.byref(limits), ev.ctypes.data, ar.ctypes.data if fields else None, cap,
                                                           C.byref(res), C.byref(st)))
            del keep
            if fields:
                return (res, ev[:res.n_events].copy(), ar[:res.n_events].copy()) if res.found else (res, None, None)
            return res, (ev[:res.n_events].copy() if res.found else None)
        if isinstance(send_gen, F.FieldSendGenerator):
            fg = self.field_gen_struct(send_gen)
            ar = np.zeros(cap, dtype=np.uint64)
            self._check(lib().demi_fuzz_campaign_fields(self._h, C.byref(par), C.byref(fg), C.byref(cp), C.byref(limits), ev.ctypes.data,
                                                        ar.ctypes.data, cap, C.byref(res)))
            del keep
            return (res, ev[:res.n_events].copy(), ar[:res.n_events].copy()) if res.found else (res, None, None)
        self._check(lib().demi_fuzz_campaign(self._h, C.byref(par), C.byref(cp), C.byref(limits), ev.ctypes.data, cap, C.byref(res)))
        del keep
        return res, (ev[:res.n_events].copy() if res.found else None)

    def random_ddmin(self, limits, params=None, seed_base=0, conjoined=None, cap=4096):
        """RunnerUtils.randomDDMin on the loaded trace, natively (demi_random_ddmin): (mcs indices, [(candidate indices, passes)]
        in consultation order, candidates per launch, stats)."""
        import numpy as np
        params = params or T.RandomDdminParams()
        mcs = np.zeros(4, dtype=np.uint64)
        consulted = np.zeros((cap, 4), dtype=np.uint64)
        passed = np.zeros(cap, dtype=np.uint8)
        batches = np.zeros(cap, dtype=np.uint32)
        st = T.DdminStats()
        conj = np.ascontiguousarray(conjoined, dtype=np.uint8) if conjoined is not None else None
        self._check(lib().demi_random_ddmin(self._h, C.c_uint64(seed_base), C.byref(limits), C.byref(params),
                                            conj.ctypes.data if conj is not None else None, mcs.ctypes.data, consulted.ctypes.data,
                                            passed.ctypes.data, cap, batches.ctypes.data, cap, C.byref(st)))
        return T.mask_to_events(mcs), [(T.mask_to_events(consulted[i]), bool(passed[i])) for i in range(min(cap, st.consultations))], \
            [int(b) for b in batches[:min(cap, st.launches)]], st

    def replay_get_kept(self, n_rec, skip, limits, mask=None):
        """(Verdict, uint8[n_rec]) of one candidate: which recorded events make up its executed trace."""
        import numpy as np
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(4)
            mp = mask.ctypes.data
        v = T.Verdict()
        kept = np.zeros(max(int(n_rec), 1), dtype=np.uint8)
        self._check(lib().demi_replay_get_kept(self._h, mp, C.c_uint32(int(skip) & 0xFFFFFFFF), C.byref(limits),
                                               C.byref(v), kept.ctypes.data))
        return v, kept[:int(n_rec)]

    def replay_removal_round(self, skips, limits, mask=None):
        """One round of STSSchedMinimizer.minimize (demi_replay_removal_round): the proposals `skips` over the loaded execution,
        reduced on the device.  (RemovalRoundResult, uint8[n_rec] kept marks of proposal first_hit - None without a hit)."""
        import numpy as np
        skips = np.ascontiguousarray(skips, dtype=np.uint32)
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(4)
            mp = mask.ctypes.data
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        kept = np.zeros(max(n_rec, 1), dtype=np.uint8)
        res = T.RemovalRoundResult()
        self._check(lib().demi_replay_removal_round(self._h, mp, skips.ctypes.data if len(skips) else None, len(skips), C.byref(limits),
                                                    kept.ctypes.data, C.byref(res)))
        return res, (kept[:n_rec] if res.first_hit != 0xFFFFFFFF else None)

    def minimize_internals(self, limits, params=None, cap=None):
        """RunnerUtils.minimizeInternals on the loaded replay, natively (demi_minimize_internals): (minimized recorded events,
        record_internal_size sequence, candidates per round, IntminStats).  The context's loaded execution is the minimized one
        afterwards - also when the call raises on a capacity (then the last adopted trace)."""
        import numpy as np
        params = params or T.IntminParams()
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        cap = n_rec if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=T.REC_EVENT_DTYPE)
        sizes = np.zeros(max(n_rec, 1), dtype=np.uint32)       # (a replay per delivery at the most)
        batches = np.zeros(max(n_rec, 1), dtype=np.uint32)
        n = C.c_uint32(0)
        st = T.IntminStats()
        self._check(lib().demi_minimize_internals(self._h, C.byref(limits), C.byref(params), out.ctypes.data, cap, C.byref(n),
                                                  sizes.ctypes.data, len(sizes), batches.ctypes.data, len(batches), C.byref(st)))
        return out[:n.value].copy(), [int(x) for x in sizes[:min(len(sizes), st.total_replays)]], \
            [int(x) for x in batches[:min(len(batches), st.rounds)]], st

    def replay_wildcard_load(self, type_sets, policies):
        """The selector of every recorded event of the loaded execution (demi_replay_wildcard_load): type_sets uint32[n_rec]
        (0 = exact delivery), policies uint8[n_rec] (types.WILDCARD_HEAD / FIRST / LAST)."""
        import numpy as np
        ts = np.ascontiguousarray(type_sets, dtype=np.uint32)
        po = np.ascontiguousarray(policies, dtype=np.uint8)
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        if len(ts) != n_rec or len(po) != n_rec:
            raise ValueError("one selector per recorded event of the loaded trace")
        pad = np.zeros(1, dtype=np.uint32)
        self._check(lib().demi_replay_wildcard_load(self._h, (ts if n_rec else pad).ctypes.data,
                                                    (po if n_rec else pad.view(np.uint8)).ctypes.data))

    @staticmethod
    def _present_words(present, n_rec):
        """bool[n, n_rec] (or already packed uint64[n, words]) -> uint64[n, ceil(n_rec / 64)]."""
        import numpy as np
        present = np.asarray(present)
        words = (int(n_rec) + 63) // 64
        if present.dtype == np.uint64:
            return np.ascontiguousarray(present).reshape(-1, max(words, 1))[:, :words] if words else present.reshape(len(present), 0)
        present = present.reshape(-1, int(n_rec)).astype(bool)
        padded = np.zeros((len(present), words * 64), dtype=np.uint8)
        padded[:, :int(n_rec)] = present
        return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint64).reshape(len(present), words)

    def replay_wildcard_batch(self, present, limits, masks=None):
        """One STSScheduler.test per row of `present` (bool[n, n_rec]: which recorded MsgEvents the candidate's trace holds)."""
        import numpy as np
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        pw = self._present_words(present, n_rec)
        out = np.zeros(len(pw), dtype=T.VERDICT_DTYPE)
        if len(pw) == 0:
            return out
        mp = None
        if masks is not None:
            masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
            if len(masks) != len(pw):
                raise ValueError("one mask per candidate")
            mp = masks.ctypes.data
        self._check(lib().demi_replay_wildcard_batch(self._h, mp, pw.ctypes.data if pw.size else out.ctypes.data, len(pw),
                                                     C.byref(limits), out.ctypes.data))
        return out

    def replay_wildcard_get_trace(self, present, limits, mask=None, cap=None):
        """(Verdict, kept uint8[n_rec], executed trace as REC_EVENT records) of one candidate (demi_replay_wildcard_get_trace)."""
        import numpy as np
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        pw = self._present_words(np.asarray(present).reshape(1, -1), n_rec)
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(4)
            mp = mask.ctypes.data
        cap = int(cap) if cap is not None else T.MAX_REC_EVENTS
        v = T.Verdict()
        kept = np.zeros(max(n_rec, 1), dtype=np.uint8)
        rec = np.zeros(max(cap, 1), dtype=T.REC_EVENT_DTYPE)
        n_out = C.c_uint32(0)
        dummy = np.zeros(1, dtype=np.uint64)
        self._check(lib().demi_replay_wildcard_get_trace(self._h, mp, (pw if pw.size else dummy).ctypes.data, C.byref(limits),
                                                         C.byref(v), kept.ctypes.data, rec.ctypes.data, cap, C.byref(n_out)))
        return v, kept[:n_rec], rec[:n_out.value].copy()

    def replay_wildcard_round(self, present, limits, mask=None):
        """One round of WildcardMinimizer.doMinimize (demi_replay_wildcard_round): the proposals `present` (bool[n, n_rec]) over the
        loaded execution and selectors, reduced on the device.  (WildcardRoundResult, uint8[n_rec] kept marks of proposal
        first_hit - None without a hit)."""
        import numpy as np
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        pw = self._present_words(present, n_rec)
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint64).reshape(4)
            mp = mask.ctypes.data
        kept = np.zeros(max(n_rec, 1), dtype=np.uint8)
        res = T.WildcardRoundResult()
        dummy = np.zeros(1, dtype=np.uint64)
        self._check(lib().demi_replay_wildcard_round(self._h, mp, (pw if pw.size else dummy).ctypes.data, len(pw), C.byref(limits),
                                                     kept.ctypes.data, C.byref(res)))
        return res, (kept[:n_rec] if res.first_hit != 0xFFFFFFFF else None)

    def minimize_wildcards(self, limits, params, cap=None):
        """WildcardMinimizer.minimize on the loaded replay, natively (demi_minimize_wildcards): (minimized recorded events,
        record_internal_size sequence, proposals per round, WcminStats).  The context's loaded execution is the minimized one
        afterwards, without selectors - also when the call raises on a capacity (then the last adopted trace)."""
        import numpy as np
        cap = T.MAX_REC_EVENTS if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=T.REC_EVENT_DTYPE)
        sizes = np.zeros(2 * T.MAX_REC_EVENTS + 4, dtype=np.uint32)    # (a replay per delivery and pass at the most, and the fencepost)
        batches = np.zeros(2 * T.MAX_REC_EVENTS + 4, dtype=np.uint32)
        n = C.c_uint32(0)
        st = T.WcminStats()
        self._check(lib().demi_minimize_wildcards(self._h, C.byref(limits), C.byref(params), out.ctypes.data, cap, C.byref(n),
                                                  sizes.ctypes.data, len(sizes), batches.ctypes.data, len(batches), C.byref(st)))
        return out[:n.value].copy(), [int(x) for x in sizes[:min(len(sizes), st.sizes)]], \
            [int(x) for x in batches[:min(len(batches), st.rounds)]], st

    def _base_present(self, base_present):
        import numpy as np
        if base_present is None:
            return None
        n_rec = int(lib().demi_replay_recorded_len(self._h))
        pw = self._present_words(np.asarray(base_present).reshape(1, -1), n_rec)
        return pw if pw.size else np.zeros((1, 1), dtype=np.uint64)

    def replay_wildcard_candidates(self, masks, drops, limits, base_present=None, want_all=False):
        """One WildcardTestOracle.test per row of `masks` (demi_replay_wildcard_candidates): proposal 0 is `base_present`
        (bool[n_rec]; None: every delivery), proposal j >= 1 that row without the MsgEvent recorded at drops[j - 1].  Returns the
        reduced records (WILDCARD_CANDIDATE_DTYPE[n_cand]), with want_all also the verdict plane [n_cand, 1 + len(drops)]."""
        import numpy as np
        m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        d = np.ascontiguousarray(drops, dtype=np.uint32).reshape(-1)
        out = np.zeros(len(m), dtype=T.WILDCARD_CANDIDATE_DTYPE)
        plane = np.zeros((len(m), len(d) + 1), dtype=T.VERDICT_DTYPE) if want_all else None
        bp = self._base_present(base_present)
        self._check(lib().demi_replay_wildcard_candidates(self._h, m.ctypes.data if len(m) else None, len(m),
                                                          bp.ctypes.data if bp is not None else None, d.ctypes.data if len(d) else None,
                                                          len(d), C.byref(limits), out.ctypes.data if len(m) else None,
                                                          plane.ctypes.data if want_all and len(m) else None))
        return (out, plane) if want_all else out

    def wildcard_ddmin(self, limits, drops, params=None, conjoined=None, base_present=None, cap=4096):
        """RunnerUtils.wildcardDDMin on the loaded replay and selectors, natively (demi_wildcard_ddmin): (mcs indices,
        [(candidate indices, passes, first_hit or None)] in consultation order, candidates per launch, stats, result)."""
        import numpy as np
        params = params or T.DdminParams(check_unmodified=0)
        mcs = np.zeros(4, dtype=np.uint64)
        consulted = np.zeros((cap, 4), dtype=np.uint64)
        passed = np.zeros(cap, dtype=np.uint8)
        hits = np.zeros(cap, dtype=np.uint32)
        batches = np.zeros(cap, dtype=np.uint32)
        st, res = T.DdminStats(), T.WildcardDdminResult()
        d = np.ascontiguousarray(drops, dtype=np.uint32).reshape(-1)
        conj = np.ascontiguousarray(conjoined, dtype=np.uint8) if conjoined is not None else None
        bp = self._base_present(base_present)
        self._check(lib().demi_wildcard_ddmin(self._h, C.byref(limits), C.byref(params), conj.ctypes.data if conj is not None else None,
                                              bp.ctypes.data if bp is not None else None, d.ctypes.data if len(d) else None, len(d),
                                              mcs.ctypes.data, consulted.ctypes.data, passed.ctypes.data, hits.ctypes.data, cap,
                                              batches.ctypes.data, cap, C.byref(st), C.byref(res)))
        cons = [(T.mask_to_events(consulted[i]), bool(passed[i]), None if int(hits[i]) == T.NO_HIT else int(hits[i]))
                for i in range(min(cap, st.consultations))]
        return T.mask_to_events(mcs), cons, [int(b) for b in batches[:min(cap, st.launches)]], st, res

    def dpor_load(self, externals, areas=None):
        import numpy as np
        ev = np.ascontiguousarray(externals, dtype=T.EXT_EVENT_DTYPE)
        if areas is not None:
            self.ext_payload_areas(areas)
        self._check(lib().demi_dpor_load(self._h, ev.ctypes.data if len(ev) else None, len(ev)))

    def dpor_batch(self, prefixes, params, shared=None):
        """prefixes: list of DPOR_TRACE_DTYPE arrays (nextTrace of each interleaving); shared[i]: leading events of
        prefix i whose racing pairs the caller already has (None / 0 = report all).  Returns
        (verdicts, [trace arrays], [pair arrays])."""
        import numpy as np
        n = len(prefixes)
        stride = max([len(p) for p in prefixes] + [1])
        pf = np.zeros((n, stride), dtype=T.DPOR_TRACE_DTYPE)
        pl = np.zeros(n, dtype=np.uint32)
        for i, p in enumerate(prefixes):
            pf[i, :len(p)] = p
            pl[i] = len(p)
        verdicts = np.zeros(n, dtype=T.VERDICT_DTYPE)
        traces = np.zeros((n, T.DPOR_MAX_TRACE), dtype=T.DPOR_TRACE_DTYPE)
        tl = np.zeros(n, dtype=np.uint32)
        pairs = np.zeros((n, max(1, params.max_pairs)), dtype=T.DPOR_PAIR_DTYPE)
        npairs = np.zeros(n, dtype=np.uint32)
        sh = np.ascontiguousarray(shared, dtype=np.uint32) if shared is not None else None
        if n:
            self._check(lib().demi_dpor_batch(self._h, pf.ctypes.data, pl.ctypes.data, sh.ctypes.data if sh is not None else None,
                                              stride, n, C.byref(params),
                                              verdicts.ctypes.data, traces.ctypes.data, tl.ctypes.data,
                                              pairs.ctypes.data, npairs.ctypes.data))
        return verdicts, [traces[i, :tl[i]].copy() for i in range(n)], [pairs[i, :npairs[i]].copy() for i in range(n)]

    def dpor_wildcard_batch(self, prefixes, params, stop_after_next_trace=True, max_alts=64):
        """One interleaving per next trace whose entries may be wildcards (demi_dpor_wildcard_batch; kinds DPOR_KIND_WILDCARD /
        DPOR_KIND_EXACT_WORD of types.py).  Returns (verdicts, [trace arrays], [sorted ignored positions], [sorted trace indices
        delivered by a wildcard], [DPOR_WILD_ALT_DTYPE arrays])."""
        import numpy as np
        n = len(prefixes)
        stride = max([len(p) for p in prefixes] + [1])
        pf = np.zeros((n, stride), dtype=T.DPOR_TRACE_DTYPE)
        pl = np.zeros(n, dtype=np.uint32)
        for i, p in enumerate(prefixes):
            pf[i, :len(p)] = p
            pl[i] = len(p)
        verdicts = np.zeros(n, dtype=T.VERDICT_DTYPE)
        traces = np.zeros((n, T.DPOR_MAX_TRACE), dtype=T.DPOR_TRACE_DTYPE)
        tl = np.zeros(n, dtype=np.uint32)
        ig = np.zeros((n, 4), dtype=np.uint64)
        wc = np.zeros((n, 4), dtype=np.uint64)
        alts = np.zeros((n, max(1, max_alts)), dtype=T.DPOR_WILD_ALT_DTYPE)
        na = np.zeros(n, dtype=np.uint32)
        self._check(lib().demi_dpor_wildcard_batch(self._h, pf.ctypes.data, pl.ctypes.data, stride, n, C.byref(params),
                                                   1 if stop_after_next_trace else 0, max_alts, verdicts.ctypes.data, traces.ctypes.data,
                                                   tl.ctypes.data, ig.ctypes.data, wc.ctypes.data, alts.ctypes.data, na.ctypes.data))
        bits = lambda row: [64 * q + b for q in range(4) for b in range(64) if (int(row[q]) >> b) & 1]
        return (verdicts, [traces[i, :tl[i]].copy() for i in range(n)], [bits(ig[i]) for i in range(n)], [bits(wc[i]) for i in range(n)],
                [alts[i, :na[i]].copy() for i in range(n)])

    def wildcard_dpor_test(self, initial, params, dpor_budget=0, batch=1, max_alts=0):
        """WildcardMinimizer.testWithDpor of one proposal (demi_wildcard_dpor_test): (the hit's executed trace or None, its sorted
        ignored positions, WcdporResult)."""
        import numpy as np
        init = np.ascontiguousarray(initial, dtype=T.DPOR_TRACE_DTYPE)
        out = np.zeros(T.DPOR_MAX_TRACE, dtype=T.DPOR_TRACE_DTYPE)
        wc = T.WcdporParams(dpor_budget, batch, max_alts, 0)
        res = T.WcdporResult()
        self._check(lib().demi_wildcard_dpor_test(self._h, init.ctypes.data if len(init) else None, len(init), C.byref(params), C.byref(wc),
                                                  out.ctypes.data, C.byref(res)))
        if not res.hit:
            return None, [], res
        return out[:res.trace_len].copy(), [64 * q + b for q in range(4) for b in range(64) if (int(res.ignored[q]) >> b) & 1], res

    def dpor_set_traces(self, original_trace=None, initial_trace=None):
        """ArvindDistanceOrdering.init(sched, originalTrace) and DPORwHeuristics.setInitialTrace for the following dpor_explore
        calls (DPOR_TRACE_DTYPE arrays; None clears)."""
        import numpy as np
        keys = np.ascontiguousarray(np.asarray(original_trace)["key"], dtype=np.uint64) if original_trace is not None else np.zeros(0, dtype=np.uint64)
        init = np.ascontiguousarray(initial_trace, dtype=T.DPOR_TRACE_DTYPE) if initial_trace is not None else np.zeros(0, dtype=T.DPOR_TRACE_DTYPE)
        self._check(lib().demi_dpor_set_traces(self._h, keys.ctypes.data if len(keys) else None, len(keys),
                                               init.ctypes.data if len(init) else None, len(init)))

    def edit_distance_dpor_ddmin(self, externals, initial_trace, params, ip=None, cap=4096, areas=None):
        """RunnerUtils.editDistanceDporDDMin natively (demi_edit_distance_dpor_ddmin: IncrementalDDMin over ResumableDPOR, every
        consultation K3 launches): (mcs indices, [(subsequence indices, passes, distance cap)] in consultation order,
        [(cap, MCS size)] per pass, the reproducing interleaving or None, stats).  areas: the payload area of every event of
        `externals` (a DEMI_MODEL_PAYLOADS table); the library gathers them for every subsequence it consults.  None: P0 / P1."""
        import numpy as np
        ev = np.ascontiguousarray(externals, dtype=T.EXT_EVENT_DTYPE)
        if areas is not None:
            self.ext_payload_areas(areas)
        init = np.ascontiguousarray(initial_trace, dtype=T.DPOR_TRACE_DTYPE)
        ip = ip or T.IncDdminParams()
        mcs = np.zeros(4, dtype=np.uint64)
        consulted = np.zeros((cap, 4), dtype=np.uint64)
        passed = np.zeros(cap, dtype=np.uint8)
        dist = np.zeros(cap, dtype=np.uint32)
        vt = np.zeros(T.DPOR_MAX_TRACE, dtype=T.DPOR_TRACE_DTYPE)
        st = T.IncDdminStats()
        self._check(lib().demi_edit_distance_dpor_ddmin(self._h, ev.ctypes.data if len(ev) else None, len(ev), init.ctypes.data, len(init),
                                                        C.byref(params), C.byref(ip), mcs.ctypes.data, consulted.ctypes.data, passed.ctypes.data,
                                                        dist.ctypes.data, cap, vt.ctypes.data, C.byref(st)))
        n = min(cap, st.consultations)
        return T.mask_to_events(mcs), [(T.mask_to_events(consulted[i]), bool(passed[i]), int(dist[i])) for i in range(n)], \
            [(int(st.pass_distance[i]), int(st.pass_mcs_len[i])) for i in range(min(16, st.passes))], \
            (vt[:st.violation_len].copy() if st.violation_len else None), st

    @staticmethod
    def dpor_buffers(max_interleavings):
        """Output arrays for dpor_explore(..., buffers=...) - what a host that calls demi_dpor_explore repeatedly keeps (a JVM's
        arrays): allocated and touched once, so that a call's time is the library's and not the page faults of fresh arrays."""
        import numpy as np
        cap = int(max_interleavings)
        b = (np.zeros(cap, dtype=T.VERDICT_DTYPE), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32),
             np.zeros(T.DPOR_MAX_TRACE, dtype=T.DPOR_TRACE_DTYPE))
        for a in b:
            a.view(np.uint8)[::4096] = 0          # (np.zeros maps its pages lazily)
        return b

    def dpor_explore(self, params, search, buffers=None):
        """The whole exploration natively: returns (verdicts, prefix_len, rounds, first violating trace, stats).  With `buffers`
        (dpor_buffers) the results are VIEWS of those arrays - valid until the next call that uses them."""
        import numpy as np
        cap = search.max_interleavings
        if buffers is not None:
            verdicts, plen, rounds, vt = buffers
            assert len(verdicts) >= cap and len(plen) >= cap and len(rounds) >= cap
        else:
            verdicts = np.zeros(cap, dtype=T.VERDICT_DTYPE)
            plen = np.zeros(cap, dtype=np.uint32)
            rounds = np.zeros(cap, dtype=np.uint32)
            vt = np.zeros(T.DPOR_MAX_TRACE, dtype=T.DPOR_TRACE_DTYPE)
        vl = C.c_uint32(0)
        stats = T.DporStats()
        self._check(lib().demi_dpor_explore(self._h, C.byref(params), C.byref(search), verdicts.ctypes.data,
                                            plen.ctypes.data, rounds.ctypes.data, vt.ctypes.data, C.byref(vl), C.byref(stats)))
        n = int(stats.interleavings)
        if buffers is not None:
            return verdicts[:n], plen[:n], rounds[:int(stats.launches)], vt[:vl.value], stats
        return verdicts[:n].copy(), plen[:n].copy(), rounds[:int(stats.launches)].copy(), vt[:vl.value].copy(), stats

    def dpor_explored(self, index):
        """Interleaving `index` of the last dpor_explore: (next trace it was started from, shared length, executed trace)."""
        import numpy as np
        nt = np.zeros(T.DPOR_MAX_TRACE, dtype=T.DPOR_TRACE_DTYPE)
        tr = np.zeros(T.DPOR_MAX_TRACE, dtype=T.DPOR_TRACE_DTYPE)
        nl, sl, tl = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(lib().demi_dpor_explored(self._h, C.c_uint64(int(index)), nt.ctypes.data, C.byref(nl), C.byref(sl), tr.ctypes.data, C.byref(tl)))
        return nt[:nl.value].copy(), int(sl.value), tr[:tl.value].copy()

    # ---- multi-GPU (one process and one Context per GPU)
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the RCCL unique id (128 bytes) every rank passes to comm_create."""
        buf = C.create_string_buffer(128)
        rc = lib().demi_comm_unique_id(buf)
        if rc != 0:
            raise DemiError(rc, "RCCL unavailable")
        return buf.raw

    def comm_create(self, unique_id: bytes, rank: int, world: int):
        """RCCL communicator over xGMI (ncclCommInitRank: collective over the ranks)."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(lib().demi_comm_create(self._h, buf, rank, world))

    def comm_create_host(self, rank: int, world: int, allgather):
        """A communicator whose all-gather the host supplies: allgather(send: bytes) -> bytes of every rank's block in rank
        order (e.g. torch.distributed over gloo).  Blocks are staged through host memory."""
        def thunk(_user, send, recv, nbytes):
            try:
                out = allgather(C.string_at(send, nbytes))
                C.memmove(recv, out, len(out))
                return 0
            except Exception:        # reported as DEMI_ERR_DEVICE by the library
                return 1
        self._allgather_cb = ALLGATHER_FN(thunk)          # keep the callback alive as long as the communicator
        self._check(lib().demi_comm_create_host(self._h, rank, world, self._allgather_cb, None))

    def comm_destroy(self):
        self._check(lib().demi_comm_destroy(self._h))

    def comm_rank(self):
        r, w = C.c_int(0), C.c_int(1)
        self._check(lib().demi_comm_rank(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_allgather_dev(self, d_send_ptr, d_recv_ptr, nbytes, stream=None):
        self._check(lib().demi_comm_allgather_dev(self._h, C.c_void_p(d_send_ptr), C.c_void_p(d_recv_ptr), nbytes, stream))

    def random_explore_sharded(self, n_total, limits, seed_base=0, cap=1 << 16):
        """n_total schedules split by index range over the communicator's ranks; the merged violation set on every rank."""
        import numpy as np
        out = np.zeros(cap, dtype=T.VIOLATION_DTYPE)
        cnt = C.c_uint64(0)
        self._check(lib().demi_random_explore_sharded(self._h, C.c_uint64(seed_base), n_total, C.byref(limits), out.ctypes.data,
                                                      cap, C.byref(cnt)))
        return out[:min(cnt.value, cap)].copy(), int(cnt.value)

    def replay_batch_sharded(self, masks, limits):
        import numpy as np
        masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(len(masks), dtype=T.VERDICT_DTYPE)
        if len(masks):
            self._check(lib().demi_replay_batch_sharded(self._h, masks.ctypes.data, len(masks), C.byref(limits), out.ctypes.data))
        return out

    def provenance_prune(self, traces, affected_masks):
        """demi_provenance_prune: traces = sequence of DPOR_TRACE_DTYPE arrays, affected_masks = one actor bitmask per trace;
        returns a list of index arrays (the kept events of every trace)."""
        import numpy as np
        n = len(traces)
        if n == 0:
            return []
        stride = max(1, max(len(t) for t in traces))
        buf = np.zeros((n, stride), dtype=T.DPOR_TRACE_DTYPE)
        lens = np.zeros(n, dtype=np.uint32)
        for i, t in enumerate(traces):
            buf[i, :len(t)] = t
            lens[i] = len(t)
        aff = np.ascontiguousarray(affected_masks, dtype=np.uint32)
        assert len(aff) == n
        words = T.DPOR_MAX_TRACE // 64
        keep = np.zeros((n, words), dtype=np.uint64)
        self._check(lib().demi_provenance_prune(self._h, buf.ctypes.data, lens.ctypes.data, aff.ctypes.data, stride, n, keep.ctypes.data))
        out = []
        for i in range(n):
            bits = np.unpackbits(keep[i].view(np.uint8), bitorder="little")[:int(lens[i])]
            out.append(np.nonzero(bits)[0].astype(np.int64))
        return out

    def device_probe(self, waves_per_simd=1, iters=20000, kind=0):
        """Shader clock under load (GHz) and SIMD cycles per wave64 instruction of the probe's kind: 0 integer VALU,
        1 SALU, 2 VALU / SALU alternating, 3 a divergent `if`, 4 - 7 one opcode alone: v_add_u32, v_mul_lo_u32, v_mul_hi_u32,
        v_mad_u64_u32 (demi_device_probe_mix)."""
        r = T.ProbeResult()
        self._check(lib().demi_device_probe_mix(self._h, waves_per_simd, iters, kind, C.byref(r)))
        return r

    def calib_rw(self, mode, nbytes, repeats=1):
        self._check(lib().demi_calib_rw(self._h, mode, nbytes, repeats))

    def random_get_trace_carried(self, seed, exec_index, limits):
        """(verdict, recorded events, executed index) of execution `exec_index` of the carried-generator instance seeded `seed`."""
        import numpy as np
        rec = np.zeros(T.MAX_REC_EVENTS, dtype=T.REC_EVENT_DTYPE)
        v = T.Verdict()
        n, ran = C.c_uint32(0), C.c_uint32(0)
        self._check(lib().demi_random_get_trace_carried(self._h, C.c_uint64(seed), exec_index, C.byref(limits), C.byref(v),
                                                        rec.ctypes.data, len(rec), C.byref(n), C.byref(ran)))
        return v, rec[:n.value].copy(), ran.value

    def random_get_trace(self, seed, limits):
        import numpy as np
        rec = np.zeros(T.MAX_REC_EVENTS, dtype=T.REC_EVENT_DTYPE)
        v = T.Verdict()
        n = C.c_uint32(0)
        self._check(lib().demi_random_get_trace(self._h, C.c_uint64(seed), C.byref(limits), C.byref(v),
                                                rec.ctypes.data, len(rec), C.byref(n)))
        return v, rec[:n.value].copy()
