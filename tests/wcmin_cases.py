"""What the tests of the native WildcardMinimizer (demi_minimize_wildcards, csrc/wcmin_host.hpp) share: the workloads, the Python
mirror W.WildcardMinimizer run over the transliterated device with every replay memoised and recorded, and the recorded rounds
written down as a case file for tests/harness/wcmin_host_harness.cpp.  Not a test file."""
import struct

import numpy as np

from demi_amd import types as T
from demi_amd import wildcard_minimization as W
from demi_amd.schedulers import MinimizationStats, SchedulerConfig

from . import test_wildcard_transliteration_cpu as X
from . import wildcard_payload_cases as Pc

CLUSTERINGS = {"ClockClusterizer": T.CLUSTER_CLOCK, "SingletonClusterizer": T.CLUSTER_SINGLETON, "ClockThenSingleton": T.CLUSTER_CLOCK_THEN_SINGLETON}
# policy name -> (transliterated strategy, mirror strategy): HEAD, FIRST, LAST
POLICIES = {"HEAD": "SrcDstFIFOOnly", "FIRST": "BackTrackStrategy", "LAST": "LastOnlyStrategy"}
_memo = {}


def workload(oracle, name):
    """(model, trace, fingerprint, device class): narrow0 / narrow1 - the narrow raft with election_budget 2, two skips of
    X.raft5_workload; real3 - the three-node real-field table's full violating execution; array5 - the ARRAY-only table."""
    if ("w", name) not in _memo:
        if name in ("narrow0", "narrow1"):
            w = X.raft5_workload(oracle, X.WORKLOAD_SKIPS[int(name[-1])], **X.WORKLOAD_MODEL) + (X.TransliteratedDevice,)
        elif name == "real3":
            w = Pc.get(oracle, Pc.WORKLOADS["real3"][0]) + (Pc.AreaTransliteratedDevice,)
        else:
            w = Pc.get(oracle, Pc.WORKLOADS[name][0]) + (Pc.AreaTransliteratedDevice,)
        _memo["w", name] = w
    return _memo["w", name]


class RecordingDevice:
    """Stands in for StsWildcardOracle over a transliterated device: every replay is run once per (loaded trace, selectors, presence
    row) and remembered; `segments` lists, per load, the rows asked for with their answers."""

    def __init__(self, device, cache):
        self.device, self.cache = device, cache
        self.segments = []
        self.launches = 0
        self.adoptions = 0                    # executed() calls that returned a trace

    def load(self, trace, type_sets, policies):
        self.device.load(trace, type_sets, policies)
        self._key = (T.rec_events(trace.events).tobytes(), np.asarray(type_sets, dtype=np.uint32).tobytes(), np.asarray(policies, dtype=np.uint8).tobytes())
        self.segments.append(dict(trace=T.rec_events(trace.events), type_sets=np.asarray(type_sets, dtype=np.uint32),
                                  policies=np.asarray(policies, dtype=np.uint8), rows={}))

    def _run(self, present, violation):
        present = np.asarray(present, dtype=bool)
        key = self._key + (present.tobytes(),)
        if key not in self.cache:
            d = self.device
            run = Pc.run_candidate if isinstance(d, Pc.AreaTransliteratedDevice) else X.run_candidate
            v, kept, executed, ignored, _ = run(d.oracle, d.model, d.trace, violation, d.wild, present)
            self.cache[key] = (bool(v[0] & T.V_VIOLATION), np.asarray(kept, dtype=np.uint8).copy(), T.rec_events(executed), set(ignored), v)
        r = self.cache[key]
        self.segments[-1]["rows"].setdefault(present.tobytes(), dict(present=present, reproduces=r[0], kept=r[1], executed=r[2], fetched=False))
        return r

    def test_batch(self, presents, violation):
        self.launches += 1
        return [self._run(p, violation)[0] for p in presents]

    def executed(self, present, violation):
        from demi_amd.schedulers import EventTrace
        ok, kept, executed, ignored, _ = self._run(present, violation)
        if not ok:
            return None
        self.segments[-1]["rows"][np.asarray(present, dtype=bool).tobytes()]["fetched"] = True
        self.adoptions += 1
        t = self.device.trace
        return EventTrace(executed.copy(), t.original_externals, t.ext_areas), set(ignored)


def mirror(oracle, name, clustering, policy, skip_clock, max_batch):
    """The Python mirror at this max_batch (0 = its default) over the transliterated device: dict(trace, total_replays,
    internal_sizes, batches, adoptions, segments).  Computed once per case; the replays are shared between the cases."""
    key = ("m", name, clustering, policy, skip_clock, max_batch)
    if key not in _memo:
        model, trace, fp, device = workload(oracle, name)
        dev = RecordingDevice(device(oracle, model), _memo.setdefault(("replays", name), {}))
        stats = MinimizationStats()
        m = W.WildcardMinimizer(SchedulerConfig(model=model), trace.original_externals, trace, fp, skipClockClusters=bool(skip_clock),
                                resolutionStrategy=X.STRATEGIES[POLICIES[policy]][1](), clusteringStrategy=clustering, stats=stats,
                                max_batch=max_batch or (1 << 14), oracle=dev)
        _, got = m.minimize()
        _memo[key] = dict(trace=T.rec_events(got.events), total_replays=stats.total_replays, internal_sizes=list(m.internal_sizes),
                          batches=list(m.batches), adoptions=dev.adoptions, segments=dev.segments)
    return _memo[key]


def params_of(model, clustering, policy, skip_clock, max_batch):
    return T.WcminParams(CLUSTERINGS[clustering], X.STRATEGIES[POLICIES[policy]][1].policy, skip_clock, max_batch,
                         model.clock_increment_types, model.clock_field)


def write_case(path, model, trace, par, segments):
    """CASE of tests/harness/wcmin_host_harness.cpp (little endian; its header comment is the format)."""
    rec = T.rec_events(trace.events)
    with open(path, "wb") as f:
        f.write(struct.pack("<9I", 0x314D4357, par.clustering, par.policy, par.skip_clock_clusters, par.max_batch, par.clock_increment_types,
                            model.n_msg_types, model.payloads, len(rec)))
        f.write(bytes(par.clock_field))
        f.write(np.asarray(model.msg_class, dtype=np.uint8).tobytes())
        f.write(rec.tobytes())
        f.write(struct.pack("<I", len(segments)))
        for s in segments:
            n = len(s["trace"])
            f.write(struct.pack("<2I", n, len(s["rows"])))
            f.write(s["trace"].tobytes())
            f.write(s["type_sets"].astype("<u4").tobytes())
            f.write(s["policies"].astype(np.uint8).tobytes())
            for r in s["rows"].values():
                words = (n + 63) // 64
                bits = np.zeros(words * 64, dtype=np.uint8)
                bits[:n] = r["present"]
                has_trace = 1 if r["fetched"] else 0
                f.write(struct.pack("<3I", 1 if r["reproduces"] else 0, len(r["executed"]), has_trace))
                f.write(np.packbits(bits, bitorder="little").tobytes())
                f.write(np.asarray(r["kept"], dtype=np.uint8)[:n].tobytes())
                if has_trace:
                    f.write(r["executed"].tobytes())


def read_result(path):
    raw = open(path, "rb").read()
    status, n_trace, n_sizes, n_batches, adoptions, rounds, total = struct.unpack_from("<6IQ", raw, 0)
    off = struct.calcsize("<6IQ")
    trace = np.frombuffer(raw, dtype=T.REC_EVENT_DTYPE, count=n_trace, offset=off)
    off += n_trace * T.REC_EVENT_DTYPE.itemsize
    sizes = np.frombuffer(raw, dtype="<u4", count=n_sizes, offset=off).tolist()
    off += 4 * n_sizes
    batches = np.frombuffer(raw, dtype="<u4", count=n_batches, offset=off).tolist()
    assert off + 4 * n_batches == len(raw)
    return dict(status=np.int32(np.uint32(status)).item(), trace=trace, sizes=sizes, batches=batches, adoptions=adoptions, rounds=rounds,
                total_replays=total)
