"""Shared inputs of the suites of the pipelined fuzz campaign (tests/test_fuzz_pipeline_*.py): the numpy restatement of the host
loop that demi_fuzz_launch_summary is tested against, the crafted flag / verdict planes, and the (tests_per_launch, max_tests)
pairs of the campaign comparison with the launch that must hold the first violating test - asserted on the mirror and the oracle
alone in tests/test_fuzz_pipeline_cpu.py, so that a GPU comparison that passes has compared the positions it claims to."""
import numpy as np

from demi_amd import types as T

OVF = T.V_PENDING_OVF | T.V_QUEUE_OVF

# the existing campaign workload (tests/test_fuzz_campaign_gpu.py: CAMPAIGN_SEED, CAMPAIGN_EPC): tests 0 .. 15 are clean, test 16
# violates first.  (tests_per_launch, max_tests, the launch that holds the first violating test or None, where that launch lies)
CAMPAIGN_FIRST = 16
CAMPAIGN_CASES = [(64, 40, 0, "first"), (8, 40, 2, "middle"), (8, 20, 2, "partial_last"), (3, 40, 5, "middle"), (3, 17, 5, "partial_last"),
                  (1, 20, 16, "middle"), (1, 13, None, "none"), (3, 13, None, "none"), (8, 13, None, "none"), (64, 13, None, "none")]


def launch_of_first(tests_per_launch, max_tests, first=CAMPAIGN_FIRST):
    """(the launch that holds test `first`, the number of launches, the tests of that launch) or (None, launches, 0)"""
    launches = (max_tests + tests_per_launch - 1) // tests_per_launch
    if first >= max_tests:
        return None, launches, 0
    k = first // tests_per_launch
    return k, launches, min(tests_per_launch, max_tests - k * tests_per_launch)


def summary_reference(flags, verdicts):
    """the host loop of demi_fuzz_campaign over one launch: (first_hit, capacity_aborts, exec_index, aborted_before, verdict bytes),
    or "device" where that loop fails with DEMI_ERR_DEVICE (a flagged test none of whose verdicts violates)"""
    n, epc = verdicts.shape
    hit, aborts = n, 0
    for i in range(n):
        if flags[i] & 1:
            hit = i
            break
        if flags[i] & 2:
            aborts += 1
    if hit == n:
        return n, aborts, epc, 0, bytes(T.VERDICT_DTYPE.itemsize)
    row = verdicts[hit]
    k = 0
    while k < epc and not row["flags"][k] & T.V_VIOLATION:
        k += 1
    if k == epc:
        return "device"
    before = 1 if any(row["flags"][j] & OVF for j in range(k)) else 0
    return hit, aborts, k, before, row[k].tobytes()


def plane(n_tests, executions, hits=(), aborts=(), both=(), viol_at=None, abort_at=()):
    """flags [n_tests] and verdicts [n_tests, executions]: `hits` tests flagged violating, `aborts` flagged aborted, `both` with both
    bits; every flagged-violating test violates in execution viol_at (default 0) and has aborted executions at abort_at; every
    verdict carries its own position in fingerprint and hash, so that the record's verdict names where it was read"""
    flags = np.zeros(n_tests, dtype=np.uint32)
    v = np.zeros((n_tests, executions), dtype=T.VERDICT_DTYPE)
    # (filled by column so that a plane of 70 001 x 1 or 65 x 4 097 costs nothing)
    idx = np.arange(n_tests * executions, dtype=np.uint64).reshape(n_tests, executions)
    v["fingerprint"] = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    v["hash"] = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    v["flags"] = T.V_MAXMSG                                     # (a flag that is neither a violation nor an abort)
    for i in aborts:
        flags[i] |= 2
        v["flags"][i, executions // 2] |= T.V_PENDING_OVF
    for i in list(hits) + list(both):
        flags[i] |= 1
        k = 0 if viol_at is None else viol_at
        v["flags"][i, k] |= T.V_VIOLATION
        if k + 1 < executions:
            v["flags"][i, executions - 1] |= T.V_VIOLATION      # (a later violation must not win)
        for j in abort_at:
            v["flags"][i, j] |= T.V_QUEUE_OVF if j & 1 else T.V_PENDING_OVF
            flags[i] |= 2
    for i in both:
        flags[i] |= 2
    return flags, v


def summary_tuple(s):
    return int(s.first_hit), int(s.capacity_aborts), int(s.exec_index), int(s.aborted_before), bytes(s.verdict)
