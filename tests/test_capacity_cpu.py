"""demi_amd/capacity.py without a device: the capacity rule over fake evaluation functions, through the batch cases of
tests/harness/replay_host_harness.cpp (the library's copy of the same rule) and the single-replay form."""
import numpy as np
import pytest

from demi_amd import types as T
from demi_amd.capacity import CapacityExceeded, OVF_FLAGS, aborted, decide_batch, decide_one, is_largest, largest


def limits(p_max):
    return T.Limits(0, 0, p_max, 1, 0x1234, 0)


class Fake:
    """Answers per item at the caller's capacity and at the largest (negative: undecided); records what it was asked."""

    def __init__(self, small, big):
        self.small, self.big = np.array(small, dtype=np.int64), np.array(big, dtype=np.int64)
        self.asked = []

    def __call__(self, lim, idx):
        self.asked.append((int(lim.p_max), None if idx is None else [int(i) for i in idx]))
        a = self.big if is_largest(lim.p_max) else self.small
        return a.copy() if idx is None else a[idx]


undecided = lambda a: a < 0


def test_nothing_undecided_is_one_evaluation():
    f = Fake([1, 2, 3], [7, 7, 7])
    v, again = decide_batch(f, limits(8), undecided, "no")
    assert v.tolist() == [1, 2, 3] and again == 0 and f.asked == [(8, None)]


def test_the_undecided_items_run_once_more_in_order_at_the_largest_capacity():
    f = Fake([1, -1, 3, -1, 5], [10, 20, 30, 40, 50])
    lim = limits(0)                                   # (0: the default, 64)
    v, again = decide_batch(f, lim, undecided, "no")
    assert v.tolist() == [1, 20, 3, 40, 5] and again == 2
    assert f.asked == [(0, None), (T.MAX_PENDING, [1, 3])] and lim.p_max == 0       # (the caller's limits are not touched)


def test_still_undecided_after_the_retry_raises_with_the_count():
    f = Fake([-1, 2, -1], [-1, 20, 30])
    with pytest.raises(CapacityExceeded, match="^1 left$"):
        decide_batch(f, limits(8), undecided, lambda n: "%d left" % n)
    assert len(f.asked) == 2


def test_a_capacity_that_is_already_the_largest_raises_after_one_evaluation():
    f = Fake([1, -1], [1, -1])
    with pytest.raises(CapacityExceeded, match="^beyond$"):
        decide_batch(f, limits(T.MAX_PENDING), undecided, "beyond")
    assert f.asked == [(T.MAX_PENDING, None)]


def test_verdict_arrays_and_the_single_replay():
    v = np.zeros(3, dtype=T.VERDICT_DTYPE)
    v["flags"] = [T.V_VIOLATION, T.V_PENDING_OVF, T.V_QUEUE_OVF | T.V_VIOLATION]
    assert aborted(v).tolist() == [False, True, True] and OVF_FLAGS == T.V_PENDING_OVF | T.V_QUEUE_OVF
    big = largest(limits(8))
    assert big.p_max == T.MAX_PENDING and big.looking_for == 0x1234 and is_largest(big.p_max) and not is_largest(0) and not is_largest(T.MAX_PENDING - 1)

    def replay(flags_small, flags_big, runs):
        def run(lim):
            runs.append(int(lim.p_max))
            return T.Verdict(flags_big if is_largest(lim.p_max) else flags_small, 0, 0), "kept at %d" % lim.p_max
        return run
    runs = []
    assert decide_one(replay(T.V_VIOLATION, 0, runs), limits(8))[1] == "kept at 8" and runs == [8]
    runs = []
    r = decide_one(replay(T.V_PENDING_OVF, T.V_VIOLATION, runs), limits(8))
    assert r[0].flags == T.V_VIOLATION and r[1] == "kept at %d" % T.MAX_PENDING and runs == [8, T.MAX_PENDING]
    runs = []
    with pytest.raises(CapacityExceeded, match="the replay exceeds the engine's capacities"):
        decide_one(replay(T.V_QUEUE_OVF, T.V_QUEUE_OVF, runs), limits(8))
    assert runs == [8, T.MAX_PENDING]
    runs = []
    with pytest.raises(CapacityExceeded):
        decide_one(replay(T.V_QUEUE_OVF, T.V_QUEUE_OVF, runs), limits(T.MAX_PENDING))
    assert runs == [T.MAX_PENDING]


def test_schedulers_re_exports_the_names_callers_import():
    from demi_amd import schedulers
    assert schedulers.CapacityExceeded is CapacityExceeded and schedulers.OVF_FLAGS == OVF_FLAGS
