"""The capacity rule of the replay path, once for every Python mirror (csrc/replay_host.hpp is the library's copy): a replay aborted
on a capacity (DEMI_V_PENDING_OVF / DEMI_V_QUEUE_OVF) is no verdict.  It is run once more with p_max = DEMI_MAX_PENDING; if it still
aborts - or p_max already was the largest - the call raises CapacityExceeded.  It is never reported as "does not reproduce"."""
import numpy as np

from . import types as T


class CapacityExceeded(RuntimeError):
    """An execution needed more than the engine's largest capacities (pending set of DEMI_MAX_PENDING messages, the
    timer queues, DEMI_FX_CAP effects per delivery): its verdict is invalid (DEMI_V_PENDING_OVF / DEMI_V_QUEUE_OVF) and the
    reference, which has no such capacities, must decide it (JVM fallback)."""


OVF_FLAGS = T.V_PENDING_OVF | T.V_QUEUE_OVF


def is_largest(p_max: int) -> bool:
    """nothing larger to run a replay again with (a p_max field of 0 is the default, 64)"""
    return (p_max or 64) >= T.MAX_PENDING


def largest(lim: T.Limits) -> T.Limits:
    """a copy of `lim` with the largest pending set"""
    big = T.Limits.from_buffer_copy(lim)
    big.p_max = T.MAX_PENDING
    return big


def aborted(v) -> np.ndarray:
    """undecided, for VERDICT_DTYPE answers"""
    return (v["flags"] & OVF_FLAGS) != 0


def decide_batch(evaluate, lim: T.Limits, undecided, message):
    """The answers of a batch under the rule: (answers, how many were evaluated again).
    evaluate(lim, idx): a numpy array with the answers of the items idx (an index array; None: all of them) under `lim`;
    undecided(answers): a bool per answer; message: CapacityExceeded's text, or a function of the number of items left undecided."""
    v = evaluate(lim, None)
    bad = np.nonzero(undecided(v))[0]
    if len(bad) and not is_largest(lim.p_max):
        v[bad] = evaluate(largest(lim), bad)
    left = int(undecided(v[bad]).sum()) if len(bad) else 0
    if left:
        raise CapacityExceeded(message(left) if callable(message) else message)
    return v, len(bad)


def decide_one(run, lim: T.Limits, message="the replay exceeds the engine's capacities"):
    """One replay under the rule.  run(lim) -> (verdict, ...): what it returned, at the largest pending set if it had to be."""
    r = run(lim)
    if (int(r[0].flags) & OVF_FLAGS) and not is_largest(lim.p_max):
        r = run(largest(lim))
    if int(r[0].flags) & OVF_FLAGS:
        raise CapacityExceeded(message)
    return r
