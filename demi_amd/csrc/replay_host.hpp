// replay_host.hpp — the capacity rule of the replay path, and the round that stops at its first hit.
// A replay aborted on a capacity (DEMI_V_PENDING_OVF / DEMI_V_QUEUE_OVF) is no verdict.  It is run once more with
// p_max = DEMI_MAX_PENDING; if it still aborts, the call fails with DEMI_ERR_CAPACITY.  It is never reported as "does not
// reproduce".  Every minimizer on the replay path is sound because of this rule, so it is written here once.
// Host control only, and no HIP: who replays is the callables' business (the library: launches on the context; the harness
// tests/harness/replay_host_harness.cpp: scripted answers); they get the caller's limits, or a copy with the largest p_max.
// A callable's non-zero status ends the call and is returned as it is; when the RULE fails the functions return
// DEMI_ERR_CAPACITY and say which items are to blame - the caller words the message.
#pragma once

#include <algorithm>
#include <vector>
#include "../../include/demi_gpu.h"

namespace demi_host {
constexpr uint32_t kNone = 0xFFFFFFFFu;
// a p_max field (demi_limits, the DPOR parameters) as the capacity it stands for (0 is the default); whether nothing larger is
// left to run a replay again with; the limits for that second run
inline uint32_t p_max_of(uint32_t field) { return field ? field : 64u; }
inline bool p_max_is_largest(uint32_t field) { return p_max_of(field) >= (uint32_t)DEMI_MAX_PENDING; }
inline demi_limits at_largest(demi_limits l) { l.p_max = DEMI_MAX_PENDING; return l; }
// items evaluated a second time; items left without an answer (non-zero iff the rule failed)
struct BatchOutcome { uint32_t retried = 0, undecided = 0; };

// answers[0..n) of n items under the rule.
//   int eval(const uint32_t* idx, uint32_t m, const demi_limits& l, A* out)   out[k] = the answer of item idx[k] under l
//   bool undecided(const A&)                                                  this answer is an abort on a capacity
// The first evaluation is of every item under `lim` (idx == nullptr, m == n); the second and last, when there is one, of the
// undecided items, in order, at DEMI_MAX_PENDING.
template <class A, class Eval, class Undecided>
int decide_batch(uint32_t n, const demi_limits& lim, A* answers, Eval&& eval, Undecided&& undecided, BatchOutcome* o) {
  *o = BatchOutcome();
  const demi_limits big = at_largest(lim);
  int rc = eval(nullptr, n, lim, answers);
  if (rc) return rc;
  std::vector<uint32_t> idx;
  for (uint32_t i = 0; i < n; i++) if (undecided(answers[i])) idx.push_back(i);
  if (!idx.empty() && !p_max_is_largest(lim.p_max)) {
    std::vector<A> again(idx.size());
    rc = eval(idx.data(), (uint32_t)idx.size(), big, again.data());
    if (rc) return rc;
    o->retried = (uint32_t)idx.size();
    for (size_t k = 0; k < idx.size(); k++) answers[idx[k]] = again[k];
  }
  for (uint32_t i : idx) o->undecided += undecided(answers[i]) ? 1u : 0u;
  return o->undecided ? DEMI_ERR_CAPACITY : DEMI_OK;
}

// what one launch of a round reports, as indices into that launch: its first hit and its first abort on a capacity
struct RoundAnswer { uint32_t first_hit = kNone, first_ovf = kNone; };

// n proposals, each assuming the ones before it failed, at most `per` of them per launch:
//   int launch(uint32_t off, uint32_t count, const demi_limits& l, RoundAnswer* a)   proposals [off, off + count) under l
// An abort before the launch's first hit (anywhere, without a hit) is no answer: the proposals the sequential loop would have
// reached - first_hit + 1 of them, or the whole launch - run once more at DEMI_MAX_PENDING.  The round stops at the launch that
// holds a hit (the last launch made is then the one that found it).  r->launches, r->retried and r->first_hit (the round's
// index; kNone on entry) are counted here; when the rule fails, *failed is the round's index of the proposal that still aborts.
template <class R, class Launch>
int first_hit_round(uint32_t n, uint32_t per, const demi_limits& lim, Launch&& launch, R* r, uint32_t* failed) {
  *failed = kNone;
  const demi_limits big = at_largest(lim);
  for (uint32_t off = 0; off < n && r->first_hit == kNone; off += per) {
    const uint32_t c = std::min(per, n - off);
    RoundAnswer a;
    int rc = launch(off, c, lim, &a);
    if (rc) return rc;
    r->launches++;
    if (a.first_ovf < a.first_hit && !p_max_is_largest(lim.p_max)) {
      const uint32_t m = a.first_hit == kNone ? c : a.first_hit + 1;
      a = RoundAnswer();
      rc = launch(off, m, big, &a);
      if (rc) return rc;
      r->launches++;
      r->retried += m;
    }
    if (a.first_ovf < a.first_hit) {
      *failed = off + a.first_ovf;
      return DEMI_ERR_CAPACITY;
    }
    if (a.first_hit != kNone) r->first_hit = off + a.first_hit;
  }
  return DEMI_OK;
}

}  // namespace demi_host
