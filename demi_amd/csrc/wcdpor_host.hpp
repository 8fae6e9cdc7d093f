// wcdpor_host.hpp — WildcardMinimizer.testWithDpor of one proposal around K3W launches (demi_wildcard_dpor_test).
// What stays on the host of the fresh DPORwHeuristics the reference builds per proposal (WildcardMinimizer.scala:84-105):
// the backtrack queue with DefaultBacktrackOrdering (highest branchI first, ties in creation order), the ExploredTacker over
// pairs of node keys, getNext() (DPORwHeuristics.scala:1142-1185 with skipBacktrackComputation: the next trace is replayThis
// alone), the budget as a count of interleavings, and what a wildcard does besides picking a message: setExplored for the one
// it took (:504-508) and a backtrack point per alternative (:485-497), rebuilt from the records of k3_wildcard.hpp.
// Up to `batch` queue heads run per launch and are committed one at a time; a committed interleaving's points that outrank
// the remaining heads are popped - and, not having run yet, launched - before them, so the commits are the reference's sequence.
// Host control only, and no HIP: who runs interleavings is the callable's business.
#pragma once

#include <map>
#include <set>
#include <utility>
#include <vector>
#include "../../include/demi_gpu.h"
#include "replay_host.hpp"

namespace demi_host {

typedef std::vector<demi_dpor_trace_entry> WcTrace;
struct WcInterleaving {            // what one interleaving of a K3W launch left
  demi_verdict v = {};
  WcTrace trace;
  uint64_t ignored[4] = {0, 0, 0, 0}, wild[4] = {0, 0, 0, 0};
  std::vector<demi_dpor_wild_alt> alts;
};
inline bool wc_capacity_abort(const WcInterleaving& r) {
  return (r.v.flags & (DEMI_V_PENDING_OVF | DEMI_V_QUEUE_OVF | DEMI_V_TRACE_OVF | DEMI_V_ALTS_OVF)) != 0;
}
// branchI of a backtrack point: the trace index of the last node of getCommonPrefix(priorEvent, toPlayNext) (:485-490) - the
// deepest common ancestor of entry a and entry b over the parent links (a parent's index is below its child's; the root is 0)
inline uint32_t wc_common_ancestor(const WcTrace& t, uint32_t a, uint32_t b) {
  while (a != b) { if (a > b) a = t[a].parent; else b = t[b].parent; }
  return a;
}

struct WcPoint { uint64_t prior = 0, alt = 0; WcTrace next; };

//   int run(const std::vector<const WcTrace*>& nexts, const demi_limits& l, WcInterleaving* out)
// runs nexts.size() interleavings in one launch with pending capacity l.p_max (DEMI_MAX_PENDING: the largest capacities)
template <class Run>
int wildcard_dpor_test(const WcTrace& initial, uint32_t p_max, uint32_t dpor_budget, uint32_t batch, Run&& run, WcTrace* hit_trace,
                       demi_wcdpor_result* r) {
  *r = demi_wcdpor_result();
  if (batch < 1) batch = 1;
  demi_limits lim = {};
  lim.p_max = p_max;
  std::map<std::pair<uint32_t, uint64_t>, WcPoint> queue;       // (255 - branchI, creation number): begin() is the head
  std::set<std::pair<uint64_t, uint64_t>> explored;
  std::map<uint64_t, WcInterleaving> ran;                       // speculated heads, by creation number
  uint64_t seq = 0, executed = 0;
  WcPoint cur;
  cur.next = initial;
  uint64_t cur_seq = ~0ull;
  for (;;) {
    // ---- the interleaving of `cur`: from the speculation, or a launch of it and of the heads behind it
    if (!ran.count(cur_seq)) {
      std::vector<const WcTrace*> nexts(1, &cur.next);
      std::vector<uint64_t> ids(1, cur_seq);
      for (auto it = queue.begin(); it != queue.end() && nexts.size() < batch; ++it) {
        if (explored.count({it->second.prior, it->second.alt}) || ran.count(it->first.second)) continue;
        nexts.push_back(&it->second.next);
        ids.push_back(it->first.second);
      }
      std::vector<WcInterleaving> out(nexts.size());
      const int rc = run(nexts, lim, out.data());
      if (rc) return rc;
      r->launches++;
      executed += nexts.size();
      for (size_t k = 0; k < ids.size(); k++) ran[ids[k]] = std::move(out[k]);
    }
    WcInterleaving il = std::move(ran[cur_seq]);
    ran.erase(cur_seq);
    r->interleavings++;
    // ---- an abort on a capacity is no answer (replay_host.hpp): once more with the largest capacities, then DEMI_ERR_CAPACITY
    if (wc_capacity_abort(il)) {
      BatchOutcome o;
      const std::vector<const WcTrace*> one(1, &cur.next);
      const int rc = decide_batch(1u, lim, &il,
                                  [&](const uint32_t*, uint32_t, const demi_limits& l, WcInterleaving* out) {
                                    if (l.p_max == lim.p_max) return (int)DEMI_OK;      // (the first evaluation is the one at hand)
                                    r->launches++;
                                    return run(one, l, out);
                                  },
                                  wc_capacity_abort, &o);
      r->retried += o.retried;
      if (rc) return rc;
    }
    if (il.v.flags & DEMI_V_SELFMSG) return DEMI_ERR_INVALID_TRACE;      // the reference throws (:631-633)
    // ---- what its wildcards did: the picked messages are explored, every alternative is a backtrack point
    const WcTrace& t = il.trace;
    for (uint32_t k = 1; k < t.size(); k++)
      if ((il.wild[k >> 6] >> (k & 63)) & 1ull) explored.insert({t[k - 1].key, t[k].key});
    for (const demi_dpor_wild_alt& a : il.alts) {
      if (a.trace_len < 1 || a.trace_len > t.size() || a.parent >= a.trace_len) return DEMI_ERR_DEVICE;
      WcPoint p;
      p.prior = t[a.trace_len - 1].key; p.alt = a.key;
      p.next.assign(t.begin() + 1, t.begin() + a.trace_len);       // currentTrace.tail
      demi_dpor_trace_entry e = {};
      e.key = a.key; e.word = a.word; e.kind = 1;
      p.next.push_back(e);                                          // toPlayNext
      if ((size_t)a.next_pos + 1 < cur.next.size()) p.next.insert(p.next.end(), cur.next.begin() + a.next_pos + 1, cur.next.end());
      const uint32_t branch = wc_common_ancestor(t, a.trace_len - 1u, a.parent);
      queue.emplace(std::make_pair(255u - branch, seq++), std::move(p));
      r->points++;
    }
    if (il.v.flags & DEMI_V_VIOLATION) {
      r->hit = 1;
      r->trace_len = (uint32_t)t.size();
      for (int k = 0; k < 4; k++) r->ignored[k] = il.ignored[k];
      *hit_trace = t;
      break;
    }
    // ---- dpor() (:1020-1185): the budget, then getNext
    if (dpor_budget && r->interleavings >= dpor_budget) { r->budget_reached = 1; break; }
    bool found = false;
    while (!queue.empty() && !found) {
      auto it = queue.begin();
      cur = std::move(it->second);
      cur_seq = it->first.second;
      queue.erase(it);
      if (explored.count({cur.prior, cur.alt})) { r->skipped_explored++; ran.erase(cur_seq); continue; }
      explored.insert({cur.prior, cur.alt});
      found = true;
    }
    if (!found) { r->exhausted = 1; break; }
  }
  r->speculated = (uint32_t)(executed - r->interleavings);
  return DEMI_OK;
}

}  // namespace demi_host
