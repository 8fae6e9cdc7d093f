// intmin_host.hpp — internal-event minimization natively on the host, around removal rounds: STSSchedMinimizer.minimize
// (minification/internal_minimization/ScheduleCheckers.scala:35-107) with the OneAtATimeStrategy family
// (OneAtATimeRemoval.scala:17-131: LeftToRightOneAtATime :134-139, SrcDstFIFORemoval :141-251), as RunnerUtils.minimizeInternals
// (RunnerUtils.scala:980-1003) sets them up.
//
// Host control only, and no HIP: the replays are the ROUND oracle's.  A strategy proposes its candidates one after another, each
// assuming the one before it failed, so the upcoming proposals are enumerated on a clone and one round evaluates them together; the
// real strategy is then advanced by the calls the sequential loop would have made.  The result, total_replays and the
// record_internal_size sequence are the sequential algorithm's (tests: this loop over the CPU oracle against the Python mirror
// demi_amd/internal_minimization.py, which restates the same walk, and the GPU against both).
//
// Round oracle (the library: demi_replay_removal_round on the context; the test harness: the CPU oracle's removal replay):
//   int round(const uint32_t* skip, uint32_t n, uint8_t* out_kept, demi_removal_round_result* r)
//       the n proposals over the LOADED execution; out_kept [its length] and r as demi_replay_removal_round defines them;
//   int load(const demi_rec_event* trace, uint32_t n)
//       make `trace` the loaded execution (same externals).
#pragma once

#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/demi_gpu.h"

namespace demi_host {

// (snd, rcv, MessageFingerprint) of a delivery: on the table-encoded model the fingerprint is the message type and the whole
// payload area (p0, p1 and p_hi of demi_rec_event, 16 bits each)
struct DeliveryKey {
  uint64_t area;      // p0 | p1 << 16 | p_hi << 32
  uint32_t head;      // snd | rcv << 8 | msg_type << 16
  bool operator==(const DeliveryKey& o) const { return area == o.area && head == o.head; }
  uint32_t snd() const { return head & 0xFFu; }
  uint32_t rcv() const { return (head >> 8) & 0xFFu; }
  uint32_t msg_type() const { return (head >> 16) & 0xFFu; }
  uint16_t pair() const { return (uint16_t)(head & 0xFFFFu); }
};
struct DeliveryKeyHash {
  size_t operator()(const DeliveryKey& k) const {
    uint64_t h = (k.area ^ ((uint64_t)k.head << 40)) * 0x9E3779B97F4A7C15ULL;
    return (size_t)(h ^ (h >> 31));
  }
};
inline DeliveryKey delivery_key(const demi_rec_event& e) {
  return DeliveryKey{DEMI_REC_AREA(e), (uint32_t)e.snd | ((uint32_t)e.rcv << 8) | ((uint32_t)e.msg_type << 16)};
}
// MultiSet[(String, String, MessageFingerprint)]
typedef std::unordered_map<DeliveryKey, int32_t, DeliveryKeyHash> DeliveryMultiset;

// RunnerUtils.countMsgEvents (RunnerUtils.scala:1315-1323)
inline uint32_t count_msg_events(const std::vector<demi_rec_event>& t) {
  uint32_t c = 0;
  for (const demi_rec_event& e : t) c += e.kind == DEMI_REC_MSG_EVENT;
  return c;
}

static constexpr uint32_t INTMIN_NONE = 0xFFFFFFFFu;

// OneAtATimeStrategy with its two choice filters.  Copying it is clone().
class OneAtATimeStrategy {
 public:
  // msg_class [n_msg_types]: the application's external-message filter (EventTypes.setExternalMessageFilter,
  // ExternalEvents.scala:157-166) is msg_class == DEMI_MSG_EXTERNAL.  dead_letters: 15, or 31 for a table of more than 8 actors.
  OneAtATimeStrategy(const demi_rec_event* verified_mcs, uint32_t n, const uint8_t* msg_class, uint32_t n_msg_types,
                     uint32_t dead_letters, uint32_t strategy)
      : fifo_(strategy == DEMI_REMOVAL_SRC_DST_FIFO), dead_(dead_letters) {
    for (uint32_t i = 0; i < n; i++) {
      if (verified_mcs[i].kind != DEMI_REC_MSG_EVENT) continue;
      const DeliveryKey k = delivery_key(verified_mcs[i]);
      verified_.push_back(k);
      // external messages are never ignored: they count as already tried (:32-35)
      if (k.msg_type() < n_msg_types && msg_class[k.msg_type()] == DEMI_MSG_EXTERNAL) { tried_[k]++; unignorable_++; }
      if (fifo_ && k.snd() != dead_) fifo_len_[k.pair()]++;
    }
  }
  OneAtATimeStrategy clone() const { return *this; }
  uint32_t unignorable() const { return unignorable_; }

  // getNextTrace (:57-124) as an index: the delivery of `trace` the next schedule drops, INTMIN_NONE when done
  uint32_t next_index(const std::vector<demi_rec_event>& trace, const DeliveryMultiset& already_removed, bool violation_triggered) {
    if (fifo_) fifo_before(already_removed, violation_triggered);
    // keysThisIteration counts the occurrences seen so far, plus everything pruned earlier
    DeliveryMultiset keys(already_removed);
    for (uint32_t i = 0; i < trace.size(); i++) {
      if (trace[i].kind != DEMI_REC_MSG_EVENT) continue;
      const DeliveryKey k = delivery_key(trace[i]);
      const int32_t seen = ++keys[k];
      int32_t& tried = tried_[k];
      if (seen > tried && choice_filter(k)) { tried++; return i; }
    }
    return INTMIN_NONE;
  }

 private:
  // SrcDstFIFORemoval.getNextTrace before it defers to OneAtATimeStrategy (:211-247)
  void fifo_before(const DeliveryMultiset& already_removed, bool violation_triggered) {
    if (!violation_triggered && have_prev_) fifo_len_.erase(prev_);           // ignoring didn't work: the pair is done
    if (violation_triggered) {
      // some FIFO entries may have been pruned as absent "freebies": recompute, in reverse (:222-243)
      fifo_len_.clear();
      DeliveryMultiset removed(already_removed);
      for (size_t i = verified_.size(); i-- > 0;) {
        const DeliveryKey& k = verified_[i];
        if (k.snd() == dead_) continue;
        auto it = removed.find(k);
        if (it != removed.end() && it->second > 0) it->second--;
        else fifo_len_[k.pair()]++;
      }
    }
    fifo_seen_.clear();                                                       // srcDstToCurrentIdx = -1 for every pair
  }
  // LeftToRightOneAtATime: everything (:134-139).  SrcDstFIFORemoval.choiceFilter (:180-205): per (src, dst) pair only the last
  // message of the FIFO; timers and externals' deliveries (sender deadLetters) in trace order.  The reference keeps each pair's
  // fingerprints in a Vector but only ever compares its LENGTH with the running index, so the length is what is kept here.
  bool choice_filter(const DeliveryKey& k) {
    if (!fifo_) return true;
    auto it = fifo_len_.find(k.pair());
    if (it != fifo_len_.end()) {
      const uint32_t idx = fifo_seen_[k.pair()]++;                           // srcDstToCurrentIdx after its increment
      if (idx == it->second - 1) {
        if (--it->second == 0) fifo_len_.erase(it);
        prev_ = k.pair(); have_prev_ = true;
        return true;
      }
    }
    have_prev_ = false;
    return k.snd() == dead_;
  }

  bool fifo_;
  uint32_t dead_;
  uint32_t unignorable_ = 0;
  std::vector<DeliveryKey> verified_;                       // the deliveries of verified_mcs
  DeliveryMultiset tried_;                                  // triedIgnoring
  std::unordered_map<uint16_t, uint32_t> fifo_len_;         // srcDstToMessages (lengths), absent = no entry
  std::unordered_map<uint16_t, uint32_t> fifo_seen_;        // srcDstToCurrentIdx + 1
  uint16_t prev_ = 0;                                       // previouslyChosenSrcDst
  bool have_prev_ = false;
};

struct IntminOutcome {
  std::vector<demi_rec_event> trace;        // lastFailingTrace
  std::vector<uint32_t> sizes;              // record_internal_size after every sequential replay
  std::vector<uint32_t> batches;            // candidates per round
  demi_intmin_stats stats;
};

// STSSchedMinimizer.minimize over the loaded execution `verified_mcs`.  Returns a demi_status; on an error of the oracle
// out->trace is the last adopted trace, which is also what the oracle holds loaded.
template <class Oracle>
int sts_sched_minimize(const demi_rec_event* verified_mcs, uint32_t n_rec, const uint8_t* msg_class, uint32_t n_msg_types,
                       uint32_t dead_letters, const demi_intmin_params* par, Oracle&& oracle, IntminOutcome* out) {
  const uint32_t max_batch = par->max_batch ? par->max_batch : 16384u;
  OneAtATimeStrategy strategy(verified_mcs, n_rec, msg_class, n_msg_types, dead_letters, par->strategy);
  std::vector<demi_rec_event>& last = out->trace;           // lastFailingTrace
  last.assign(verified_mcs, verified_mcs + n_rec);
  out->sizes.clear(); out->batches.clear();
  demi_intmin_stats& st = out->stats;
  memset(&st, 0, sizeof st);
  st.unignorable = strategy.unignorable();
  uint32_t last_size = count_msg_events(last);
  st.deliveries_before = st.deliveries_after = last_size;
  DeliveryMultiset pruned_overall;
  bool violation_triggered = false;
  std::vector<uint32_t> cands;
  std::vector<uint8_t> kept;
  std::vector<demi_rec_event> executed;
  for (;;) {
    // the strategy's upcoming proposals, each assuming the one before it failed
    {
      OneAtATimeStrategy spec = strategy.clone();
      cands.clear();
      bool vt = violation_triggered;
      while (cands.size() < max_batch) {
        const uint32_t i = spec.next_index(last, pruned_overall, vt);
        if (i == INTMIN_NONE) break;
        cands.push_back(i);
        vt = false;
      }
    }
    if (cands.empty()) break;
    const uint32_t n = (uint32_t)cands.size();
    kept.assign(last.size() + 1, 0);
    demi_removal_round_result r;
    memset(&r, 0, sizeof r);
    const int rc = oracle.round(cands.data(), n, kept.data(), &r);
    if (rc) return rc;
    out->batches.push_back(n);
    st.rounds++; st.launches += r.launches; st.retried += r.retried; st.replays_run += (uint64_t)n + r.retried;
    const bool hit = r.first_hit != INTMIN_NONE;
    if (hit && r.first_hit >= n) return DEMI_ERR_INVALID_ARG;
    const uint32_t consumed = hit ? r.first_hit + 1 : n;
    // bring the real strategy to where the sequential loop would be
    {
      bool vt = violation_triggered;
      for (uint32_t k = 0; k < consumed; k++) {
        const uint32_t i = strategy.next_index(last, pruned_overall, vt);
        if (i != cands[k]) return DEMI_ERR_INVALID_ARG;       // (the clone and the strategy disagree: cannot happen)
        vt = false;
      }
    }
    st.total_replays += consumed;
    out->sizes.insert(out->sizes.end(), hit ? consumed - 1 : consumed, last_size);
    if (!hit) { violation_triggered = false; continue; }      // cut by max_batch, or the next proposal is None (the loop ends above)
    // test() returned Some(executed trace): the kept subset of the recorded events
    executed.clear();
    for (size_t i = 0; i < last.size(); i++) if (kept[i]) executed.push_back(last[i]);
    // other deliveries may have been pruned by virtue of being absent (:58-92): prunedThisRun, a multiset difference
    DeliveryMultiset diff;
    for (const demi_rec_event& e : last) if (e.kind == DEMI_REC_MSG_EVENT) diff[delivery_key(e)]++;
    for (const demi_rec_event& e : executed) if (e.kind == DEMI_REC_MSG_EVENT) diff[delivery_key(e)]--;
    for (const auto& kv : diff) if (kv.second > 0) pruned_overall[kv.first] += kv.second;
    last.swap(executed);
    last_size = count_msg_events(last);
    st.deliveries_after = last_size;
    st.adoptions++;
    out->sizes.push_back(last_size);
    violation_triggered = true;
    const int lrc = oracle.load(last.data(), (uint32_t)last.size());
    if (lrc) return lrc;
  }
  return DEMI_OK;
}

}  // namespace demi_host
