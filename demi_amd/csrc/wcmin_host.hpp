// wcmin_host.hpp — wildcard (fungible-clock) minimization natively on the host, around wildcard rounds: WildcardMinimizer
// (minification/wildcard_minimization/WildcardMinimizer.scala:44-242) with TestScheduler.STSSched and its Clusterizers
// (Clusterizer.scala, OneAtATimeClusterizer.scala, ClockClusterizer.scala), restated as demi_amd/wildcard_minimization.py
// restates them: class for class, line for line.
//
// Host control only, and no HIP: the replays are the ROUND oracle's.  A Clusterizer proposes its traces one after another, each
// assuming the one before it failed, so the upcoming proposals are enumerated on a copy and one round evaluates them together; the
// real Clusterizer is then advanced by the calls the sequential loop would have made.  The result, total_replays and the
// record_internal_size sequence are the sequential algorithm's.  Per adoption the loop needs the winner's kept marks (the
// deliveries ignored as absent go back to getNextTrace) and its executed length (`ret.size <= minTrace.size`, :217); the adopted
// TRACE is fetched once per doMinimize, for the last row that satisfied the length rule.
//
// A delivery's id is the Uniq id of its UniqueMsgEvent (demi_rec_event.id); `sorted` sequences are sorted by it, as in the Scala.
// A proposal is a presence bitmask over the recorded events (bit i of word i / 64), as demi_replay_wildcard_batch takes it.
//
// Round oracle (the library: the context; the test harness: a file of recorded answers):
//   int selectors(const uint32_t* type_sets, const uint8_t* policies)     one per recorded event of the LOADED execution;
//   int round(const uint64_t* present, uint32_t n, uint32_t words, uint8_t* out_kept, demi_wildcard_round_result* r)
//       the n proposals over the loaded execution; out_kept [its length] and r as demi_replay_wildcard_round defines them;
//   int get_trace(const uint64_t* present, std::vector<demi_rec_event>* out)
//       the executed trace of one proposal that reproduces (demi_replay_wildcard_get_trace); counts as one launch;
//   int load(const demi_rec_event* trace, uint32_t n)                      make `trace` the loaded execution (same externals).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <set>
#include <unordered_map>
#include <vector>

#include "../../include/demi_gpu.h"

namespace demi_host {

typedef std::set<int64_t> IdSet;                 // a Set[Int] of Uniq ids (-1: "none yet", as in the Scala)
typedef std::vector<uint64_t> PresenceRow;

// the table's side of MessageFingerprinter and EventTypes
struct WcModel {
  const uint8_t* msg_class;                      // [n_msg_types]: external iff DEMI_MSG_EXTERNAL (EventTypes.isExternal)
  uint32_t n_msg_types;
  uint32_t n_payloads;                           // DEMI_MODEL_PAYLOADS_N of the table
  uint32_t clock_increment_types;                // causesClockIncrement
  const uint8_t* clock_field;                    // getLogicalClock: payload field per type, 255 = none
};

// The UniqueMsgEvents of a trace: record index, Uniq id, message type, external or not, clock hooks (_Deliveries).
struct WcDeliveries {
  uint32_t n_rec = 0;
  std::vector<uint32_t> idx, types;
  std::vector<int64_t> ids, clock;               // clock: -1 = None
  std::vector<uint8_t> external, clock_inc;
  bool unique = true;                            // "Must be UniqueMsgEvent"

  WcDeliveries(const demi_rec_event* ev, uint32_t n, const WcModel& m) : n_rec(n) {
    IdSet seen;
    for (uint32_t i = 0; i < n; i++) {
      if (ev[i].kind != DEMI_REC_MSG_EVENT) continue;
      const uint32_t t = ev[i].msg_type;
      idx.push_back(i);
      ids.push_back((int64_t)ev[i].id);
      unique &= seen.insert((int64_t)ev[i].id).second;
      types.push_back(t);
      external.push_back(t < m.n_msg_types && m.msg_class[t] == DEMI_MSG_EXTERNAL);
      clock_inc.push_back(t < 32 && ((m.clock_increment_types >> t) & 1u));
      const uint32_t k = t < DEMI_MAX_MSG_TYPES ? m.clock_field[t] : 255u;
      clock.push_back(k == 255u ? -1 : (int64_t)DEMI_REC_PAYLOAD(ev[i], m.n_payloads, k));
    }
  }
  uint32_t words() const { return (n_rec + 63) / 64; }
  // the trace that holds the external deliveries and the deliveries whose id is in `include`
  PresenceRow present(const IdSet& include) const {
    PresenceRow p(words(), 0);
    for (size_t k = 0; k < idx.size(); k++)
      if (external[k] || include.count(ids[k])) p[idx[k] >> 6] |= 1ull << (idx[k] & 63u);
    return p;
  }
};

inline IdSet set_minus(const IdSet& a, const IdSet& b) {
  IdSet r;
  for (int64_t x : a) if (!b.count(x)) r.insert(x);
  return r;
}
inline IdSet set_and(const IdSet& a, const IdSet& b) {
  IdSet r;
  for (int64_t x : a) if (b.count(x)) r.insert(x);
  return r;
}
inline void set_add(IdSet& a, const IdSet& b) { a.insert(b.begin(), b.end()); }

// Clusterizer.scala.  next_trace returns false for None.  clone() is a deep copy.
class Clusterizer {
 public:
  virtual ~Clusterizer() {}
  virtual bool next_trace(bool violation_reproduced_last_run, const IdSet& ignored_absent_ids, PresenceRow* out) = 0;
  virtual void selectors(std::vector<uint32_t>* type_sets, std::vector<uint8_t>* policies) const = 0;
  virtual std::unique_ptr<Clusterizer> clone() const = 0;
  virtual const WcDeliveries& deliveries() const = 0;
};

// OneAtATimeClusterizer.scala: pick an event to remove, wildcard all the others.
class SingletonClusterizer : public Clusterizer {
 public:
  SingletonClusterizer(std::shared_ptr<const WcDeliveries> d, uint32_t policy) : d_(d), policy_(policy) {
    for (size_t k = 0; k < d_->ids.size(); k++) {
      if (!d_->external[k]) sorted_ids_.push_back(d_->ids[k]);       // getIdsToRemove
      all_ids_.insert(d_->ids[k]);
    }
    std::sort(sorted_ids_.begin(), sorted_ids_.end());
  }
  bool next_trace(bool reproduced, const IdSet& ignored_absent_ids, PresenceRow* out) override {
    if (head_ >= sorted_ids_.size()) return false;
    if (reproduced) {
      set_add(successfully_removed_, ignored_absent_ids);
      successfully_removed_.insert(ignored_last_run_);
    }
    if (!first_run_) ignored_last_run_ = sorted_ids_[head_++];
    else first_run_ = false;
    IdSet gone(successfully_removed_);
    gone.erase(ignored_last_run_);                                    // successfullyRemoved - ignoredLastRun
    *out = d_->present(set_minus(all_ids_, gone));
    return true;
  }
  void selectors(std::vector<uint32_t>* ts, std::vector<uint8_t>* po) const override {
    ts->assign(d_->n_rec, 0); po->assign(d_->n_rec, 0);
    for (size_t k = 0; k < d_->idx.size(); k++) {
      if (d_->external[k]) continue;
      (*ts)[d_->idx[k]] = 1u << d_->types[k];                        // the class tag
      (*po)[d_->idx[k]] = (uint8_t)policy_;
    }
  }
  std::unique_ptr<Clusterizer> clone() const override { return std::unique_ptr<Clusterizer>(new SingletonClusterizer(*this)); }
  const WcDeliveries& deliveries() const override { return *d_; }

 private:
  std::shared_ptr<const WcDeliveries> d_;
  uint32_t policy_;
  std::vector<int64_t> sorted_ids_;
  size_t head_ = 0;                              // sortedIds = sorted_ids_[head_ ..]
  IdSet all_ids_, successfully_removed_;
  int64_t ignored_last_run_ = -1;
  bool first_run_ = true;
};

enum : uint32_t { WC_AGGR_NONE = 0, WC_AGGR_ALL_TIMERS_FIRST_ITR = 1, WC_AGGR_STOP_IMMEDIATELY = 2 };   // ClockClusterizer.scala:12-21

// ClockClusterIterator (ClockClusterizer.scala:138-228): the first iteration includes all events.
class ClockClusterIterator {
 public:
  explicit ClockClusterIterator(const WcDeliveries* d) : d_(d) {
    for (size_t k = 0; k < d->ids.size(); k++)
      if (!d->clock_inc[k] && d->clock[k] >= 0) all_ids_.insert(d->ids[k]);
    clocks_ = compute_remaining_clocks();
  }
  std::vector<int64_t> compute_remaining_clocks() const {
    const int64_t lowest = head_ < clocks_.size() ? clocks_[head_] : 0;
    std::set<int64_t> vals;
    for (size_t k = 0; k < d_->ids.size(); k++)
      if (!blacklist_.count(d_->ids[k]) && d_->clock[k] >= 0) vals.insert(d_->clock[k]);
    std::vector<int64_t> r;
    for (int64_t c : vals) if (c >= lowest) r.push_back(c);
    return r;
  }
  IdSet current() const {
    const int64_t current_clock_to_remove = first_cluster_removal_ ? -1 : next_clock_to_remove_;
    IdSet out;
    for (size_t k = 0; k < d_->ids.size(); k++) {
      if (d_->clock_inc[k]) continue;                                 // handled by OneAtATimeIterator
      if (d_->clock[k] < 0 || !(d_->clock[k] == current_clock_to_remove || blacklist_.count(d_->ids[k]))) out.insert(d_->ids[k]);
    }
    return out;
  }
  IdSet next() {
    if (first_cluster_removal_) {
      IdSet ret = current();
      first_cluster_removal_ = false;
      return ret;
    }
    next_clock_to_remove_ = clocks_[head_];
    IdSet ret = current();
    head_++;
    return ret;
  }
  bool has_next() const { return first_cluster_removal_ || head_ < clocks_.size(); }
  void produced_violation(const IdSet& previously_included, const IdSet& ignored_absents) {
    set_add(blacklist_, set_minus(all_ids_, previously_included));   // inverse
    if (!ignored_absents.empty()) {
      set_add(blacklist_, set_and(all_ids_, ignored_absents));
      std::vector<int64_t> c = compute_remaining_clocks();
      clocks_.swap(c);
      head_ = 0;
    }
  }
  size_t clocks_left() const { return clocks_.size() - head_; }

 private:
  const WcDeliveries* d_;
  IdSet all_ids_, blacklist_;
  bool first_cluster_removal_ = true;
  int64_t next_clock_to_remove_ = -1;
  std::vector<int64_t> clocks_;
  size_t head_ = 0;                              // clocks = clocks_[head_ ..]
};

// OneAtATimeIterator (ClockClusterizer.scala:230-290): all timers, then all but the first, all but the second, ...
class OneAtATimeIterator {
 public:
  OneAtATimeIterator() {}
  explicit OneAtATimeIterator(const IdSet& all) : all_(all), to_remove_(all.begin(), all.end()) {}
  IdSet current() const {
    IdSet r = set_minus(all_, blacklist_);
    if (!first_) r.erase(to_remove_[head_]);
    return r;
  }
  IdSet next() {
    IdSet ret = current();
    if (first_) first_ = false;
    else head_++;
    return ret;
  }
  bool has_next() const { return first_ || head_ < to_remove_.size(); }
  void produced_violation(const IdSet& previously_included, const IdSet& ignored_absents) {
    set_add(blacklist_, set_minus(all_, previously_included));       // inverse
    set_add(blacklist_, set_and(all_, ignored_absents));
  }
  void reset() {
    const IdSet left = set_minus(all_, blacklist_);
    to_remove_.assign(left.begin(), left.end());
    head_ = 0;
    first_ = true;
  }

 private:
  IdSet all_, blacklist_;
  std::vector<int64_t> to_remove_;
  size_t head_ = 0;                              // toRemove = to_remove_[head_ ..]
  bool first_ = true;
};

// ClockClusterizer.scala:23-135: cluster the deliveries by their logical clock, and for every cluster try the timers (the messages
// that cause a clock increment) one at a time.
class ClockClusterizer : public Clusterizer {
 public:
  ClockClusterizer(std::shared_ptr<const WcDeliveries> d, uint32_t policy, uint32_t clock_increment_types, uint32_t aggressiveness,
                   bool skip_clock_clusters)
      : d_(d), policy_(policy), inc_set_(clock_increment_types), aggressiveness_(aggressiveness), skip_(skip_clock_clusters),
        cluster_iterator_(d.get()) {
    current_cluster_ = cluster_iterator_.next();                      // start by not removing any clusters
    IdSet timers;
    for (size_t k = 0; k < d_->ids.size(); k++) if (d_->clock_inc[k]) timers.insert(d_->ids[k]);
    timer_iterator_ = OneAtATimeIterator(timers);
  }
  bool next_trace(bool reproduced, const IdSet& ignored_absent_ids, PresenceRow* out) override {
    if (reproduced) {
      timer_iterator_.produced_violation(current_timers_, ignored_absent_ids);
      cluster_iterator_.produced_violation(current_cluster_, ignored_absent_ids);
    }
    if (!timer_iterator_.has_next() ||
        (aggressiveness_ == WC_AGGR_ALL_TIMERS_FIRST_ITR && reproduced && !trying_first_cluster_) ||
        (aggressiveness_ == WC_AGGR_STOP_IMMEDIATELY && reproduced)) {
      trying_first_cluster_ = false;
      if (!cluster_iterator_.has_next() || skip_) return false;
      timer_iterator_.reset();
      current_cluster_ = cluster_iterator_.next();
    }
    current_timers_ = timer_iterator_.next();                         // (reset() above: hasNext holds)
    IdSet both(current_timers_);
    set_add(both, current_cluster_);
    *out = d_->present(both);
    return true;
  }
  void selectors(std::vector<uint32_t>* ts, std::vector<uint8_t>* po) const override {
    ts->assign(d_->n_rec, 0); po->assign(d_->n_rec, 0);
    for (size_t k = 0; k < d_->idx.size(); k++) {
      if (d_->external[k]) continue;
      if (d_->clock_inc[k]) {            // timers bypass the resolutionStrategy: lst.indexWhere(causesClockIncrement)
        (*ts)[d_->idx[k]] = inc_set_; (*po)[d_->idx[k]] = (uint8_t)DEMI_WILDCARD_FIRST;
      } else {
        (*ts)[d_->idx[k]] = 1u << d_->types[k]; (*po)[d_->idx[k]] = (uint8_t)policy_;
      }
    }
  }
  // (the iterator points at the deliveries the shared_ptr keeps alive: a copy shares them)
  std::unique_ptr<Clusterizer> clone() const override { return std::unique_ptr<Clusterizer>(new ClockClusterizer(*this)); }
  const WcDeliveries& deliveries() const override { return *d_; }

 private:
  std::shared_ptr<const WcDeliveries> d_;
  uint32_t policy_, inc_set_, aggressiveness_;
  bool skip_;
  ClockClusterIterator cluster_iterator_;
  IdSet current_cluster_;
  bool trying_first_cluster_ = true;
  OneAtATimeIterator timer_iterator_;
  IdSet current_timers_;
};

struct WcminOutcome {
  std::vector<demi_rec_event> trace;        // minTrace
  std::vector<uint32_t> sizes;              // record_internal_size after every sequential replay, and the fencepost entry
  std::vector<uint32_t> batches;            // proposals per round
  demi_wcmin_stats stats;
};

inline uint32_t wc_count_msg_events(const std::vector<demi_rec_event>& t) {
  uint32_t c = 0;
  for (const demi_rec_event& e : t) c += e.kind == DEMI_REC_MSG_EVENT;
  return c;
}

// WildcardMinimizer.doMinimize (:182-240) over `start`, which the oracle holds loaded.  On return *min_trace is minTrace (`start`
// itself without an adoption that satisfied the length rule).  On an error of the oracle the last adopted trace is fetched and
// loaded where that is still possible, and *min_trace holds it.
template <class Oracle>
int wc_do_minimize(Clusterizer& clusterizer, const std::vector<demi_rec_event>& start, const demi_wcmin_params* par, Oracle&& oracle,
                   WcminOutcome* out, std::vector<demi_rec_event>* min_trace) {
  const uint32_t max_batch = std::min<uint32_t>(par->max_batch ? par->max_batch : 16384u, DEMI_MAX_REC_EVENTS);   // (what one round holds)
  const WcDeliveries& d = clusterizer.deliveries();
  if (!d.unique) return DEMI_ERR_INVALID_TRACE;
  const uint32_t words = d.words();
  demi_wcmin_stats& st = out->stats;
  *min_trace = start;
  size_t min_len = start.size();                 // len(minTrace.events)
  uint32_t min_deliveries = wc_count_msg_events(start);
  PresenceRow min_row;                           // the row whose executed trace minTrace is
  bool have_min = false;                         // (false: minTrace is startTrace itself)
  {
    std::vector<uint32_t> ts;
    std::vector<uint8_t> po;
    clusterizer.selectors(&ts, &po);
    ts.push_back(0); po.push_back(0);            // (a trace without events: the pointers stay valid)
    const int rc = oracle.selectors(ts.data(), po.data());
    if (rc) return rc;
  }
  // the last adopted trace becomes minTrace (and, after an error, the loaded execution)
  auto fetch = [&](bool reload) -> int {
    if (!have_min) return DEMI_OK;
    min_row.push_back(0);                        // (a trace without events: the pointer stays valid)
    std::vector<demi_rec_event> got;
    int rc = oracle.get_trace(min_row.data(), &got);
    st.launches++; st.replays_run++;
    if (rc) return rc;
    min_trace->swap(got);
    return reload ? oracle.load(min_trace->data(), (uint32_t)min_trace->size()) : DEMI_OK;
  };
  bool last_reproduced = false;                  // what the next getNextTrace is told about the last run
  IdSet last_ignored;
  const IdSet none;
  std::vector<PresenceRow> cands;
  std::vector<uint64_t> flat;
  std::vector<uint8_t> kept;
  for (;;) {
    // the clusterizer's upcoming proposals, each assuming the one before it failed
    cands.clear();
    {
      std::unique_ptr<Clusterizer> spec = clusterizer.clone();
      bool rep = last_reproduced;
      const IdSet* ign = &last_ignored;
      PresenceRow p;
      while (cands.size() < max_batch) {
        if (!spec->next_trace(rep, *ign, &p)) break;
        cands.push_back(p);
        rep = false; ign = &none;
      }
    }
    if (cands.empty()) break;                    // (the real clusterizer's next proposal is None as well)
    const uint32_t n = (uint32_t)cands.size();
    flat.clear();
    for (const PresenceRow& p : cands) flat.insert(flat.end(), p.begin(), p.end());
    flat.push_back(0);
    kept.assign(start.size() + 1, 0);
    demi_wildcard_round_result r;
    memset(&r, 0, sizeof r);
    const int rc = oracle.round(flat.data(), n, words, kept.data(), &r);
    if (rc) { (void)fetch(true); return rc; }
    out->batches.push_back(n);
    st.rounds++; st.launches += r.launches; st.retried += r.retried; st.replays_run += (uint64_t)n + r.retried;
    const bool hit = r.first_hit != 0xFFFFFFFFu;
    if (hit && r.first_hit >= n) return DEMI_ERR_INVALID_ARG;
    const uint32_t consumed = hit ? r.first_hit + 1 : n;
    // bring the real clusterizer to where the sequential loop would be
    {
      bool rep = last_reproduced;
      const IdSet* ign = &last_ignored;
      PresenceRow p;
      for (uint32_t k = 0; k < consumed; k++) {
        if (!clusterizer.next_trace(rep, *ign, &p) || p != cands[k]) return DEMI_ERR_INVALID_ARG;   // (the copy and the clusterizer disagree: cannot happen)
        if (!par->skip_clock_clusters) out->sizes.push_back(min_deliveries);
        rep = false; ign = &none;
      }
    }
    st.total_replays += consumed;
    if (!hit) { last_reproduced = false; last_ignored.clear(); continue; }
    // test() returned Some(ret): ret.size <= minTrace.size decides whether it becomes minTrace (:217)
    st.adoptions++;
    const PresenceRow& won = cands[r.first_hit];
    IdSet ignored;                               // present deliveries that were ignored as absent (IgnoreAbsentCallback)
    uint32_t delivered = 0;
    for (size_t k = 0; k < d.idx.size(); k++) {
      const uint32_t i = d.idx[k];
      if (kept[i]) delivered++;
      else if ((won[i >> 6] >> (i & 63u)) & 1ull) ignored.insert(d.ids[k]);
    }
    if (r.executed_len <= min_len) {
      min_len = r.executed_len;
      min_row = won;
      have_min = true;
      min_deliveries = delivered;
    }
    last_reproduced = true;
    last_ignored.swap(ignored);
  }
  return fetch(false);
}

// WildcardMinimizer.minimize (:60-180) over the loaded execution `trace`.  Returns a demi_status.
template <class Oracle>
int wildcard_minimize(const demi_rec_event* trace, uint32_t n_rec, const WcModel& model, const demi_wcmin_params* par, Oracle&& oracle,
                      WcminOutcome* out) {
  out->sizes.clear(); out->batches.clear();
  memset(&out->stats, 0, sizeof out->stats);
  const std::vector<demi_rec_event> start(trace, trace + n_rec);
  out->trace = start;
  out->stats.deliveries_before = out->stats.deliveries_after = wc_count_msg_events(start);
  const uint32_t aggressiveness = par->skip_clock_clusters ? WC_AGGR_STOP_IMMEDIATELY : WC_AGGR_ALL_TIMERS_FIRST_ITR;
  std::unique_ptr<Clusterizer> clusterizer;
  std::shared_ptr<const WcDeliveries> d = std::make_shared<const WcDeliveries>(trace, n_rec, model);
  if (par->clustering == DEMI_CLUSTER_CLOCK || par->clustering == DEMI_CLUSTER_CLOCK_THEN_SINGLETON)
    clusterizer.reset(new ClockClusterizer(d, par->policy, model.clock_increment_types, aggressiveness, par->skip_clock_clusters != 0));
  else
    clusterizer.reset(new SingletonClusterizer(d, par->policy));
  std::vector<demi_rec_event> min_trace;
  int rc = wc_do_minimize(*clusterizer, start, par, oracle, out, &min_trace);
  out->trace = min_trace;
  out->stats.deliveries_after = wc_count_msg_events(out->trace);
  if (rc) return rc;
  if (par->clustering == DEMI_CLUSTER_CLOCK_THEN_SINGLETON) {
    // the second pass runs over minTrace, which becomes the loaded execution
    rc = oracle.load(out->trace.data(), (uint32_t)out->trace.size());
    if (rc) return rc;
    const std::vector<demi_rec_event> second(out->trace);
    d = std::make_shared<const WcDeliveries>(second.data(), (uint32_t)second.size(), model);
    SingletonClusterizer singleton(d, par->policy);
    rc = wc_do_minimize(singleton, second, par, oracle, out, &min_trace);
    out->trace = min_trace;
    out->stats.deliveries_after = wc_count_msg_events(out->trace);
    if (rc) return rc;
  }
  if (!par->skip_clock_clusters) out->sizes.push_back(out->stats.deliveries_after);          // fencepost
  out->stats.sizes = (uint32_t)out->sizes.size();
  return DEMI_OK;
}

}  // namespace demi_host
