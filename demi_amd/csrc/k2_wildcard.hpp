// k2_wildcard.hpp — K2W: one STSScheduler.test per wavefront lane of a trace whose internal deliveries are WILDCARDS:
// the replay oracle of the wildcard (fungible-clock) minimizers, minification/wildcard_minimization/*.scala.
//
// Restates, on top of what k2_replay.hpp restates for exact deliveries,
//   * STSScheduler.messagePending for MsgEvent(snd, rcv, WildCardMatch(selector, _)) (schedulers/STSScheduler.scala:380-402):
//     the selector sees ALL pending messages of (snd, rcv) sorted by Uniq id (= send order); pending iff it returns an index
//     and the receiver is not blocked; otherwise advanceReplay ignores the event ("Ignoring message", :528-529);
//   * STSScheduler.schedule_new_message for the same event (:696-711): the selector sees the HEADS of the fingerprint groups
//     of (snd, rcv), the groups sorted by their head's id, and the chosen group's head is dequeued;
//   * the selectors that exist when the backtrack setter is a no-op (TestScheduler.STSSched): a class-tag filter ("same
//     message type") resolved by an AmbiguityResolutionStrategy (AmbiguityResolutionStrategies.scala) - SrcDstFIFOOnly: the
//     head of the list must match; BackTrackStrategy / FirstAndLastBacktrack: the first match; LastOnlyStrategy: the last
//     match - and ClockClusterizer's timer wildcard, indexWhere(causesClockIncrement): the first match.  Every selector is
//     therefore (a 32-bit set of message types, a policy HEAD / FIRST / LAST); type set 0 is the exact delivery of K2.
// Which message a wildcard takes depends on the SEND ORDER within the (snd, rcv) pair, and its payload may differ from the
// recorded one: the word counters of k2_replay<true> ("equal (snd, rcv, fingerprint) are interchangeable") cannot serve it.
// The pending set is the scanning variant's array (hot slots in LDS, HBM spill: LaneMem) with a per-lane sequence number
// per entry in the aux plane; swap-remove stays, and the reference's orders are minima / maxima of the sequence numbers:
//   exact      the oldest entry with the expected word (Queue.dequeue of its fingerprint group);
//   HEAD       the oldest entry of (snd, rcv), if its type is in the set;
//   FIRST      the oldest entry of (snd, rcv) whose type is in the set (also the head of the first matching group);
//   LAST       pending iff any entry matches; taken: among the matching entries that are the oldest of their word (the group
//              heads), the youngest - the head of the last matching group, which is NOT the youngest matching message when
//              that one has an older twin.
// notify_timer_cancel (:828-855) removes the oldest pending timer message of that fingerprint.
//
// lane = candidate: the external mask of K2 plus a PRESENCE bitmask over the recorded events (bit i: the MsgEvent recorded at
// index i is part of the trace; it generalises K2's `skip` from one removed delivery to a set; other kinds ignore their bit).
// A wave takes lanes_per_wave candidates at a time (K2's small-launch shaping); every lane walks its own replay - lanes of a
// wave deliver different messages to different receivers, so there is no lock step to keep.  A minimizer's batch is
// 10 .. 10^3 candidates, each one replay's dependent chain long: this kernel is latency-bound.
// filter_known_absents == 0 only; tables of up to 8 actors: narrow, DEMI_MODEL_WIDE, and with DEMI_MODEL_PAYLOADS (the whole
// 48-bit area in every message word formed, compared or recorded) and DEMI_MODEL_ARRAY (the array words are state words:
// initialised, carved and hashed with the fields).  The host refuses the rest.
#pragma once

#include "sim_core.hpp"

#ifndef DEMI_VM_RUN   // the table interpreter, unless a specialised build supplies the compiled handlers (jit.hpp)
#define DEMI_VM_RUN vm_run
#endif

namespace demi {

enum : uint32_t { K2W_HEAD = 0, K2W_FIRST = 1, K2W_LAST = 2 };   // demi_wildcard_policy
constexpr int K2W_WAVES = 4;

struct K2WArgs {
  const DevModel* model;
  const uint64_t* ext;      // original external events [n_ext]
  uint32_t n_ext;
  uint32_t exists;
  const uint64_t* expected; // lowered original trace [n_exp] (k2_replay.hpp: the lowering without the actors' MsgSends)
  const uint64_t* exp_area; // DEMI_MODEL_WIDE tables only: [n_exp] payload area of the expected event's message
  const uint64_t* sel;      // [n_exp] bits 0..31: type set (0 = exact); 32..39: policy; 40..63: recorded index
  uint32_t n_exp;
  uint32_t n_rec;           // recorded events of the loaded trace: the presence masks have present_words = ceil(n_rec / 64) words
  uint32_t present_words;
  uint32_t p_max, looking_for;
  uint32_t lanes_per_wave;
  const uint64_t* masks;    // [n][4]; null = every external kept
  const uint64_t* present;  // [n][present_words]
  uint8_t* kept;            // [n][n_exp] (pre-zeroed) 1 where the expected event took effect, or null
  demi_rec_event* rec_out;  // [n][rec_cap] the executed trace (every MsgSend, delivered or not), or null
  uint32_t* rec_n;          // [n] events of the executed trace (may exceed rec_cap: then the buffer holds the first rec_cap)
  uint32_t rec_cap;
  uint64_t n;
  demi_verdict* out;
  unsigned long long* work_counter;
  uint32_t* spill;
};

__host__ __device__ inline size_t k2w_lds_bytes(uint32_t code_len, uint32_t n_ext, uint32_t n_hs, uint32_t n_actors, bool wide = WIDE_TU,
                                                uint32_t hot = PEND_HOT, uint32_t arr_words = ARR_WORDS) {
  return tables_lds_bytes(code_len, n_ext, n_hs, wide, arr_words, false) + K2W_WAVES * lane_mem_wave_bytes(n_actors, true, hot, wide, DEMI_FX_CAP, arr_words);
}

// The candidates launch (k2_replay_wildcard_candidates below): work item = (candidate c, proposal j), c < n_cand, j <= n_drop.
// Candidate c has the external mask masks[c]; proposal 0 keeps every delivery of the base presence row, proposal j >= 1 drops
// the MsgEvent recorded at drops[j - 1] - the proposals of ClockClusterizer(skipClockClusters, STOP_IMMEDIATELY), which do not
// depend on each other's outcome (WildcardTestOracle.test, one DDMin consultation).  The launch reduces the proposals of a
// candidate on the device: key[c] = min over the reproducing proposals of j << 32 | executed length, first_ovf[c] = min over
// the proposals that were aborted on a capacity of j.
struct K2WCand {
  const uint64_t* base_present;   // [present_words] shared by the launch, or null = all ones
  const uint32_t* drops;          // [n_drop] recorded indices
  uint32_t n_drop;
  unsigned long long* key;        // [n_cand], preset to ~0
  uint32_t* first_ovf;            // [n_cand], preset to ~0
};
struct K2WCandArgs { K2WArgs a; K2WCand c; };

// The body of both kernels is k2_wildcard_body.hpp, included once per kernel with K2W_CAND 0 / 1 (a textual include, so that
// k2_replay_wildcard stays the code it was: same parameter accesses, same instructions).  K2W_CAND 1: args.n counts work items,
// args.masks is [n_cand][4], args.present / kept / rec_out are unused, args.out is the full [n_cand][1 + n_drop] plane.
// k2_wildcard_round.hpp includes it a third time, K2W_CAND 0 with K2W_ROUND 1: the rows and the kept plane of this kernel, the
// executed length and the reduction of the candidates kernel (one key / first_ovf word per launch).
__global__ __launch_bounds__(K2W_WAVES * 64) void k2_replay_wildcard(const K2WArgs args) {
  const K2WCand cand = {};
#define K2W_CAND 0
#include "k2_wildcard_body.hpp"
#undef K2W_CAND
}

}  // namespace demi
