// k2_wildcard_cand.hpp — K2W over (candidate, proposal) work items: one consultation of WildcardTestOracle.test
// (minification/wildcard_minimization/WildcardTestOracle.scala:33-61) per candidate, the oracle of RunnerUtils.wildcardDDMin.
//
// A consultation runs WildcardMinimizer(skipClockClusters = true): ClockClusterizer with Aggressiveness.STOP_IMMEDIATELY proposes
// the trace with every timer, then the trace without the first, the second, ... timer (in id order), and stops at the first
// proposal that reproduces the violation.  The proposals do not depend on each other's outcome, so a speculative DDMin frontier
// is candidates x (1 + timers) independent replays.  The replay is k2_wildcard_body.hpp, the body of k2_replay_wildcard, unchanged; what is new is
// where a work item's external mask and presence come from, the executed length counted without a record buffer, and the
// reduction of a candidate's proposals on the device (the body's last lines under K2W_CAND, then k2w_cand_finish).
#pragma once

#include "k2_wildcard.hpp"

namespace demi {

__global__ __launch_bounds__(K2W_WAVES * 64) void k2_replay_wildcard_candidates(const K2WCandArgs cargs) {
  const K2WArgs& args = cargs.a;
  const K2WCand& cand = cargs.c;
#define K2W_CAND 1
#include "k2_wildcard_body.hpp"
#undef K2W_CAND
}

#ifndef DEMI_JIT_A     // (not part of a specialised module: it reads no table)
// one thread per candidate, after the replays: the record the host reads.  rec_len = events of the loaded trace.
__global__ void k2w_cand_finish(const unsigned long long* key, const uint32_t* first_ovf, const demi_verdict* plane, uint32_t n_cand,
                                uint32_t n_drop, uint32_t rec_len, demi_wildcard_candidate* out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;
  const unsigned long long k = key[c];
  const uint32_t hit = (uint32_t)(k >> 32), ovf = first_ovf[c];
  demi_wildcard_candidate r;
  r.first_hit = hit; r.executed_len = 0; r.flags = 0; r.first_ovf = ovf; r.hash = 0;
  if (ovf < hit) {
    r.flags = DEMI_WC_UNKNOWN;               // the sequential loop meets the aborted replay first (also: no hit at all)
  } else if (hit != 0xFFFFFFFFu) {
    r.executed_len = (uint32_t)k;
    r.hash = plane[(size_t)c * (n_drop + 1u) + hit].hash;
    r.flags = DEMI_WC_REPRODUCES | (r.executed_len > rec_len ? DEMI_WC_LONGER : 0u);
  }
  out[c] = r;
}
#endif

}  // namespace demi
