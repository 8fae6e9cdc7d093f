// k2_wildcard_round.hpp — one ROUND of WildcardMinimizer.doMinimize (minification/wildcard_minimization/WildcardMinimizer.scala:
// 182-240) on the device: the wildcard counterpart of k2_removal_round.hpp.
//
// A Clusterizer proposes its traces one after another, each assuming the one before it failed, and the sequential loop adopts the
// FIRST that still triggers the violation; of that one it needs the deliveries that were ignored as absent (fed back to
// getNextTrace) and the length of the executed trace (`ret.size <= minTrace.size`, :217).  So after the replay of a round's n
// proposals the host needs the lowest reproducing index with its executed length, the lowest index aborted on a capacity (an
// aborted replay before the first hit is no verdict), and the winner's verdict and kept marks - not n verdicts and a second,
// recording replay of the winner.
//
//   k2_replay_wildcard_round  k2_wildcard_body.hpp a third time: explicit presence rows and the kept plane as k2_replay_wildcard,
//                             the executed length counted without a record buffer and the vector atomicMin on two words as
//                             k2_replay_wildcard_candidates (cand.key[0] = index << 32 | length over the reproducing proposals,
//                             cand.first_ovf[0] = the lowest aborted index).  A minimum does not depend on the order of the atomics.
//   k2w_round_pick            one workgroup behind it on the same stream (a kernel boundary: no flag, no fence): writes the record
//                             and copies the winner's n_exp-byte row of the kept plane behind it.
//
// The host reads K2W_ROUND_HEAD + n_exp bytes.
#pragma once

#include "k2_wildcard.hpp"

namespace demi {

// K2W_CAND 0 with K2W_ROUND 1: args as for k2_replay_wildcard (args.masks: ONE row for all proposals, or null; args.kept set;
// args.rec_out unused), cargs.c.key / first_ovf one word each, preset to ~0; the rest of cargs.c is unused.
__global__ __launch_bounds__(K2W_WAVES * 64) void k2_replay_wildcard_round(const K2WCandArgs cargs) {
  const K2WArgs& args = cargs.a;
  const K2WCand& cand = cargs.c;
#define K2W_CAND 0
#define K2W_ROUND 1
#include "k2_wildcard_body.hpp"
#undef K2W_ROUND
#undef K2W_CAND
}

struct K2WRoundRecord {
  uint32_t first_hit;      // lowest index with DEMI_V_VIOLATION and no capacity flag, 0xFFFFFFFF = none
  uint32_t first_ovf;      // lowest index with DEMI_V_PENDING_OVF or DEMI_V_QUEUE_OVF, 0xFFFFFFFF = none
  uint32_t executed_len;   // of first_hit (0 without one): the length demi_replay_wildcard_get_trace returns for it
  uint32_t pad[5];
  demi_verdict verdict;    // of first_hit (all zero without one)
};                         // 48 bytes; the winner's kept row follows it in the result buffer
#define K2W_ROUND_HEAD 48u

#ifndef DEMI_JIT_A     // (not part of a specialised module: it reads no table)
// one workgroup; result = K2WRoundRecord, then n_exp bytes.  n: proposals of the launch (an index that is not below n is "none").
__global__ __launch_bounds__(256) void k2w_round_pick(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ first_ovf,
                                                      const demi_verdict* __restrict__ v, const uint8_t* __restrict__ kept, uint32_t n,
                                                      uint32_t n_exp, unsigned char* __restrict__ result) {
  const unsigned long long k = key[0];
  const uint32_t hit = (uint32_t)(k >> 32) < n ? (uint32_t)(k >> 32) : 0xFFFFFFFFu, ovf = first_ovf[0] < n ? first_ovf[0] : 0xFFFFFFFFu;
  if (threadIdx.x == 0) {
    K2WRoundRecord r;
    r.first_hit = hit; r.first_ovf = ovf; r.executed_len = 0;
    for (int i = 0; i < 5; i++) r.pad[i] = 0;
    r.verdict.flags = 0; r.verdict.fingerprint = 0; r.verdict.hash = 0;
    if (hit != 0xFFFFFFFFu) { r.executed_len = (uint32_t)k; r.verdict = v[hit]; }
    *reinterpret_cast<K2WRoundRecord*>(result) = r;
  }
  if (hit == 0xFFFFFFFFu) return;
  const uint8_t* row = kept + (size_t)hit * n_exp;
  for (uint32_t i = threadIdx.x; i < n_exp; i += blockDim.x) result[K2W_ROUND_HEAD + i] = row[i];
}
#endif

}  // namespace demi
