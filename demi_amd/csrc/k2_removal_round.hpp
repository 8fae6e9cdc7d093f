// k2_removal_round.hpp — what follows the removal replay (k2_replay.hpp with K2Args.skip and a kept plane) in one round of
// STSSchedMinimizer.minimize (minification/internal_minimization/ScheduleCheckers.scala:35-107).
//
// A removal strategy proposes its candidates one after another, each assuming the one before it failed, and the sequential loop
// adopts the FIRST that still triggers the violation.  After the replay of a round's n candidates the host therefore needs one
// number (the lowest reproducing index), one more to know whether that number is an answer (the lowest index aborted on a
// capacity: an aborted replay before the first hit is no verdict), and the winner's verdict and executed-trace marks - not n
// verdicts and a second replay of the winner.  Two kernels behind the replay on the same stream:
//
//   k2_removal_select  one candidate per lane, grid-stride: ballot the reproducing and the aborted lanes, lowest set bit per
//                      wave and pass, the wave's minimum kept in a register; ONE atomicMin per wave and word at the end.  A
//                      minimum does not depend on the order of the atomics, so the answer is the same whichever wave arrives first.
//   k2_removal_pick    reads the two words after the select kernel has finished (a kernel boundary: no flag, no fence), writes
//                      the record and copies the winner's n_exp-byte row of the kept plane behind it.
//
// The host reads K2_ROUND_HEAD + n_exp bytes.  Neither kernel reads the transition table: they are not part of a specialised module.
#pragma once

#include "demi_device.hpp"

namespace demi {

struct K2RoundRecord {
  uint32_t first_hit;      // lowest index with DEMI_V_VIOLATION and no capacity flag, 0xFFFFFFFF = none
  uint32_t first_ovf;      // lowest index with DEMI_V_PENDING_OVF or DEMI_V_QUEUE_OVF, 0xFFFFFFFF = none
  uint32_t pad[2];
  demi_verdict verdict;    // of first_hit (all zero without one)
};                         // 32 bytes; the winner's kept row follows it in the result buffer
#define K2_ROUND_HEAD 32u

// best[0] / best[1] start at 0xFFFFFFFF
__global__ __launch_bounds__(256) void k2_removal_select(const demi_verdict* __restrict__ v, uint32_t n, uint32_t* __restrict__ best) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t stride = gridDim.x * blockDim.x;
  uint32_t hit_min = 0xFFFFFFFFu, ovf_min = 0xFFFFFFFFu;         // wave-uniform
  // `base` is the index of the wave's lane 0: the whole wave makes the same number of passes, so the ballots meet
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint32_t i = base + lane;
    const uint32_t f = i < n ? v[i].flags : 0u;
    const bool ovf = (f & (DEMI_V_PENDING_OVF | DEMI_V_QUEUE_OVF)) != 0;
    const bool hit = (f & DEMI_V_VIOLATION) != 0 && !ovf;
    const uint64_t mh = __ballot(hit), mo = __ballot(ovf);
    // (passes ascend: the first pass with a set bit holds the wave's minimum)
    if (mh && hit_min == 0xFFFFFFFFu) hit_min = base + (uint32_t)__builtin_ctzll(mh);
    if (mo && ovf_min == 0xFFFFFFFFu) ovf_min = base + (uint32_t)__builtin_ctzll(mo);
  }
  if (lane == 0) {
    if (hit_min != 0xFFFFFFFFu) atomicMin(&best[0], hit_min);
    if (ovf_min != 0xFFFFFFFFu) atomicMin(&best[1], ovf_min);
  }
}

// one workgroup; result = K2RoundRecord, then n_exp bytes.  n: candidates of the launch (a word that is not below n is "none").
__global__ __launch_bounds__(256) void k2_removal_pick(const uint32_t* __restrict__ best, const demi_verdict* __restrict__ v,
                                                       const uint8_t* __restrict__ kept, uint32_t n, uint32_t n_exp,
                                                       unsigned char* __restrict__ result) {
  const uint32_t hit = best[0] < n ? best[0] : 0xFFFFFFFFu, ovf = best[1] < n ? best[1] : 0xFFFFFFFFu;
  if (threadIdx.x == 0) {
    K2RoundRecord r;
    r.first_hit = hit; r.first_ovf = ovf; r.pad[0] = r.pad[1] = 0;
    r.verdict.flags = 0; r.verdict.fingerprint = 0; r.verdict.hash = 0;
    if (hit != 0xFFFFFFFFu) r.verdict = v[hit];
    *reinterpret_cast<K2RoundRecord*>(result) = r;
  }
  if (hit == 0xFFFFFFFFu) return;
  const uint8_t* row = kept + (size_t)hit * n_exp;
  for (uint32_t k = threadIdx.x; k < n_exp; k += blockDim.x) result[K2_ROUND_HEAD + k] = row[k];
}

}  // namespace demi
