// k_fuzz_reduce.hpp — a fuzz launch reduced on the device: what the host loop of demi_fuzz_campaign computes
// from a launch's flag words and the hit test's verdict row, as one fixed-size record plus the hit test's row, and a generated
// launch's largest n_ev / n_batches as two words.  Generic kernels of the library (no table is compiled into them), gfx950 wave64.
//
//   k_fuzz_meta_max     max n_ev, max n_batches of a generated launch -> two words (they size K1's LDS)
//   k_fuzz_first_hit    the lowest test index whose flag word has bit 0 -> red[FZR_FIRST]
//   k_fuzz_summarise    behind it in stream order: the tests below first_hit with bit 1 and without bit 0; the hit test's lowest
//                       violating execution and its lowest execution aborted on a capacity; the workgroup that finishes LAST (a
//                       ticket, nobody waits for anybody) writes the record and copies the hit test's events / areas behind it
//
// Reductions are per wave by __ballot and its lowest set lane (the lanes of a wave scan 64 consecutive items, so the first non-empty
// ballot of a wave's ascending walk holds its minimum), per workgroup through four LDS words, and ONE vector atomic per workgroup
// and address (65 536 same-address atomics cost more than the kernel they report for).  No kernel
// polls anything: k_fuzz_summarise reads what k_fuzz_first_hit left because it is behind it in the stream.
#pragma once

#include "demi_device.hpp"

namespace demi {

constexpr int FZR_THREADS = 256;             // four waves per workgroup
constexpr uint32_t FZR_MAX_BLOCKS = 256;     // a grid walks its range in passes of FZR_MAX_BLOCKS * FZR_THREADS items
constexpr uint32_t FZR_NONE = 0xFFFFFFFFu;
// the reduction words of one summary; the host sets FIRST / EXEC / ABORT to FZR_NONE and COUNT / TICKET to 0 in front of the kernels
enum : uint32_t { FZR_FIRST = 0, FZR_EXEC = 1, FZR_ABORT = 2, FZR_COUNT = 3, FZR_TICKET = 4, FZR_WORDS = 5 };
// the staging block: demi_fuzz_summary (10 words), then - 8-byte aligned - the hit test's events [stride], then its areas [stride]
constexpr uint32_t FZR_RECORD_WORDS = 10;
constexpr uint32_t FZR_ROW_OFFSET = 64;      // bytes

struct FuzzSummaryArgs {
  const uint32_t* flags;        // [n_tests]
  const uint32_t* verdicts;     // [n_tests][executions] demi_verdict as four words each; word 0 holds the DEMI_V_* bits
  const uint64_t* events;       // [n_tests][stride] or null
  const uint64_t* areas;        // [n_tests][stride] or null
  const uint32_t* n_ev;         // [n_tests] (null with events == null)
  uint32_t n_tests, executions, stride, pad;
  uint32_t* red;                // [FZR_WORDS]
  uint32_t* stage;              // the staging block
};

__device__ __forceinline__ uint32_t fzr_lowest(uint64_t mask) { return (uint32_t)__builtin_ctzll(mask); }

__global__ __launch_bounds__(FZR_THREADS) void k_fuzz_meta_max(const uint32_t* n_ev, const uint32_t* n_batches, uint32_t n, uint32_t* out) {
  __shared__ uint32_t s_ev[FZR_THREADS / 64], s_nb[FZR_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t ev = 0, nb = 0;
  for (uint32_t i = blockIdx.x * FZR_THREADS + threadIdx.x; i < n; i += gridDim.x * FZR_THREADS) {
    ev = max(ev, n_ev[i]);
    nb = max(nb, n_batches[i]);
  }
  for (uint32_t off = 32; off; off >>= 1) {          // (every lane of the wave is here: nothing returned early)
    ev = max(ev, (uint32_t)__shfl((int)ev, (int)(lane ^ off)));
    nb = max(nb, (uint32_t)__shfl((int)nb, (int)(lane ^ off)));
  }
  if (lane == 0) { s_ev[wave] = ev; s_nb[wave] = nb; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < FZR_THREADS / 64; w++) { ev = max(ev, s_ev[w]); nb = max(nb, s_nb[w]); }
    if (ev) atomicMax(&out[0], ev);
    if (nb) atomicMax(&out[1], nb);
  }
}

__global__ __launch_bounds__(FZR_THREADS) void k_fuzz_first_hit(const uint32_t* flags, uint32_t n_tests, uint32_t* red) {
  __shared__ uint32_t s_first[FZR_THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t first = FZR_NONE;
  // (the bound is the wave's: its 64 lanes take every ballot together)
  for (uint64_t base = (uint64_t)blockIdx.x * FZR_THREADS + wave * 64u; base < n_tests; base += (uint64_t)gridDim.x * FZR_THREADS) {
    const uint64_t i = base + lane;
    const uint64_t m = __ballot(i < n_tests && (flags[i < n_tests ? i : 0] & 1u));
    if (m) { first = (uint32_t)base + fzr_lowest(m); break; }
  }
  if (lane == 0) s_first[wave] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < FZR_THREADS / 64; w++) first = min(first, s_first[w]);
    if (first != FZR_NONE) atomicMin(&red[FZR_FIRST], first);
  }
}

__global__ __launch_bounds__(FZR_THREADS) void k_fuzz_summarise(const FuzzSummaryArgs a) {
  __shared__ uint32_t s_count[FZR_THREADS / 64], s_exec[FZR_THREADS / 64], s_abort[FZR_THREADS / 64];
  __shared__ uint32_t s_last, s_len;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t first = min(a.red[FZR_FIRST], a.n_tests);       // (k_fuzz_first_hit is done: stream order)
  const uint64_t pass = (uint64_t)gridDim.x * FZR_THREADS;
  // tests below first_hit with an aborted execution and none that violates
  uint32_t count = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * FZR_THREADS + wave * 64u; base < first; base += pass) {
    const uint64_t i = base + lane;
    count += (uint32_t)__popcll(__ballot(i < first && (a.flags[i < first ? i : 0] & 3u) == 2u));
  }
  // the hit test's row: its lowest violating execution, its lowest aborted one (an abort behind the violation this wave found
  // cannot be the row's lowest abort BEFORE the row's lowest violation, so the wave's walk ends there)
  uint32_t w_exec = FZR_NONE, w_abort = FZR_NONE;
  if (first < a.n_tests) {
    const uint32_t* row = a.verdicts + (size_t)first * a.executions * 4u;
    for (uint64_t base = (uint64_t)blockIdx.x * FZR_THREADS + wave * 64u; base < a.executions; base += pass) {
      const uint64_t k = base + lane;
      const uint32_t f = k < a.executions ? row[k * 4u] : 0u;
      const uint64_t m_abort = __ballot((f & (DEMI_V_PENDING_OVF | DEMI_V_QUEUE_OVF)) != 0);
      const uint64_t m_viol = __ballot((f & DEMI_V_VIOLATION) != 0);
      if (m_abort && w_abort == FZR_NONE) w_abort = (uint32_t)base + fzr_lowest(m_abort);
      if (m_viol) { w_exec = (uint32_t)base + fzr_lowest(m_viol); break; }
    }
  }
  if (lane == 0) { s_count[wave] = count; s_exec[wave] = w_exec; s_abort[wave] = w_abort; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < FZR_THREADS / 64; w++) { count += s_count[w]; w_exec = min(w_exec, s_exec[w]); w_abort = min(w_abort, s_abort[w]); }
    if (count) atomicAdd(&a.red[FZR_COUNT], count);
    if (w_exec != FZR_NONE) atomicMin(&a.red[FZR_EXEC], w_exec);
    if (w_abort != FZR_NONE) atomicMin(&a.red[FZR_ABORT], w_abort);
    __threadfence();                                   // this workgroup's three words before its ticket
    s_last = atomicAdd(&a.red[FZR_TICKET], 1u) == gridDim.x - 1u ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  // the final pass, by the workgroup that drew the last ticket: every other workgroup's words are in memory
  uint32_t* const rec = a.stage;
  if (threadIdx.x == 0) {
    __threadfence();
    const uint32_t exec = min(__hip_atomic_load(&a.red[FZR_EXEC], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), a.executions);
    const uint32_t abort = __hip_atomic_load(&a.red[FZR_ABORT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool hit = first < a.n_tests;
    rec[0] = first;
    rec[1] = __hip_atomic_load(&a.red[FZR_COUNT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rec[2] = hit ? exec : a.executions;
    rec[3] = (hit && abort < exec) ? 1u : 0u;
    rec[4] = (hit && a.n_ev) ? a.n_ev[first] : 0u;
    rec[5] = 0u;
    const bool have = hit && exec < a.executions;
    const uint32_t* v = a.verdicts + ((size_t)first * a.executions + exec) * 4u;
    for (uint32_t j = 0; j < 4; j++) rec[6 + j] = have ? v[j] : 0u;
    s_len = rec[4];
  }
  __syncthreads();
  if (first < a.n_tests && a.events) {
    const uint32_t len = min(s_len, a.stride);
    uint64_t* const out_ev = reinterpret_cast<uint64_t*>(reinterpret_cast<unsigned char*>(a.stage) + FZR_ROW_OFFSET);
    uint64_t* const out_ar = out_ev + a.stride;
    for (uint32_t j = threadIdx.x; j < len; j += FZR_THREADS) {
      out_ev[j] = a.events[(size_t)first * a.stride + j];
      if (a.areas) out_ar[j] = a.areas[(size_t)first * a.stride + j];
    }
  }
}

}  // namespace demi
