// k_fuzz.hpp — k_fuzz_generate: Fuzzer.generateFuzzTest (fuzzing/Fuzzer.scala:84-175), one generated test per lane.
//
// Test i runs under java.util.Random(seed_base + i) (or seeds[i]) and restates, per lane: the weight walk of getNextEventType
// (:44-57), the three RandomizedHashSets (alive nodes, unpartitioned pairs, partitioned pairs: schedulers/Util.scala:110-185,
// swap-remove), the retry on an empty (un)partition set - which draws a new double -, the rule against two WaitQuiescence in a
// row, the early return when a Kill finds nobody alive, the postfix and the final WaitQuiescence.  The application's
// MessageGenerator closure is the described generator of include/demi_gpu.h (demi_fuzz_send_gen); the order of its draws is
// written down there and in demi_amd/fuzzer.py SendGenerator, the host mirror this kernel is tested against byte for byte.
//
// Floating point: the host passes totalMass and the four cumulative thresholds as doubles.  nextDouble() is an exact integer
// (53 bits) times 2^-53 - exact -, so the device's only rounding operation is ONE multiply, by totalMass; everything after it
// is comparisons.  IEEE-754 fixes that product, so the walk takes the same branch as the JVM's and the mirror's.  The multiply
// is kept from being contracted with anything (fp contract off).
//
// The three sets are indexed by a per-lane random slot: as private arrays they would live in scratch memory.  They are LDS
// byte columns [slot][lane] instead (256 slots x 64 lanes = 16 KB per wave).  Bytes, not dwords: lanes 4k .. 4k + 3 share a dword and
// lanes at different slots may meet in a bank, so the layout is chosen for its size, not for conflict-free access - the generator
// is 0.19 ms of a launch beside K1's milliseconds.
//
// k_fuzz_generate_fields (below) is the same generator with demi_fuzz_field_gen: up to DEMI_MAX_PAYLOADS described
// fields per alternative, drawn in the order 0, 1, .. n_fields - 1, and beside every event its 48-bit payload area - the fields packed
// as DEMI_PAYLOAD_OF reads them - for the K1 front end that takes a test's areas (K1TestsArgs.test_areas).  A second kernel, not a
// template over both: k_fuzz_generate keeps the instructions it was measured with.  The field width is a kernel argument; neither
// kernel is specialised for a table.
#pragma once

#include "demi_device.hpp"

namespace demi {

constexpr uint32_t FZ_MAX_NODES = DEMI_MAX_ACTORS_BIG;                        // 16 alive actors at most
constexpr uint32_t FZ_MAX_PAIRS = FZ_MAX_NODES * (FZ_MAX_NODES - 1) / 2;      // 120 unordered pairs
constexpr uint32_t FZ_SLOTS = FZ_MAX_NODES + 2 * FZ_MAX_PAIRS;                // alive, unpartitioned, partitioned
constexpr int FZ_THREADS = 64;                                                // one wave per workgroup

struct FuzzArgs {
  const uint32_t* magic;        // [257] nextInt multiply-high magics (the loaded model's divmagic)
  const uint64_t* prefix;       // demi_ext_event[n_prefix] as 8-byte words
  const uint64_t* postfix;      // [n_postfix]
  uint32_t n_prefix, n_postfix, num_events, stride, n_tests, field_mask, n_nodes, pad;
  uint8_t nodes[FZ_MAX_NODES];  // the actors the prefix Start()s, in its order
  uint64_t seed_base;
  const uint64_t* seeds;        // optional
  double total, cum[4];         // totalMass; kill, + send, + partition, + unpartition
  demi_fuzz_send_gen gen;
  uint64_t* out_events;         // [n_tests][stride]
  uint32_t* out_n_ev;           // [n_tests]
  uint32_t* out_n_batches;      // [n_tests] WaitQuiescence events + 1
  uint32_t* out_started;        // [n_tests] the actors the test Start()s (the prefix's and the postfix's)
};

__device__ __forceinline__ uint32_t jr_next_bits(uint64_t& s, uint32_t bits) {
  s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
  return (uint32_t)(s >> (48 - bits));
}
// java.util.Random.nextDouble: ((next(26) << 27) + next(27)) * 0x1p-53 - the conversion and the product are exact
__device__ __forceinline__ double jr_next_double(uint64_t& s) {
  const uint64_t hi = jr_next_bits(s, 26);
  const uint64_t lo = jr_next_bits(s, 27);
  return (double)((hi << 27) + lo) * 0x1p-53;
}

__device__ __forceinline__ uint64_t fz_event(uint32_t kind, uint32_t a, uint32_t b, uint32_t msg_type, uint32_t p0, uint32_t p1) {
  // demi_ext_event: kind, a, b, msg_type, p0, p1, p0_hi, p1_hi
  return (uint64_t)kind | ((uint64_t)a << 8) | ((uint64_t)b << 16) | ((uint64_t)msg_type << 24) | ((uint64_t)(p0 & 0xFFu) << 32) |
         ((uint64_t)(p1 & 0xFFu) << 40) | ((uint64_t)((p0 >> 8) & 0xFFu) << 48) | ((uint64_t)((p1 >> 8) & 0xFFu) << 56);
}

__global__ __launch_bounds__(FZ_THREADS) void k_fuzz_generate(const FuzzArgs a) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  __shared__ uint8_t s_sets[FZ_SLOTS * FZ_THREADS];
  const uint32_t lane = threadIdx.x;
  const uint32_t test = blockIdx.x * FZ_THREADS + lane;
  if (test >= a.n_tests) return;        // (no cross-lane operation below: a partial last wave just has fewer lanes)
  uint8_t* const alive = s_sets + lane;                                        // element k at [k * FZ_THREADS]
  uint8_t* const unparted = s_sets + FZ_MAX_NODES * FZ_THREADS + lane;          // a pair is one byte: a << 4 | b
  uint8_t* const parted = unparted + FZ_MAX_PAIRS * FZ_THREADS;
  uint64_t rng = jr_seed(a.seeds ? a.seeds[test] : a.seed_base + test);
  uint32_t n_alive = a.n_nodes, n_unparted = 0, n_parted = 0;
  for (uint32_t i = 0; i < a.n_nodes; i++) alive[i * FZ_THREADS] = a.nodes[i];
  for (uint32_t i = 0; i < a.n_nodes; i++)
    for (uint32_t j = i + 1; j < a.n_nodes; j++) unparted[(n_unparted++) * FZ_THREADS] = (uint8_t)((a.nodes[i] << 4) | a.nodes[j]);

  uint64_t* const out = a.out_events + (size_t)test * a.stride;
  uint32_t n = 0, n_wq = 0, started = 0;
  auto emit = [&](uint64_t ev) {
    const uint32_t kind = (uint32_t)ev & 0xFFu;
    if (kind == DEMI_EV_WAIT_QUIESCENCE) n_wq++;
    if (kind == DEMI_EV_START) started |= 1u << ((uint32_t)(ev >> 8) & 0xFFu);
    out[n++] = ev;                      // n < stride: prefix + at most num_events + postfix + 1
  };
  for (uint32_t i = 0; i < a.n_prefix; i++) emit(a.prefix[i]);
  bool just_wq = a.n_prefix != 0 && ((uint32_t)a.prefix[a.n_prefix - 1] & 0xFFu) == DEMI_EV_WAIT_QUIESCENCE;
  uint32_t n_sends = 0;
  bool ended = false;                   // a Kill found nobody alive: generateFuzzTest returns what it has
  for (uint32_t k = 0; k < a.num_events && !ended; k++) {
    for (;;) {                          // one generated event; `continue` = draw again
      const double scaled = jr_next_double(rng) * a.total;
      if (scaled < a.cum[0]) {                                  // Kill
        if (n_alive == 0) { ended = true; break; }
        const uint32_t i = jr_next_int(rng, n_alive, a.magic);
        const uint32_t v = alive[i * FZ_THREADS];
        n_alive--;
        alive[i * FZ_THREADS] = alive[n_alive * FZ_THREADS];
        emit(fz_event(DEMI_EV_KILL, v, 0, 0, 0, 0));
        just_wq = false;
        break;
      }
      if (scaled < a.cum[1]) {                                  // Send: the described generator, in its documented draw order
        n_sends++;
        const uint32_t alt = a.gen.n_alts > 1 ? jr_next_int(rng, a.gen.n_alts, a.magic) : 0u;
        // (selected by value: an alternative indexed per lane would put the argument struct into scratch memory)
        demi_fuzz_send_alt g = a.gen.alts[0];
        for (uint32_t q = 1; q < DEMI_FUZZ_MAX_ALTS; q++) if (q == alt) g = a.gen.alts[q];
        uint32_t target = g.target_actor;
        if (g.target_kind == DEMI_FUZZ_TARGET_RANDOM_ALIVE)
          target = n_alive ? alive[jr_next_int(rng, n_alive, a.magic) * FZ_THREADS] : 0u;
        uint32_t p0 = g.p0_arg, p1 = g.p1_arg;
        if (g.p0_kind == DEMI_FUZZ_FIELD_COUNTER) p0 = n_sends & a.field_mask;
        else if (g.p0_kind == DEMI_FUZZ_FIELD_RANDOM) p0 = jr_next_int(rng, g.p0_arg, a.magic);
        if (g.p1_kind == DEMI_FUZZ_FIELD_COUNTER) p1 = n_sends & a.field_mask;
        else if (g.p1_kind == DEMI_FUZZ_FIELD_RANDOM) p1 = jr_next_int(rng, g.p1_arg, a.magic);
        emit(fz_event(DEMI_EV_SEND, target, 0, g.msg_type, p0, p1));
        just_wq = false;
        break;
      }
      if (scaled < a.cum[2]) {                                  // Partition
        if (n_unparted == 0) continue;
        const uint32_t i = jr_next_int(rng, n_unparted, a.magic);
        const uint32_t pr = unparted[i * FZ_THREADS];
        n_unparted--;
        unparted[i * FZ_THREADS] = unparted[n_unparted * FZ_THREADS];
        parted[(n_parted++) * FZ_THREADS] = (uint8_t)pr;
        emit(fz_event(DEMI_EV_PARTITION, pr >> 4, pr & 15u, 0, 0, 0));
        just_wq = false;
        break;
      }
      if (scaled < a.cum[3]) {                                  // UnPartition
        if (n_parted == 0) continue;
        const uint32_t i = jr_next_int(rng, n_parted, a.magic);
        const uint32_t pr = parted[i * FZ_THREADS];
        n_parted--;
        parted[i * FZ_THREADS] = parted[n_parted * FZ_THREADS];
        unparted[(n_unparted++) * FZ_THREADS] = (uint8_t)pr;
        emit(fz_event(DEMI_EV_UNPARTITION, pr >> 4, pr & 15u, 0, 0, 0));
        just_wq = false;
        break;
      }
      if (just_wq) continue;                                    // no two WaitQuiescence in a row: generate again
      emit(fz_event(DEMI_EV_WAIT_QUIESCENCE, 0, 0, 0, 0, 0));
      just_wq = true;
      break;
    }
  }
  if (!ended) {
    for (uint32_t i = 0; i < a.n_postfix; i++) emit(a.postfix[i]);
    if (n != 0 && ((uint32_t)out[n - 1] & 0xFFu) != DEMI_EV_WAIT_QUIESCENCE) emit(fz_event(DEMI_EV_WAIT_QUIESCENCE, 0, 0, 0, 0, 0));
  }
  a.out_n_ev[test] = n;
  a.out_n_batches[test] = n_wq + 1;
  a.out_started[test] = started;
  for (uint32_t i = n; i < a.stride; i++) out[i] = 0;           // the row's tail: defined bytes
}

// k_fuzz_generate_fields: FuzzArgs with the wider generator, the areas' row and the layout of an area
struct FuzzFieldArgs {
  const uint32_t* magic;
  const uint64_t* prefix;
  const uint64_t* postfix;
  uint32_t n_prefix, n_postfix, num_events, stride, n_tests, field_mask, n_nodes, pad;
  uint8_t nodes[FZ_MAX_NODES];
  uint64_t seed_base;
  const uint64_t* seeds;
  double total, cum[4];
  demi_fuzz_field_gen gen;
  uint64_t* out_events;
  uint32_t* out_n_ev;
  uint32_t* out_n_batches;
  uint32_t* out_started;
  uint64_t* out_areas;          // [n_tests][stride], zero off the Sends and behind a test's length
  uint32_t area_bits;           // the width of a field in the area (= the width field_mask is of); 0 = a table with two fields: every area is 0
  uint32_t pad2;
};

// k_fuzz_generate with up to DEMI_MAX_PAYLOADS described fields per Send and the payload areas beside the events (the comments of
// k_fuzz_generate apply line by line; what differs is marked).  A template, so that only the translation unit that launches it
// carries it: one that includes this header for the two-field kernel alone holds that kernel alone.
template <int UNUSED = 0>
__global__ __launch_bounds__(FZ_THREADS) void k_fuzz_generate_fields(const FuzzFieldArgs a) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  __shared__ uint8_t s_sets[FZ_SLOTS * FZ_THREADS];
  const uint32_t lane = threadIdx.x;
  const uint32_t test = blockIdx.x * FZ_THREADS + lane;
  if (test >= a.n_tests) return;        // (no cross-lane operation below: a partial last wave just has fewer lanes)
  uint8_t* const alive = s_sets + lane;                                        // element k at [k * FZ_THREADS]
  uint8_t* const unparted = s_sets + FZ_MAX_NODES * FZ_THREADS + lane;          // a pair is one byte: a << 4 | b
  uint8_t* const parted = unparted + FZ_MAX_PAIRS * FZ_THREADS;
  uint64_t rng = jr_seed(a.seeds ? a.seeds[test] : a.seed_base + test);
  uint32_t n_alive = a.n_nodes, n_unparted = 0, n_parted = 0;
  for (uint32_t i = 0; i < a.n_nodes; i++) alive[i * FZ_THREADS] = a.nodes[i];
  for (uint32_t i = 0; i < a.n_nodes; i++)
    for (uint32_t j = i + 1; j < a.n_nodes; j++) unparted[(n_unparted++) * FZ_THREADS] = (uint8_t)((a.nodes[i] << 4) | a.nodes[j]);

  uint64_t* const out = a.out_events + (size_t)test * a.stride;
  uint64_t* const out_area = a.out_areas + (size_t)test * a.stride;      // (fields: the row of areas, written with every event)
  uint32_t n = 0, n_wq = 0, started = 0;
  auto emit = [&](uint64_t ev, uint64_t area = 0) {
    const uint32_t kind = (uint32_t)ev & 0xFFu;
    if (kind == DEMI_EV_WAIT_QUIESCENCE) n_wq++;
    if (kind == DEMI_EV_START) started |= 1u << ((uint32_t)(ev >> 8) & 0xFFu);
    out_area[n] = area;
    out[n++] = ev;                      // n < stride: prefix + at most num_events + postfix + 1
  };
  // a Send of the prefix / postfix: the area a load without staged areas makes of its P0 / P1 (demi_trace_load)
  auto emit_fixed = [&](uint64_t ev) {
    uint64_t area = 0;
    if (((uint32_t)ev & 0xFFu) == DEMI_EV_SEND && a.area_bits != 0) {
      const uint32_t p0 = ((uint32_t)(ev >> 32) & 0xFFu) | (((uint32_t)(ev >> 48) & 0xFFu) << 8);
      const uint32_t p1 = ((uint32_t)(ev >> 40) & 0xFFu) | (((uint32_t)(ev >> 56) & 0xFFu) << 8);
      area = (uint64_t)(p0 & a.field_mask) | ((uint64_t)(p1 & a.field_mask) << a.area_bits);
    }
    emit(ev, area);
  };
  for (uint32_t i = 0; i < a.n_prefix; i++) emit_fixed(a.prefix[i]);
  bool just_wq = a.n_prefix != 0 && ((uint32_t)a.prefix[a.n_prefix - 1] & 0xFFu) == DEMI_EV_WAIT_QUIESCENCE;
  uint32_t n_sends = 0;
  bool ended = false;                   // a Kill found nobody alive: generateFuzzTest returns what it has
  for (uint32_t k = 0; k < a.num_events && !ended; k++) {
    for (;;) {                          // one generated event; `continue` = draw again
      const double scaled = jr_next_double(rng) * a.total;
      if (scaled < a.cum[0]) {                                  // Kill
        if (n_alive == 0) { ended = true; break; }
        const uint32_t i = jr_next_int(rng, n_alive, a.magic);
        const uint32_t v = alive[i * FZ_THREADS];
        n_alive--;
        alive[i * FZ_THREADS] = alive[n_alive * FZ_THREADS];
        emit(fz_event(DEMI_EV_KILL, v, 0, 0, 0, 0));
        just_wq = false;
        break;
      }
      if (scaled < a.cum[1]) {                                  // Send: the described generator, in its documented draw order
        n_sends++;
        const uint32_t alt = a.gen.n_alts > 1 ? jr_next_int(rng, a.gen.n_alts, a.magic) : 0u;
        // (selected by value: an alternative indexed per lane would put the argument struct into scratch memory)
        demi_fuzz_field_alt g = a.gen.alts[0];
        for (uint32_t q = 1; q < DEMI_FUZZ_MAX_ALTS; q++) if (q == alt) g = a.gen.alts[q];
        uint32_t target = g.target_actor;
        if (g.target_kind == DEMI_FUZZ_TARGET_RANDOM_ALIVE)
          target = n_alive ? alive[jr_next_int(rng, n_alive, a.magic) * FZ_THREADS] : 0u;
        // fields 0 .. n_fields - 1 in that order, the others 0; unrolled: kind[k] / arg[k] are then members, not indexed
        uint32_t p0 = 0, p1 = 0;
        uint64_t area = 0;
#pragma unroll
        for (uint32_t f = 0; f < DEMI_MAX_PAYLOADS; f++) {
          if (f >= g.n_fields) continue;
          uint32_t v = g.arg[f];
          if (g.kind[f] == DEMI_FUZZ_FIELD_COUNTER) v = n_sends & a.field_mask;
          else if (g.kind[f] == DEMI_FUZZ_FIELD_RANDOM) v = jr_next_int(rng, g.arg[f], a.magic);
          if (f == 0) p0 = v;
          if (f == 1) p1 = v;
          area |= (uint64_t)v << (f * a.area_bits);      // (v < 2^area_bits: CONST and RANDOM are validated, COUNTER is masked)
        }
        if (a.area_bits == 0) area = 0;                  // (a table without DEMI_MODEL_PAYLOADS: no areas)
        emit(fz_event(DEMI_EV_SEND, target, 0, g.msg_type, p0, p1), area);
        just_wq = false;
        break;
      }
      if (scaled < a.cum[2]) {                                  // Partition
        if (n_unparted == 0) continue;
        const uint32_t i = jr_next_int(rng, n_unparted, a.magic);
        const uint32_t pr = unparted[i * FZ_THREADS];
        n_unparted--;
        unparted[i * FZ_THREADS] = unparted[n_unparted * FZ_THREADS];
        parted[(n_parted++) * FZ_THREADS] = (uint8_t)pr;
        emit(fz_event(DEMI_EV_PARTITION, pr >> 4, pr & 15u, 0, 0, 0));
        just_wq = false;
        break;
      }
      if (scaled < a.cum[3]) {                                  // UnPartition
        if (n_parted == 0) continue;
        const uint32_t i = jr_next_int(rng, n_parted, a.magic);
        const uint32_t pr = parted[i * FZ_THREADS];
        n_parted--;
        parted[i * FZ_THREADS] = parted[n_parted * FZ_THREADS];
        unparted[(n_unparted++) * FZ_THREADS] = (uint8_t)pr;
        emit(fz_event(DEMI_EV_UNPARTITION, pr >> 4, pr & 15u, 0, 0, 0));
        just_wq = false;
        break;
      }
      if (just_wq) continue;                                    // no two WaitQuiescence in a row: generate again
      emit(fz_event(DEMI_EV_WAIT_QUIESCENCE, 0, 0, 0, 0, 0));
      just_wq = true;
      break;
    }
  }
  if (!ended) {
    for (uint32_t i = 0; i < a.n_postfix; i++) emit_fixed(a.postfix[i]);
    if (n != 0 && ((uint32_t)out[n - 1] & 0xFFu) != DEMI_EV_WAIT_QUIESCENCE) emit(fz_event(DEMI_EV_WAIT_QUIESCENCE, 0, 0, 0, 0, 0));
  }
  a.out_n_ev[test] = n;
  a.out_n_batches[test] = n_wq + 1;
  a.out_started[test] = started;
  for (uint32_t i = n; i < a.stride; i++) out[i] = 0;           // the row's tail: defined bytes
  for (uint32_t i = n; i < a.stride; i++) out_area[i] = 0;
}

}  // namespace demi
