// k3_wildcard.hpp — K3W: one DPORwHeuristics interleaving per wavefront lane whose next trace may hold WILDCARDS.
//
// The oracle of WildcardMinimizer with TestScheduler.DPORwHeuristics (WildcardMinimizer.testWithDpor,
// minification/wildcard_minimization/WildcardMinimizer.scala:67-114): the next trace of an interleaving is a proposal's
// UniqueMsgEvents, most of them MsgEvent(snd, rcv, WildCardMatch(selector)), and a wildcard that could have taken another
// pending message reports it through its backtrackSetter (DPORwHeuristics.scala:474-514;
// AmbiguityResolutionStrategies.scala:44-107).  Restated here: k3_dpor's scheduling step (k3_dpor.hpp: the same pending set
// with its side words and key plane, the same node keys, trace entries, verdict and hash) with
//   (a) prefix entries of kind 3 (a wildcard) and 4 (an exact delivery named by its message word, not by its node:
//       equivalentTo's first case, :433-438, what a proposal holds for the deliveries of external messages),
//   (b) the match of a wildcard against ALL pending messages of (snd, rcv) in send order - not the heads of the fingerprint
//       groups, as STSScheduler has it (k2_wildcard_body.hpp) - with one record per alternative,
//   (c) stopAfterNextTrace (:588-590, 612-613) and the positions getNextMatchingMessage reports as absent (:542-555),
// and WITHOUT what skipBacktrackComputation switches off or this oracle never uses: no racing pairs, no next traces built from
// an arena, no checkpoints.  A kernel of its own rather than a flag of k3_dpor: that kernel's exact match is two unrolled
// passes over the LDS-resident slots and its fresh-start is the checkpoint code, neither of which this one has, and every
// instantiation of k3_dpor stays the instruction stream it was.  All results leave through vector stores in plain C++.
#pragma once

#include "k3_dpor.hpp"

namespace demi {

// what a kind-3 prefix entry carries in its key: the 32-bit type set, the demi_wildcard_policy, the demi_wildcard_backtrack
__host__ __device__ inline uint64_t k3w_selector_key(uint32_t types, uint32_t policy, uint32_t mode) {
  return (uint64_t)types | ((uint64_t)(policy & 0xFFu) << 32) | ((uint64_t)(mode & 0xFFu) << 40);
}

struct K3WArgs {
  const DevModel* model;
  const uint64_t* ext;               // external events (Start / Send / WaitQuiescence)
  uint32_t n_ext;
  const demi_dpor_trace_entry* prefixes;  // [n][stride]: kinds 0 / 1 / 2 as k3_dpor reads them, 3 and 4 as above
  const uint32_t* prefix_len;        // [n]
  uint32_t stride;
  uint64_t n;
  uint32_t depth_bound, max_messages, looking_for_valid, looking_for, p_max, prioritize;
  uint32_t stop_after_next_trace;    // stopAfterNextTrace
  uint32_t max_alts;                 // alternative records an interleaving may write
  uint32_t lanes_per_wave;
  demi_verdict* out;
  demi_dpor_trace_entry* traces;     // [n][DEMI_DPOR_MAX_TRACE]
  uint32_t* trace_len;               // [n]
  uint64_t* ignored;                 // [n][4]: bit p = the head at position p of the next trace was absent (ignoreAbsentCallback)
  uint64_t* wild;                    // [n][4]: bit i = trace entry i was picked by a wildcard (setExplored, :504-508)
  demi_dpor_wild_alt* alts;          // [n][max_alts]
  uint32_t* n_alts;                  // [n]
  unsigned long long* work_counter;
  uint32_t* spill;
};

__global__ __launch_bounds__(K3_WAVES * 64) void k3_dpor_wild(const K3WArgs args) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Tables t;
  unsigned char* wave_base = tables_load(t, smem, args.model, args.ext, args.n_ext, (1u << args.model->n_actors) - 1);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const LaneMem mem = lane_mem_carve(wave_base + (size_t)wave * lane_mem_wave_bytes(t.A, true), t.A, true, lane,
                                     args.spill, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
                                     (size_t)gridDim.x * blockDim.x);
  uint64_t* const st = mem.st;
  // (the key plane of k3_dpor.hpp: the node key of every LDS-resident pending message beside its word and side word)
  uint64_t* const kp = reinterpret_cast<uint64_t*>(wave_base + (size_t)(blockDim.x >> 6) * lane_mem_wave_bytes(t.A, true) +
                                                   (size_t)wave * k3_key_wave_bytes(PEND_HOT)) + lane;      // [slot * 64]
  const uint32_t A = t.A, NE = t.E, PMAX = args.p_max;
  const uint32_t max_messages = args.max_messages ? args.max_messages : 0x7FFFFFFFu;

  bool active = false, fresh = false;
  uint64_t sched = 0, hash = 0, app_rng = 0;
  demi_dpor_trace_entry* tr = nullptr;
  const demi_dpor_trace_entry* pf = nullptr;
  uint32_t pfx = 0, pfx_len = 0;
  uint32_t n_pend = 0, next_seq = 0, parent = 0, parent_depth = 0, cur_root = 0, qperiod = 0, next_qperiod = 0;
  uint64_t parent_key = DPOR_ROOT_KEY;
  uint32_t marker_ext = 0, qmarker_ext = 0, isolated = 0, flags = 0, count = 0, deliveries = 0;
  tmask_t rep = 0;
  uint32_t blocked = 0;
  uint32_t n_trace = 0, ext_idx = 0, n_alt = 0;
  bool awaiting = false, marker_pending = false;
  uint64_t ig0 = 0, ig1 = 0, ig2 = 0, ig3 = 0, wc0 = 0, wc1 = 0, wc2 = 0, wc3 = 0;     // the two 256-bit masks, selected by value
  uint64_t b_next = 0, b_end = 0;
  bool exhausted = false;

#define K3W_ABORT (DEMI_OVF_ANY | DEMI_V_TRACE_OVF | DEMI_V_SELFMSG | DEMI_V_ALTS_OVF)
#define K3W_TIMER_BIT(RCV, TYPE) ((tmask_t)1 << ((RCV) * DEMI_MAX_TIMER_TYPES + (t.meta[(TYPE)] >> 8)))
#define K3W_SET_BIT(M, I)                                                                            \
  do {                                                                                               \
    const uint32_t q_ = ((I) >> 6) & 3u;                                                             \
    const uint64_t b_ = 1ull << ((I) & 63u);                                                         \
    M##0 |= q_ == 0 ? b_ : 0ull; M##1 |= q_ == 1 ? b_ : 0ull; M##2 |= q_ == 2 ? b_ : 0ull; M##3 |= q_ == 3 ? b_ : 0ull; \
  } while (0)

  // event_produced + getMessage (:773-847), as k3_dpor
  auto produce = [&](word_t word) {
    if (args.depth_bound && parent_depth + 1 >= args.depth_bound) return;
    if (flags & DEMI_OVF_ANY) return;
    if (n_pend >= PMAX) { flags |= DEMI_V_PENDING_OVF; return; }
    const uint32_t side = parent | (qperiod << 8) | (next_seq << 16);
    pend_store(mem, n_pend, word);
    aux_store(mem, n_pend, side);
    if (n_pend < PEND_HOT) kp[n_pend * 64] = (parent_key ^ (uint64_t)word) * DPOR_PRIME;
    next_seq++;
    n_pend++;
  };
  auto key_at = [&](uint32_t k, word_t cw, uint32_t aux) -> uint64_t {
    return k < PEND_HOT ? kp[k * 64] : (tr[aux & 0xFF].key ^ (uint64_t)cw) * DPOR_PRIME;
  };
  auto pend_remove_at = [&](uint32_t k) {
    const uint32_t last = n_pend - 1;
    const word_t lw = pend_load(mem, last);
    const uint32_t la = aux_load(mem, last);
    if (k < PEND_HOT && k != last) kp[k * 64] = key_at(last, lw, la);
    pend_store(mem, k, lw);
    aux_store(mem, k, la);
    n_pend--;
  };
  uint32_t pushed_depth = 0;
  auto trace_push = [&](uint64_t key, word_t word, uint32_t par, uint32_t qp, uint32_t kind) -> int {
    if (n_trace >= DEMI_DPOR_MAX_TRACE) { flags |= DEMI_V_TRACE_OVF; return -1; }
    demi_dpor_trace_entry e;
    e.key = key; e.word = (uint32_t)word; e.parent = (uint8_t)par; e.qperiod = (uint8_t)qp;
    e.depth = (uint8_t)(n_trace == 0 ? 0 : tr[par].depth + 1);
    e.kind = (uint8_t)kind;
    tr[n_trace] = e;
    pushed_depth = e.depth;
    return (int)n_trace++;
  };
  // runExternal (:684-721)
  auto run_external = [&]() {
    bool await = false;
    while (ext_idx < NE && !await) {
      const uint64_t ev = t.trace[ext_idx];
      const uint32_t kind = (uint32_t)ev & 0xFF, a = (uint32_t)(ev >> 8) & 0xFF;
      if (kind == DEMI_EV_START) isolated &= ~(1u << a);
#ifdef DEMI_JIT_NPAY
      else if (kind == DEMI_EV_SEND)
        produce(msg_word_area((uint32_t)(ev >> 24) & 0xFF, DL, a, args.ext[EXT_AREA_OFFSET + ext_idx] & 0xFFFFFFFFFFFFull));
#else
      else if (kind == DEMI_EV_SEND)
        produce(msg_word((uint32_t)(ev >> 24) & 0xFF, DL, a,
                         ((uint32_t)(ev >> 32) & 0xFF) | (WIDE_TU ? ((uint32_t)(ev >> 48) & 0xFF) << 8 : 0u),
                         ((uint32_t)(ev >> 40) & 0xFF) | (WIDE_TU ? ((uint32_t)(ev >> 56) & 0xFF) << 8 : 0u)));
#endif
      else if (kind == DEMI_EV_WAIT_QUIESCENCE) { marker_pending = true; marker_ext = ext_idx; await = true; }
      ext_idx++;
    }
  };

  for (;;) {
    {   // idle lanes take the next interleavings of the launch (as k3_dpor)
      const uint64_t idle = __ballot(!active && lane < args.lanes_per_wave);
      if (idle != 0 && !exhausted) {
        const uint32_t want = (uint32_t)__popcll(idle);
        const uint64_t have = b_end - b_next;
        uint64_t got = 0;
        if (have < want) {
          if (lane == 0) got = atomicAdd(args.work_counter, (unsigned long long)args.lanes_per_wave);
          got = __shfl(got, 0);
        }
        if (!active && lane < args.lanes_per_wave) {
          const uint32_t rank = (uint32_t)__popcll(idle & ((1ULL << lane) - 1));
          const uint64_t my = (rank < have) ? (b_next + rank) : (got + (rank - have));
          if (my < args.n) { sched = my; active = true; fresh = true; }
        }
        if (have < want) { b_next = got + (want - have); b_end = got + args.lanes_per_wave; }
        else b_next += want;
        if (b_next >= args.n) exhausted = true;
      }
      if (__ballot(active) == 0) break;
    }

    word_t w = 0;
    bool deliver = false, finish = false;
    if (active) {
      if (fresh) {
        fresh = false;
        tr = args.traces + sched * DEMI_DPOR_MAX_TRACE;
        pf = args.prefixes + sched * (uint64_t)args.stride;
        pfx_len = args.prefix_len[sched];
        pfx = 0;
        hash = 0xCBF29CE484222325ULL;
        app_rng = jr_seed(0);
        isolated = (1u << A) - 1;
        for (uint32_t a = 0; a < A * ST_WORDS; a++) st[a * 64] = t.init[a];
        n_pend = 0; next_seq = 0; qperiod = 0; next_qperiod = 0; rep = 0; flags = 0; count = 0; deliveries = 0; blocked = 0;
        n_trace = 0; ext_idx = 0; n_alt = 0; awaiting = false; marker_pending = false;
        ig0 = ig1 = ig2 = ig3 = 0; wc0 = wc1 = wc2 = wc3 = 0;      // resetCallback (:337)
        trace_push(DPOR_ROOT_KEY, 0, 0, 0, 0);
        parent = 0; parent_depth = 0; cur_root = 0; parent_key = DPOR_ROOT_KEY;
        run_external();
      }
      if (flags & K3W_ABORT) {
        finish = true;
      } else {
        // ------------------------------------------------------ schedule_new_message (:421-648)
        int chosen = -1;
        bool chose_marker = false, none = false, by_wildcard = false;
        count++;
        if (count > max_messages) none = true;
        if (!none && args.stop_after_next_trace && pfx >= pfx_len) none = true;      // (:588-590)
        if (!none && !awaiting) {
          // getMatchingMessage, under getNextMatchingMessage's loop when prioritizePendingUponDivergence (:542-555)
          do {
            if (pfx >= pfx_len) break;
            const uint32_t pos = pfx;              // origNextTraceSize - nextTrace.size (:547)
            demi_dpor_trace_entry want = pf[pfx];
            while (want.kind == 0) {               // getNextTraceMessage: root / id-0 heads are skipped (:363-372)
              pfx++;
              if (pfx >= pfx_len) break;
              want = pf[pfx];
            }
            if (pfx < pfx_len) {
              pfx++;
              if (want.kind == 2) {
                if (marker_pending && want.key == dpor_marker_key(marker_ext)) chose_marker = true;
              } else if (want.kind == 3) {
                // ---- a wildcard (:477-514): every pending message of (snd, rcv), in send order
                const uint32_t snd = w_src((word_t)want.word), rcv = w_dst((word_t)want.word);
                const uint32_t types = (uint32_t)want.key, policy = (uint32_t)(want.key >> 32) & 0xFFu, mode = (uint32_t)(want.key >> 40) & 0xFFu;
                if (!((blocked >> rcv) & 1u)) {
                  uint32_t head_seq = 0xFFFFFFFFu, best_seq = 0;
                  int head = -1;
                  for (uint32_t k = 0; k < n_pend; k++) {
                    const word_t pw = pend_load(mem, k);
                    if (w_src(pw) != snd || w_dst(pw) != rcv) continue;
                    const uint32_t sq = aux_load(mem, k) >> 16;
                    if (sq < head_seq) { head_seq = sq; head = (int)k; }
                    if (!((types >> w_type(pw)) & 1u)) continue;
                    const bool better = chosen < 0 || (policy == DEMI_WILDCARD_LAST ? sq > best_seq : sq < best_seq);
                    if (better) { chosen = (int)k; best_seq = sq; }
                  }
                  if (policy == DEMI_WILDCARD_HEAD && chosen != head) chosen = -1;      // SrcDstFIFOOnly: the oldest must match
                  if (chosen >= 0) by_wildcard = true;
                  if (chosen >= 0 && policy == DEMI_WILDCARD_FIRST && mode != DEMI_WILDCARD_BACKTRACK_NONE) {
                    // backtrackSetter: of the later matches, the youngest of every message value that is not the first's,
                    // youngest first (reversed(matching.tail) with alreadyTried); LAST_DISTINCT stops at the first of them
                    const word_t first_w = pend_load(mem, (uint32_t)chosen);
                    uint32_t bound = 0xFFFFFFFFu;
                    for (;;) {
                      int cand = -1;
                      uint32_t cand_seq = 0;
                      for (uint32_t k = 0; k < n_pend; k++) {
                        const word_t pw = pend_load(mem, k);
                        if (w_src(pw) != snd || w_dst(pw) != rcv || !((types >> w_type(pw)) & 1u)) continue;
                        const uint32_t sq = aux_load(mem, k) >> 16;
                        if (sq > best_seq && sq < bound && (cand < 0 || sq > cand_seq)) { cand = (int)k; cand_seq = sq; }
                      }
                      if (cand < 0) break;
                      bound = cand_seq;
                      const word_t cw = pend_load(mem, (uint32_t)cand);
                      if (cw == first_w) continue;
                      bool youngest = true;      // (a younger pending message with this value was reported in its place)
                      for (uint32_t k = 0; k < n_pend && youngest; k++)
                        if (pend_load(mem, k) == cw && (aux_load(mem, k) >> 16) > cand_seq) youngest = false;
                      if (!youngest) continue;
                      if (n_alt >= args.max_alts) { flags |= DEMI_V_ALTS_OVF; break; }
                      const uint32_t aux = aux_load(mem, (uint32_t)cand);
                      demi_dpor_wild_alt r;
                      r.key = key_at((uint32_t)cand, cw, aux); r.word = (uint32_t)cw; r.trace_len = (uint16_t)n_trace;
                      r.next_pos = (uint8_t)pos; r.parent = (uint8_t)(aux & 0xFF);
                      args.alts[sched * (uint64_t)args.max_alts + n_alt] = r;
                      n_alt++;
                      if (mode == DEMI_WILDCARD_BACKTRACK_LAST_DISTINCT) break;
                    }
                  }
                }
              } else {
                // ---- an exact delivery: by node (kind 1, dequeueFirst(equivalentTo), :516-524) or by message word (kind 4)
                const bool by_word = want.kind == 4;
                const uint32_t rcv = w_dst((word_t)want.word);
                uint32_t best_seq = 0xFFFFFFFFu;
                if (!((blocked >> rcv) & 1u)) {
                  for (uint32_t k = 0; k < n_pend; k++) {
                    const word_t pw = pend_load(mem, k);
                    if (by_word ? pw != (word_t)want.key : (uint32_t)pw != want.word) continue;
                    const uint32_t aux = aux_load(mem, k);
                    if (!by_word && key_at(k, pw, aux) != want.key) continue;
                    if ((aux >> 16) < best_seq) { best_seq = aux >> 16; chosen = (int)k; }
                  }
                }
              }
            }
            if (chosen < 0 && !chose_marker && args.prioritize) K3W_SET_BIT(ig, pos);      // ignoreAbsentCallback(idx) (:549-552)
          } while (args.prioritize && chosen < 0 && !chose_marker && !(flags & K3W_ABORT));
        }
        if (flags & K3W_ABORT) {
          finish = true;
        } else {
        if (!none && chosen < 0 && !chose_marker) {
          if (!awaiting && args.stop_after_next_trace && pfx >= pfx_len) none = true;      // (:612-613)
          else {
            // getPendingEvent (:452-472), iteration order pinned: (snd, rcv) ascending, FIFO inside
            uint32_t best = 0xFFFFFFFFu;
            for (uint32_t k = 0; k < n_pend; k++) {
              const word_t pw = pend_load(mem, k);
              const uint32_t ord = (((w_src(pw) << 4) | w_dst(pw)) << 16) | (aux_load(mem, k) >> 16);
              const bool ok = !((blocked >> w_dst(pw)) & 1u) && ord < best;
              best = ok ? ord : best;
              chosen = ok ? (int)k : chosen;
            }
            if (chosen < 0 && marker_pending) chose_marker = true;
            if (chosen < 0 && !chose_marker) none = true;
          }
        }
        if (chose_marker) {                              // awaitQuiescenceUpdate (:256-266)
          marker_pending = false; awaiting = true; next_qperiod = marker_ext + 1; qmarker_ext = marker_ext;
        } else if (!none) {
          const word_t pw = pend_load(mem, (uint32_t)chosen);
          const uint32_t aux = aux_load(mem, (uint32_t)chosen);
          const uint64_t key = key_at((uint32_t)chosen, pw, aux);
          pend_remove_at((uint32_t)chosen);
          const uint32_t snd = w_src(pw), rcv = w_dst(pw);
          if ((snd < MAX_ACT && ((isolated >> snd) & 1)) || ((isolated >> rcv) & 1)) {
            if (snd == rcv) { flags |= DEMI_V_SELFMSG; finish = true; }   // (:631-633)
            // else: discarded, schedule again (:626-635)
          } else {
            const int ti = trace_push(key, pw, aux & 0xFF, (aux >> 8) & 0xFF, 1);
            if (ti < 0) finish = true;
            else {
              if (by_wildcard) K3W_SET_BIT(wc, (uint32_t)ti);
              parent = (uint32_t)ti; parent_depth = pushed_depth; parent_key = key;   // setParentEvent
              w = pw; deliver = true;
              deliveries++;
              hash_step(hash, w);
              const uint32_t type = w_type(w), meta = t.meta[type];
              if (((meta & 0xFF) == DEMI_MSG_TIMER) && (rep & ((tmask_t)1 << (rcv * DEMI_MAX_TIMER_TYPES + (meta >> 8)))))
                produce(msg_word(type, DL, rcv, 0, 0));   // retrigger: enqueue_timer = `!`
            }
          }
        } else {
          // ---------------------------------------------------- notify_quiescence (:855-942)
          if (awaiting) {
            awaiting = false;
            qperiod = next_qperiod; next_qperiod = 0;
            const int ti = trace_push(dpor_marker_key(qmarker_ext), 0, cur_root, qperiod, 2);
            if (ti < 0) finish = true;
            else {
              cur_root = (uint32_t)ti; parent = (uint32_t)ti; parent_depth = pushed_depth; parent_key = dpor_marker_key(qmarker_ext);
              run_external();
            }
          } else {
            finish = true;
          }
        }
        }
      }
    }

    uint32_t nfx = 0;
    if (deliver) nfx = DEMI_VM_RUN(t, mem, w, flags, app_rng);
    if (deliver) {
      const uint32_t me = w_dst(w);
      for (uint32_t k = 0; k < nfx && !(flags & DEMI_OVF_ANY); k++) {
        const word_t fxw = mem.fxq[k * 64];
        const uint32_t fx = (uint32_t)fxw;
        const uint32_t op = fx & 31u, type = (fx >> 5) & 31u, target = fx_target(fx);
        if (op <= DEMI_OP_BCAST) {
          const bool bc = (op == DEMI_OP_BCAST);
          const uint32_t first = bc ? 0u : target, last = bc ? A : (target < A ? target + 1 : 0u);
          for (uint32_t r = first; r < last; r++) {
            if (bc && r == me) continue;
            produce(fx_msg_word(fxw, type, me, r));
          }
        } else if (op == DEMI_OP_CRASH) {
          blocked |= 1u << me;                 // actorCrashed (Instrumenter.scala:184-199)
        } else if (op == DEMI_OP_TCANCEL) {
          // notify_timer_cancel (:961-984): first of the (deadLetters, rcv) queue with this message
          rep &= ~K3W_TIMER_BIT(me, type);
          const word_t wantw = msg_word(type, DL, me, 0, 0);
          int best = -1;
          uint32_t best_seq = 0xFFFFFFFFu;
          for (uint32_t q = 0; q < n_pend; q++) {
            if (pend_load(mem, q) != wantw) continue;
            const uint32_t sq = aux_load(mem, q) >> 16;
            if (sq < best_seq) { best_seq = sq; best = (int)q; }
          }
          if (best >= 0) pend_remove_at((uint32_t)best);
        } else {
          const tmask_t bit = K3W_TIMER_BIT(me, type);
          if (!(rep & bit)) {
            if (op == DEMI_OP_TREP) rep |= bit;
            produce(msg_word(type, DL, me, 0, 0));
          }
        }
      }
    }

    // ---------------------------------------------------------- finished interleavings
    if (active && finish) {
      const bool aborted = (flags & K3W_ABORT) != 0;
      uint32_t viol = 0;
      if (!aborted) {   // checkInvariant (:394-418)
        const uint32_t fp = invariant_code(t, st, (1u << A) - 1, A, DEMI_INV_KIND_OF(t), t.inv_fa, t.inv_va, t.inv_fb);
        if (fp) {
          if (!args.looking_for_valid) viol = fp;
          else if (((fp ^ args.looking_for) & t.fp_mask) == 0) viol = args.looking_for;
        }
      }
      for (uint32_t a = 0; a < A * ST_WORDS; a++) hash_step(hash, st[a * 64]);
      uint4 v;
      if (aborted) {
        v.x = flags & K3W_ABORT; v.y = 0; v.z = 0; v.w = 0;
        args.trace_len[sched] = 0;
        args.n_alts[sched] = 0;
      } else {
        v.x = (viol ? DEMI_V_VIOLATION : 0u) |
              ((count > max_messages) ? DEMI_V_MAXMSG : 0u) | ((deliveries < 0xFFFFu ? deliveries : 0xFFFFu) << 16);
        v.y = viol; v.z = (uint32_t)hash; v.w = (uint32_t)(hash >> 32);
        args.trace_len[sched] = n_trace;
        args.n_alts[sched] = n_alt;
      }
      *reinterpret_cast<uint4*>(&args.out[sched]) = v;
      uint64_t* const ig = args.ignored + sched * 4;
      ig[0] = aborted ? 0ull : ig0; ig[1] = aborted ? 0ull : ig1; ig[2] = aborted ? 0ull : ig2; ig[3] = aborted ? 0ull : ig3;
      uint64_t* const wc = args.wild + sched * 4;
      wc[0] = aborted ? 0ull : wc0; wc[1] = aborted ? 0ull : wc1; wc[2] = aborted ? 0ull : wc2; wc[3] = aborted ? 0ull : wc3;
      active = false;
    }
  }
#undef K3W_SET_BIT
#undef K3W_TIMER_BIT
#undef K3W_ABORT
}

}  // namespace demi
