// k2_wildcard_body.hpp - the body of k2_replay_wildcard (k2_wildcard.hpp), k2_replay_wildcard_candidates
// (k2_wildcard_cand.hpp) and k2_replay_wildcard_round (k2_wildcard_round.hpp).  NOT a header of its own: it is included inside a
// kernel that has `args` (K2WArgs), `cand` (K2WCand) and the macro K2W_CAND (0 / 1) in scope; K2W_ROUND (1: the round kernel,
// with K2W_CAND 0) is optional.  No include guard: once per kernel.
#ifndef K2W_ROUND
#define K2W_ROUND 0
#define K2W_ROUND_DEFAULTED 1
#endif
  constexpr bool CAND = K2W_CAND != 0;
  constexpr bool ROUND = K2W_ROUND != 0;   // explicit presence rows and the kept plane as the batch kernel, the executed length
  constexpr bool XLEN = CAND || ROUND;     // counted as the candidates kernel does, the launch reduced into cand.key[0] / first_ovf[0]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Tables t;
  unsigned char* wave_base = tables_load(t, smem, args.model, args.ext, args.n_ext, args.exists);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t NX = args.n_exp;
  const uint64_t* expected = args.expected;
  const LaneMem mem = lane_mem_carve(wave_base + (size_t)wave * lane_mem_wave_bytes(t.A, true), t.A, true, lane,
                                     args.spill, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
  uint64_t* const st = mem.st;
  const uint32_t A = t.A, NE = t.E, exists = t.exists, PMAX = args.p_max;

#define IN_MASK(I) ((uint32_t)((((((I) >> 6) & 3u) == 0u ? m0 : 0ull) | ((((I) >> 6) & 3u) == 1u ? m1 : 0ull) | \
                                ((((I) >> 6) & 3u) == 2u ? m2 : 0ull) | ((((I) >> 6) & 3u) == 3u ? m3 : 0ull)) >> ((I) & 63u)) & 1u)
#define TIMER_BIT(RCV, TYPE) ((tmask_t)1 << ((RCV) * DEMI_MAX_TIMER_TYPES + (t.meta[(TYPE)] >> 8)))
#ifdef DEMI_WIDE
#define EXP_WORD(E, I, SRC, DST) msg_word_area((uint32_t)((E) >> 24) & 0xFF, (SRC), (DST), args.exp_area[(I)])
#else
#define EXP_WORD(E, I, SRC, DST) msg_word((uint32_t)((E) >> 24) & 0xFF, (SRC), (DST), (uint32_t)((E) >> 32) & 0xFFu, (uint32_t)((E) >> 40) & 0xFFu)
#endif
// the executed trace (event_orchestrator.events): AREA is demi_rec_event's p0 | p1 << 16 | p_hi << 32
#define REC_PUSH(KIND, SND, RCV, TYPE, AREA, FL, EXT, ID)                                     \
  do {                                                                                        \
    if (rec) {                                                                                \
      if (n_rec < args.rec_cap) {                                                             \
        demi_rec_event e_;                                                                    \
        e_.kind = (uint8_t)(KIND); e_.snd = (uint8_t)(SND); e_.rcv = (uint8_t)(RCV);          \
        const uint64_t ar_ = (uint64_t)(AREA);                                                \
        e_.msg_type = (uint8_t)(TYPE); e_.p0 = (uint16_t)ar_; e_.p1 = (uint16_t)(ar_ >> 16);  \
        e_.flags = (uint8_t)(FL); e_.ext_idx = (uint8_t)(EXT); e_.p_hi = (uint16_t)(ar_ >> 32); e_.id = (ID); \
        rec[n_rec] = e_;                                                                      \
      }                                                                                       \
      n_rec++;                                                                                \
    }                                                                                         \
  } while (0)
// event_produced (:561-623): the message gets the next Uniq id (send order) and joins the pending set
#define PEND_APPEND(WORD, FL, EXT)                                                            \
  do {                                                                                        \
    const word_t w_ = (WORD);                                                                 \
    if (n_pend >= PMAX) { flags |= DEMI_V_PENDING_OVF; }                                      \
    else {                                                                                    \
      /* (candidates, round: the sequence number carries whether the message is an external MsgSend; the order is the ids') */ \
      pend_store(mem, n_pend, w_); aux_store(mem, n_pend, XLEN ? ((next_id << 1) | ((FL) == 1 ? 1u : 0u)) : next_id); n_pend++; \
      if (XLEN && (FL) == 1) xlen++;                                                          \
      REC_PUSH(DEMI_REC_MSG_SEND, w_src(w_), w_dst(w_), w_type(w_), w_area(w_), (FL), (EXT), next_id); \
      next_id++;                                                                              \
    }                                                                                         \
  } while (0)

  for (;;) {
    uint64_t base = 0;
    if (lane == 0) base = atomicAdd(args.work_counter, (unsigned long long)args.lanes_per_wave);
    base = __shfl(base, 0);
    if (base >= args.n) break;
    const uint64_t sched = base + lane;
    if (!(lane < args.lanes_per_wave && sched < args.n)) continue;      // (no cross-lane operation from here to the end of the body)

    // candidates: sched = c * (1 + n_drop) + j
    const uint64_t cand_c = CAND ? sched / (cand.n_drop + 1u) : 0ull;
    const uint32_t cand_j = CAND ? (uint32_t)(sched - cand_c * (cand.n_drop + 1u)) : 0u;
    const uint32_t dropped = (CAND && cand_j) ? cand.drops[cand_j - 1] : 0xFFFFFFFFu;
    // The executed trace's length in the convention of demi_replay_wildcard_get_trace, counted without recording it: applied
    // external events, external MsgSends, every MsgEvent, and the MsgSend of every DELIVERED internal or timer message.
    uint32_t xlen = 0;
    uint64_t m0, m1, m2, m3;
    if (args.masks) {
      const uint64_t* mk = args.masks + (CAND ? cand_c : ROUND ? 0ull : sched) * 4;      // (round: one row for all)
      m0 = mk[0]; m1 = mk[1]; m2 = mk[2]; m3 = mk[3];
    } else {
      m0 = m1 = m2 = m3 = ~0ull;
    }
    const uint64_t* present = CAND ? cand.base_present : args.present + sched * (uint64_t)args.present_words;
    demi_rec_event* rec = (!CAND && !ROUND && args.rec_out) ? args.rec_out + sched * (uint64_t)args.rec_cap : nullptr;
    uint64_t hash = 0xCBF29CE484222325ULL;
    uint64_t app_rng = jr_seed(0);
    Net net;
    net.inaccessible = exists; net.killed = 0; pairs_clear(net.partitioned);
    for (uint32_t a = 0; a < A * ST_WORDS; a++) st[a * 64] = t.init[a];
    uint32_t idx = 0, cur = 0, n_pend = 0, count = 0, ignored = 0, flags = 0, blocked = 0;
    uint32_t next_id = 1, n_rec = 0;
    tmask_t rep = 0;
    uint64_t tq = 0;
    uint32_t n_tq = 0;

    auto cur_skip = [&]() __attribute__((always_inline)) {
      while (cur < NE) {
        const uint32_t kind = (uint32_t)t.trace[cur] & 0xFF;
        if (IN_MASK(cur) && kind != DEMI_EV_SEND && kind != DEMI_EV_WAIT_QUIESCENCE) break;
        cur++;
      }
    };
    auto handle_timer = [&](uint32_t rcv, uint32_t type) __attribute__((always_inline)) {
      if (n_tq >= DEMI_TQ_CAP) { flags |= DEMI_V_QUEUE_OVF; return; }
      tq |= (uint64_t)tq_pack(rcv, type, 0u) << (8 * n_tq);
      n_tq++;
    };
    // swap-remove of slot k: the words and their sequence numbers move together
    auto pend_remove = [&](uint32_t k) __attribute__((always_inline)) {
      n_pend--;
      if (k != n_pend) { pend_store(mem, k, pend_load(mem, n_pend)); aux_store(mem, k, aux_load(mem, n_pend)); }
    };
    cur_skip();

    for (;;) {
      // -------------------------------------------------------- advanceReplay (:405-559)
      word_t w = 0;
      uint32_t wid = 0;
      bool deliver = false;
      while (idx < NX && !(flags & DEMI_OVF_ANY)) {
        const uint64_t e = expected[idx];
        idx++;
        const uint32_t kind = (uint32_t)e & 0xFF, a = (uint32_t)(e >> 8) & 0xFF, b = (uint32_t)(e >> 16) & 0xFF;
        const uint32_t ext = (uint32_t)(e >> 48) & 0xFF;
        if (kind <= DEMI_REC_UNPARTITION) {
          if (cur >= NE) continue;
          const uint64_t x = t.trace[cur];
          const uint32_t xk = (uint32_t)x & 0xFF, xa = (uint32_t)(x >> 8) & 0xFF, xb = (uint32_t)(x >> 16) & 0xFF;
          const bool two = kind >= DEMI_REC_PARTITION;
          const uint32_t want_kind = (kind == DEMI_REC_SPAWN) ? DEMI_EV_START : (kind == DEMI_REC_KILL) ? DEMI_EV_KILL
                                   : (kind == DEMI_REC_PARTITION) ? DEMI_EV_PARTITION : DEMI_EV_UNPARTITION;
          if (xk != want_kind || xa != a || (two && xb != b)) continue;
          cur++;
          cur_skip();
          if (!CAND && args.kept) args.kept[sched * NX + idx - 1] = 1;
          if (XLEN) xlen++;
          REC_PUSH(kind, two ? a : 0u, two ? b : a, 0, 0, 0, ext, 0);
          if (kind == DEMI_REC_SPAWN) { net.inaccessible &= ~(1u << a); net.killed &= ~(1u << a); blocked &= ~(1u << a); }
          else if (kind == DEMI_REC_KILL) { net.killed |= 1u << a; net.inaccessible |= 1u << a; }
          else if (kind == DEMI_REC_PARTITION) pairs_put(net.partitioned, a, b, true);
          else pairs_put(net.partitioned, a, b, false);
        } else if (kind == DEMI_REC_MSG_SEND) {
          // external MsgSend -> enqueue_message (:509-511) unless its Send was pruned (the lowering holds no other MsgSend)
          if (ext != 255 && IN_MASK(ext) && ((exists >> b) & 1)) {
            PEND_APPEND(EXP_WORD(e, idx - 1, DL, b), 1, ext);
            if (!CAND && args.kept && !(flags & DEMI_OVF_ANY)) args.kept[sched * NX + idx - 1] = 1;
          }
        } else {  // MSG_EVENT
          const uint64_t s = args.sel[idx - 1];
          const uint32_t ri = (uint32_t)(s >> 40), policy = (uint32_t)(s >> 32) & 0xFFu, types = (uint32_t)s;
          if (CAND ? (ri == dropped || (present && !((present[ri >> 6] >> (ri & 63u)) & 1ull)))
                   : !((present[ri >> 6] >> (ri & 63u)) & 1ull)) continue;   // outside the candidate's cluster: not part of the trace
          if (ext != 255 && !IN_MASK(ext)) continue;                  // pruned together with its Send (filterSends)
          if ((blocked >> b) & 1u) { ignored++; continue; }           // (:392-402)
          // ---- messagePending + schedule_new_message: which pending entry this event takes (0xFFFFFFFF: none)
          const word_t want = EXP_WORD(e, idx - 1, a, b);
          uint32_t best = 0xFFFFFFFFu, best_seq = 0;
          bool best_in = false;            // HEAD: is the oldest entry's type in the set
          for (uint32_t k = 0; k < n_pend; k++) {
            const word_t pw = pend_load(mem, k);
            if (w_src(pw) != a || w_dst(pw) != b) continue;
            const bool in = types == 0 ? pw == want : ((types >> w_type(pw)) & 1u) != 0;
            if (policy != K2W_HEAD && !in) continue;                  // (an exact delivery is lowered with policy FIRST)
            const uint32_t sq = aux_load(mem, k);
            bool better;
            if (policy == K2W_LAST) {
              // only the oldest entry of each word (the head of its fingerprint group) counts
              bool head = true;
              for (uint32_t j = 0; j < n_pend && head; j++)
                if (j != k && pend_load(mem, j) == pw && aux_load(mem, j) < sq) head = false;
              if (!head) continue;
              better = best == 0xFFFFFFFFu || sq > best_seq;
            } else {
              better = best == 0xFFFFFFFFu || sq < best_seq;
            }
            if (better) { best = k; best_seq = sq; best_in = in; }
          }
          if (best == 0xFFFFFFFFu || (policy == K2W_HEAD && !best_in)) { ignored++; continue; }   // "Ignoring message" (:528-529)
          w = pend_load(mem, best);
          wid = best_seq;
          pend_remove(best);
          if (!CAND && args.kept) args.kept[sched * NX + idx - 1] = 1;
          deliver = true;
          break;
        }
      }
      if (!deliver) break;
      const uint32_t type = w_type(w), me = w_dst(w);
      count++;
      hash_step(hash, w);
      if (XLEN) xlen += 2u - (wid & 1u);
      REC_PUSH(DEMI_REC_MSG_EVENT, w_src(w), me, type, w_area(w), 0, 255, wid);
      {
        // Instrumenter retrigger of a repeating timer (Instrumenter.scala:1008-1016)
        const uint32_t meta = t.meta[type];
        if (((meta & 0xFF) == DEMI_MSG_TIMER) && (rep & ((tmask_t)1 << (me * DEMI_MAX_TIMER_TYPES + (meta >> 8)))))
          handle_timer(me, type);
        if (flags & DEMI_OVF_ANY) break;
      }
      const uint32_t nfx = DEMI_VM_RUN(t, mem, w, flags, app_rng);
      for (uint32_t k = 0; k < nfx && !(flags & DEMI_OVF_ANY); k++) {
        const word_t fxw = mem.fxq[k * 64];
        const uint32_t fx = (uint32_t)fxw;
        const uint32_t op = fx & 31u, ftype = (fx >> 5) & 31u, target = fx_target(fx);
        if (op <= DEMI_OP_BCAST) {
          const bool bc = (op == DEMI_OP_BCAST);
          const uint32_t first = bc ? 0u : target, last = bc ? A : (target < A ? target + 1 : 0u);
          for (uint32_t r = first; r < last; r++) {
            if ((bc && r == me) || !((exists >> r) & 1)) continue;
            if (!crosses_partition(net, me, r)) PEND_APPEND(fx_msg_word(fxw, ftype, me, r), 0, 255);
          }
        } else if (op == DEMI_OP_CRASH) {
          blocked |= 1u << me;                 // actorCrashed (Instrumenter.scala:184-199)
        } else if (op == DEMI_OP_TCANCEL) {
          // notify_timer_cancel (:828-855): messagesToSend first, then the first of the (deadLetters, rcv) queue
          rep &= ~TIMER_BIT(me, ftype);
          const uint32_t wantt = tq_pack(me, ftype, 0u);
          bool found = false;
          for (uint32_t q = 0; q < n_tq; q++) {
            if (((uint32_t)(tq >> (8 * q)) & 0xFF) == wantt) {
              const uint64_t lowm = (q == 0) ? 0ull : (~0ull >> (64 - 8 * q));
              tq = (tq & lowm) | ((tq >> 8) & ~lowm);
              n_tq--; found = true; break;
            }
          }
          if (!found) {
            const word_t wantw = msg_word(ftype, DL, me, 0, 0);
            uint32_t best = 0xFFFFFFFFu, best_seq = 0;
            for (uint32_t q = 0; q < n_pend; q++) {
              if (pend_load(mem, q) != wantw) continue;
              const uint32_t sq = aux_load(mem, q);
              if (best == 0xFFFFFFFFu || sq < best_seq) { best = q; best_seq = sq; }
            }
            if (best != 0xFFFFFFFFu) pend_remove(best);
          }
        } else {
          const tmask_t bit = TIMER_BIT(me, ftype);
          if (!(rep & bit)) {
            if (op == DEMI_OP_TREP) rep |= bit;
            handle_timer(me, ftype);
          }
        }
      }
      // schedule_new_message starts with send_external_messages (:655): timers become pending now,
      // unless the receiver is inaccessible (crosses_partition(deadLetters, rcv))
      for (uint32_t k = 0; k < n_tq && !(flags & DEMI_OVF_ANY); k++) {
        const uint32_t bt = (uint32_t)(tq >> (8 * k)) & 0xFF, rcv = tq_rcv(bt), ttype = tq_type(bt);
        if (!((net.inaccessible >> rcv) & 1)) PEND_APPEND(msg_word(ttype, DL, rcv, 0, 0), 2, 255);
      }
      tq = 0; n_tq = 0;
      if (flags & DEMI_OVF_ANY) break;
    }

    // the invariant on the final state; verdict = fingerprint.matches(target) (:278-300)
    uint32_t viol = 0;
    if (!(flags & DEMI_OVF_ANY)) {
      const uint32_t fp = invariant_code(t, st, exists, A, DEMI_INV_KIND_OF(t), t.inv_fa, t.inv_va, t.inv_fb);
      if (fp && (((fp ^ args.looking_for) & t.fp_mask) == 0)) viol = args.looking_for;
    }
    for (uint32_t a = 0; a < A * ST_WORDS; a++) hash_step(hash, st[a * 64]);
    uint4 v;
    if (flags & DEMI_OVF_ANY) {
      v.x = flags & DEMI_OVF_ANY; v.y = 0; v.z = 0; v.w = 0;
    } else {
      v.x = (viol ? DEMI_V_VIOLATION : 0u) | (ignored ? DEMI_V_DIVERGED : 0u) | ((count < 0xFFFFu ? count : 0xFFFFu) << 16);
      v.y = viol; v.z = (uint32_t)hash; v.w = (uint32_t)(hash >> 32);
    }
    *reinterpret_cast<uint4*>(&args.out[sched]) = v;
    if (!CAND && args.rec_n) args.rec_n[sched] = n_rec;
    if (CAND) {
      // the candidate's record: vector atomics on its two words; whichever lane runs first or last, the minima are the same
      if (flags & DEMI_OVF_ANY) atomicMin(&cand.first_ovf[cand_c], cand_j);
      else if (viol) atomicMin(&cand.key[cand_c], ((unsigned long long)cand_j << 32) | (unsigned long long)xlen);
    }
    if (ROUND) {
      // the round's record: the lowest reproducing proposal with its executed length, and the lowest aborted one
      if (flags & DEMI_OVF_ANY) atomicMin(&cand.first_ovf[0], (uint32_t)sched);
      else if (viol) atomicMin(&cand.key[0], ((unsigned long long)sched << 32) | (unsigned long long)xlen);
    }
  }
#undef IN_MASK
#undef EXP_WORD
#undef TIMER_BIT
#undef PEND_APPEND
#undef REC_PUSH
#ifdef K2W_ROUND_DEFAULTED
#undef K2W_ROUND
#undef K2W_ROUND_DEFAULTED
#endif
