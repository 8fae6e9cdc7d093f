// k3_layout.hpp — where the staging areas of the K3 (DPOR) host path keep what: one function per area.
// Every area is one allocation that its user carves by byte offsets.  The offsets used to be `o_x = o_y + s_y` chains at the
// place of use, nine of them; here each area is a function of its shape that returns named offsets and `total`, and the
// adjacencies some readers rely on (one copy that brings two fields) are properties of the function.  A struct names its fields
// in carving order and the function lists their sizes in that order; tests/harness/k3_layout_harness.cpp holds order, alignment,
// adjacency and the literal offsets.
// Host arithmetic only, and no HIP: the records' sizes that only device headers declare are constants here, and demi_gpu.hip
// asserts them against the types.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include "../../include/demi_gpu.h"
#include "dpor_types.hpp"

namespace k3_layout {
constexpr size_t kQPointBytes = 24, kQRangeBytes = 16, kRefDeltaBytes = 24;      // demi::QPoint, QRange, RefDeltaDev
constexpr size_t kQTile = 2048;                                                  // demi::Q_TILE
constexpr size_t kQOutWords = 260;     // a queue round's result words: count, reported, table full, dropped, 256 run lengths
constexpr size_t kQPopWords = 4;       // a dequeue's result words
constexpr size_t kCounterBytes = 4 * sizeof(unsigned long long);      // a round's counters: points, kills, table full, records
constexpr size_t kItem = sizeof(demi::DporItem), kVerdict = sizeof(demi_verdict), kPair = sizeof(demi_dpor_pair),
                 kEntry = sizeof(demi_dpor_trace_entry), kPoint = sizeof(demi::DporPoint), kKill = sizeof(demi::DporKill),
                 kRec = sizeof(demi::DporPairRec);

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The carving cursor.  take: the field gets its size rounded up to 256 bytes, so a chain of takes from 0 keeps every offset
// 256-aligned.  take_packed: the next field starts at this one's last byte + 1 - for fields that ONE copy reads together.  (The
// fields behind a packed one are shifted by its size: they are as aligned as that size is.)  The functions below carve inside
// a braced list, which is evaluated left to right.
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at += align256(bytes); return o; }
  size_t take_packed(size_t bytes) { const size_t o = at; at += bytes; return o; }
};

// demi_dpor_batch / the ordered and host-bookkeeping loops (ctx->d_dpor): prefixes, their lengths, verdicts, traces, trace
// lengths, pairs, pair counts, and the shared lengths last
struct BatchLayout { size_t o_pfx, o_pl, o_v, o_t, o_tl, o_p, o_np, o_sh, total; };
inline BatchLayout batch_area(uint64_t n, uint32_t stride, uint32_t max_pairs) {
  Carve c;
  return {c.take(kEntry * (size_t)stride * n), c.take(4 * n), c.take(kVerdict * n), c.take(kEntry * DEMI_DPOR_MAX_TRACE * n),
          c.take(4 * n), c.take(kPair * (size_t)max_pairs * n), c.take(4 * n), c.take(4 * n), c.at};
}

// demi_dpor_wildcard_batch / demi_wildcard_dpor_test (ctx->d_dpor): prefixes, their lengths, verdicts, traces, trace lengths,
// the ignored-position and picked-by-wildcard masks (256 bits each per interleaving), the alternative records and their counts
struct WildBatchLayout { size_t o_pfx, o_pl, o_v, o_t, o_tl, o_ig, o_wc, o_al, o_na, total; };
inline WildBatchLayout wild_batch_area(uint64_t n, uint32_t stride, uint32_t max_alts) {
  Carve c;
  return {c.take(kEntry * (size_t)stride * n), c.take(4 * n), c.take(kVerdict * n), c.take(kEntry * DEMI_DPOR_MAX_TRACE * n),
          c.take(4 * n), c.take(32 * n), c.take(32 * n), c.take(sizeof(demi_dpor_wild_alt) * (size_t)max_alts * n), c.take(4 * n), c.at};
}

// A round of the resident exploration (ctx->d_res): items, verdicts, pair counts, pairs, the flipped pairs' slots, decided
// points, kills, counters - so far also what a launch of the REFERENCE order reads (round_ref_begin: items, pairs, pair
// counts, verdicts, counters) - and behind them the parent filter's survivors and their counts.
struct RoundLayout { size_t o_it, o_v, o_np, o_p, o_ps, o_pt, o_k, o_c, o_sk, o_ns, total; };
inline RoundLayout round_area(uint32_t n, uint32_t max_pairs, uint32_t points_cap, uint32_t kills_cap) {
  Carve c;
  const size_t mp = max_pairs;
  return {c.take(kItem * n), c.take(kVerdict * n), c.take(4 * (size_t)n), c.take(kPair * mp * n), c.take(4 * mp * n),
          c.take(kPoint * points_cap), c.take(kKill * kills_cap), c.take(kCounterBytes), c.take(2 * mp * n), c.take(4 * (size_t)n), c.at};
}

// A round over `world` ranks (ctx->d_res): every rank runs a block of blk = ceil(n / world) items.  Items; this rank's
// verdicts and (o_va) all ranks'; pair counts, pairs; this rank's records and (o_ra) all ranks'; the flipped slots, points,
// kills; this rank's counters and (o_ca) all ranks'.  The gathered points and kills reuse o_ra, whose room is ra_bytes.
struct ShardLayout { size_t o_it, o_v, o_va, o_np, o_p, o_r, o_ra, o_ps, o_pt, o_k, o_c, o_ca, total, ra_bytes; uint32_t blk; };
inline ShardLayout shard_area(uint32_t n, uint32_t world, uint32_t max_pairs, uint32_t recs_cap, uint32_t points_cap, uint32_t kills_cap) {
  Carve c;
  const size_t W = world, blk = (n + world - 1) / world, mp = max_pairs, recs = recs_cap;
  return {c.take(kItem * n), c.take(kVerdict * blk), c.take(kVerdict * blk * W), c.take(4 * blk), c.take(kPair * mp * blk),
          c.take(kRec * recs), c.take(kRec * recs * W), c.take(4 * recs * W), c.take(kPoint * points_cap), c.take(kKill * kills_cap),
          c.take(kCounterBytes), c.take(kCounterBytes * W), c.at, align256(kRec * recs * W), (uint32_t)blk};
}

// A round with the backtrack queue on the device (ctx->d_res): items; the verdicts and right behind them the result words -
// one copy of out_bytes from o_v reads both -; pair counts, pairs, flipped slots, survivors and their counts; the keep bits,
// the per-interleaving point counts and the scan's tile sums
struct QLayout { size_t o_it, o_v, o_out, o_np, o_p, o_ps, o_sk, o_ns, o_kb, o_ip, o_ts, total, out_bytes; };
inline QLayout q_area(uint32_t n, uint32_t max_pairs) {
  Carve c;
  const size_t mp = max_pairs, words = (max_pairs + 63) / 64;
  return {c.take(kItem * n), c.take_packed(kVerdict * n), c.take(8 * kQOutWords), c.take(4 * (size_t)n), c.take(kPair * mp * n),
          c.take(4 * mp * n), c.take(2 * mp * n), c.take(4 * (size_t)n), c.take(8 * words * n), c.take(4 * (size_t)n),
          c.take(4 * (((size_t)n + 1023) / 1024)), c.at, kVerdict * n + 8 * kQOutWords};
}

// The staging area of a queue round's points (ctx->d_qstage), `cap` points: the points in creation order, a histogram of 256
// branches per tile of kQTile points, the 256 digit starts
struct QStageLayout { size_t o_staging, o_tile_hist, o_digit_start, total, tiles; };
inline QStageLayout q_stage_area(uint32_t cap) {
  Carve c;
  const size_t tiles = ((size_t)cap + kQTile - 1) / kQTile;
  return {c.take(kQPointBytes * cap), c.take(4 * 256 * tiles), c.take(4 * 256), c.at, tiles};
}

// A dequeue (ctx->d_qpop): the ranges; the candidates' slots; the live counts per block of 256 candidates; the result words and
// right behind them the items - one copy of out_bytes from o_out reads both
struct QPopLayout { size_t o_r, o_cs, o_bl, o_out, o_it, total, out_bytes; };
inline QPopLayout q_pop_area(uint32_t n_ranges, uint32_t n_cand, uint32_t want) {
  Carve c;
  return {c.take(kQRangeBytes * n_ranges), c.take(4 * (size_t)n_cand), c.take(4 * (((size_t)n_cand + 255) / 256)),
          c.take_packed(8 * kQPopWords), c.take(kItem * want), c.at, 8 * kQPopWords + kItem * want};
}

// A launch of the REFERENCE order, its pinned area (ctx->h_round): [items | use_parent | deltas] up, [verdicts | the round's
// four and the filter's two counters (room for eight) | record counts] down ...
struct RefPinnedLayout { size_t h_it, h_up, h_dl, h_v, h_c, h_rc, total; };
inline RefPinnedLayout ref_pinned_area(uint32_t n, uint32_t n_deltas) {
  Carve c;
  return {c.take(kItem * n), c.take(n), c.take(kRefDeltaBytes * (n_deltas ? n_deltas : 1)), c.take(kVerdict * n),
          c.take(8 * sizeof(unsigned long long)), c.take(4 * (size_t)n), c.at};
}
// ... and the commit filter's device area (ctx->d_ref): room for the flags and the deltas (read where they lie in the pinned
// area since round 6), and the filter's two counters
struct RefDeviceLayout { size_t o_up, o_dl, o_c, total; };
inline RefDeviceLayout ref_device_area(uint32_t n, uint32_t n_deltas) {
  Carve c;
  return {c.take(n), c.take(kRefDeltaBytes * (n_deltas ? n_deltas : 1)), c.take(2 * sizeof(unsigned long long)), c.at};
}

// A record fetch of the REFERENCE order's commit (ctx->h_fetch, pinned and device-mapped): the ids and the deltas up; per id
// the answer's offset and count, and the table-full word, down
struct FetchLayout { size_t o_id, o_dl, o_off, o_cnt, o_fl, total; };
inline FetchLayout fetch_area(uint32_t m, uint32_t n_deltas) {
  Carve c;
  return {c.take(4 * (size_t)m), c.take(kRefDeltaBytes * (n_deltas ? n_deltas : 1)), c.take(8 * (size_t)m), c.take(4 * (size_t)m),
          c.take(sizeof(unsigned long long)), c.at};
}

}  // namespace k3_layout
