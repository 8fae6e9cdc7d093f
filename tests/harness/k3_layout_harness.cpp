// The staging-area layouts of the K3 host path (demi_amd/csrc/k3_layout.hpp) without a GPU: every layout function at the shapes
// listed in k3_layout_expected.inc, where its offsets and total must EQUAL the literals - which were printed by the offset chains
// the host path spelled out at each place of use before the header existed, not by the header - and, whatever the literals say,
// must be a sound carving: fields in order that do not overlap, every aligned field a multiple of 256 bytes behind the start (or
// behind the packed field in front of it), every packed field's successor exactly behind its last byte, `total` covering the last.
// Built with -fsanitize=address,undefined by tests/test_k3_layout_cpu.py and run as a child process.
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../demi_amd/csrc/k3_layout.hpp"

using namespace k3_layout;

struct Expected { const char* area; std::vector<unsigned long long> in; std::vector<unsigned long long> out; };
static const Expected kExpected[] = {
#include "k3_layout_expected.inc"
};

struct Field { const char* name; size_t at, bytes; bool packed; };      // in carving order
static int failures = 0;
static void bad(const Expected& e, const std::string& what) {
  failures++;
  std::string in;
  for (unsigned long long x : e.in) in += " " + std::to_string(x);
  fprintf(stderr, "%s(%s ): %s\n", e.area, in.c_str(), what.c_str());
}

// the properties of a carving, and equality with the literals (`extra`: what the struct holds besides offsets and total)
static void check(const Expected& e, const std::vector<Field>& f, size_t total, const std::vector<size_t>& extra = {}) {
  size_t skew = 0;      // bytes of packed fields so far: what the aligned fields behind them are shifted by
  for (size_t i = 0; i < f.size(); i++) {
    const size_t end = i + 1 < f.size() ? f[i + 1].at : total;
    if (f[i].at + f[i].bytes > end) bad(e, std::string(f[i].name) + " overlaps what follows it");
    if ((f[i].at - skew) % 256) bad(e, std::string(f[i].name) + " is not 256-aligned");
    if (f[i].packed) {
      if (end != f[i].at + f[i].bytes) bad(e, std::string(f[i].name) + ": the next field is not exactly behind it");
      skew += f[i].bytes;
    } else if (end != f[i].at + align256(f[i].bytes)) bad(e, std::string(f[i].name) + ": its room is not its size rounded up to 256");
  }
  if (!f.empty() && f[0].at != 0) bad(e, "the first field is not at 0");
  std::vector<unsigned long long> got;
  for (const Field& x : f) got.push_back(x.at);
  got.push_back(total);
  for (size_t x : extra) got.push_back(x);
  if (got != e.out) {
    std::string s = "offsets differ from the literals:";
    for (unsigned long long x : got) s += " " + std::to_string(x);
    bad(e, s);
  }
}

int main() {
  int n_cases = 0;
  for (const Expected& e : kExpected) {
    const std::string a = e.area;
    const std::vector<unsigned long long>& in = e.in;
    n_cases++;
    if (a == "batch") {
      const uint64_t n = in[0]; const uint32_t stride = (uint32_t)in[1], mp = (uint32_t)in[2];
      const BatchLayout L = batch_area(n, stride, mp);
      check(e, {{"prefixes", L.o_pfx, sizeof(demi_dpor_trace_entry) * (size_t)stride * n, false}, {"prefix_len", L.o_pl, 4 * n, false},
                {"verdicts", L.o_v, sizeof(demi_verdict) * n, false}, {"traces", L.o_t, sizeof(demi_dpor_trace_entry) * DEMI_DPOR_MAX_TRACE * n, false},
                {"trace_len", L.o_tl, 4 * n, false}, {"pairs", L.o_p, sizeof(demi_dpor_pair) * (size_t)mp * n, false},
                {"n_pairs", L.o_np, 4 * n, false}, {"shared_len", L.o_sh, 4 * n, false}}, L.total);
    } else if (a == "round") {
      const uint32_t n = (uint32_t)in[0], mp = (uint32_t)in[1], pc = (uint32_t)in[2], kc = (uint32_t)in[3];
      const RoundLayout L = round_area(n, mp, pc, kc);
      check(e, {{"items", L.o_it, sizeof(demi::DporItem) * (size_t)n, false}, {"verdicts", L.o_v, sizeof(demi_verdict) * (size_t)n, false},
                {"n_pairs", L.o_np, 4 * (size_t)n, false}, {"pairs", L.o_p, sizeof(demi_dpor_pair) * (size_t)mp * n, false},
                {"pair_slot_of", L.o_ps, 4 * (size_t)mp * n, false}, {"points", L.o_pt, sizeof(demi::DporPoint) * (size_t)pc, false},
                {"kills", L.o_k, sizeof(demi::DporKill) * (size_t)kc, false}, {"counters", L.o_c, 32, false},
                {"surv_k", L.o_sk, 2 * (size_t)mp * n, false}, {"n_surv", L.o_ns, 4 * (size_t)n, false}}, L.total);
    } else if (a == "shard") {
      const uint32_t n = (uint32_t)in[0], W = (uint32_t)in[1], mp = (uint32_t)in[2], rc = (uint32_t)in[3], pc = (uint32_t)in[4], kc = (uint32_t)in[5];
      const ShardLayout L = shard_area(n, W, mp, rc, pc, kc);
      const size_t blk = L.blk;
      if (blk * W < n || (blk - 1) * W >= n) bad(e, "blk is not ceil(n / world)");
      check(e, {{"items", L.o_it, sizeof(demi::DporItem) * (size_t)n, false}, {"verdicts", L.o_v, sizeof(demi_verdict) * blk, false},
                {"verdicts of all", L.o_va, sizeof(demi_verdict) * blk * W, false}, {"n_pairs", L.o_np, 4 * blk, false},
                {"pairs", L.o_p, sizeof(demi_dpor_pair) * (size_t)mp * blk, false}, {"records", L.o_r, sizeof(demi::DporPairRec) * (size_t)rc, false},
                {"records of all", L.o_ra, sizeof(demi::DporPairRec) * (size_t)rc * W, false}, {"pair_slot_of", L.o_ps, 4 * (size_t)rc * W, false},
                {"points", L.o_pt, sizeof(demi::DporPoint) * (size_t)pc, false}, {"kills", L.o_k, sizeof(demi::DporKill) * (size_t)kc, false},
                {"counters", L.o_c, 32, false}, {"counters of all", L.o_ca, 32 * (size_t)W, false}}, L.total, {L.ra_bytes, L.blk});
      if (L.o_ps - L.o_ra != L.ra_bytes) bad(e, "ra_bytes is not the room of the gathered records");
    } else if (a == "q") {
      const uint32_t n = (uint32_t)in[0], mp = (uint32_t)in[1];
      const QLayout L = q_area(n, mp);
      check(e, {{"items", L.o_it, sizeof(demi::DporItem) * (size_t)n, false}, {"verdicts", L.o_v, sizeof(demi_verdict) * (size_t)n, true},
                {"result words", L.o_out, 8 * kQOutWords, false}, {"n_pairs", L.o_np, 4 * (size_t)n, false},
                {"pairs", L.o_p, sizeof(demi_dpor_pair) * (size_t)mp * n, false}, {"pair_slot_of", L.o_ps, 4 * (size_t)mp * n, false},
                {"surv_k", L.o_sk, 2 * (size_t)mp * n, false}, {"n_surv", L.o_ns, 4 * (size_t)n, false},
                {"keep_bits", L.o_kb, 8 * (size_t)((mp + 63) / 64) * n, false}, {"item_points", L.o_ip, 4 * (size_t)n, false},
                {"tile_sum", L.o_ts, 4 * (((size_t)n + 1023) / 1024), false}}, L.total, {L.out_bytes});
      // one read of out_bytes from the verdicts brings the result words too, all of them
      if (L.o_out != L.o_v + sizeof(demi_verdict) * (size_t)n || L.out_bytes != L.o_out + 8 * kQOutWords - L.o_v) bad(e, "verdicts + result words are not one read");
    } else if (a == "q_stage") {
      const uint32_t cap = (uint32_t)in[0];
      const QStageLayout L = q_stage_area(cap);
      if (L.tiles * kQTile < cap || (L.tiles - 1) * kQTile >= cap) bad(e, "tiles is not ceil(cap / tile)");
      check(e, {{"staging", L.o_staging, kQPointBytes * (size_t)cap, false}, {"tile_hist", L.o_tile_hist, 4 * 256 * L.tiles, false},
                {"digit_start", L.o_digit_start, 4 * 256, false}}, L.total, {L.tiles});
    } else if (a == "q_pop") {
      const uint32_t nr = (uint32_t)in[0], nc = (uint32_t)in[1], want = (uint32_t)in[2];
      const QPopLayout L = q_pop_area(nr, nc, want);
      check(e, {{"ranges", L.o_r, kQRangeBytes * (size_t)nr, false}, {"cand_slot", L.o_cs, 4 * (size_t)nc, false},
                {"blk_live", L.o_bl, 4 * (((size_t)nc + 255) / 256), false}, {"result words", L.o_out, 8 * kQPopWords, true},
                {"items", L.o_it, sizeof(demi::DporItem) * (size_t)want, false}}, L.total, {L.out_bytes});
      if (L.o_it != L.o_out + 8 * kQPopWords || L.out_bytes != L.o_it + sizeof(demi::DporItem) * (size_t)want - L.o_out) bad(e, "result words + items are not one read");
    } else if (a == "ref_pinned") {
      const uint32_t n = (uint32_t)in[0], nd = (uint32_t)in[1];
      const RefPinnedLayout L = ref_pinned_area(n, nd);
      check(e, {{"items", L.h_it, sizeof(demi::DporItem) * (size_t)n, false}, {"use_parent", L.h_up, n, false},
                {"deltas", L.h_dl, kRefDeltaBytes * (size_t)(nd ? nd : 1), false}, {"verdicts", L.h_v, sizeof(demi_verdict) * (size_t)n, false},
                {"counters", L.h_c, 64, false}, {"rec_cnt", L.h_rc, 4 * (size_t)n, false}}, L.total);
    } else if (a == "ref_device") {
      const uint32_t n = (uint32_t)in[0], nd = (uint32_t)in[1];
      const RefDeviceLayout L = ref_device_area(n, nd);
      check(e, {{"use_parent", L.o_up, n, false}, {"deltas", L.o_dl, kRefDeltaBytes * (size_t)(nd ? nd : 1), false}, {"counters", L.o_c, 16, false}}, L.total);
    } else if (a == "fetch") {
      const uint32_t m = (uint32_t)in[0], nd = (uint32_t)in[1];
      const FetchLayout L = fetch_area(m, nd);
      check(e, {{"ids", L.o_id, 4 * (size_t)m, false}, {"deltas", L.o_dl, kRefDeltaBytes * (size_t)(nd ? nd : 1), false},
                {"offsets", L.o_off, 8 * (size_t)m, false}, {"counts", L.o_cnt, 4 * (size_t)m, false}, {"table full", L.o_fl, 8, false}}, L.total);
    } else {
      bad(e, "no such area");
    }
  }
  // the prefix a launch of the REFERENCE order reads of a round's area does not depend on what lies behind it: the same offsets
  // as an area without survivors' room would have (max_pairs = 0 behind o_c changes nothing in front of it)
  {
    const RoundLayout A = round_area(63, 64, 1u << 21, 1u << 21);
    Carve c;
    const size_t o_it = c.take(8 * 63), o_v = c.take(16 * 63), o_np = c.take(4 * 63), o_p = c.take(4 * 64 * 63);
    if (A.o_it != o_it || A.o_v != o_v || A.o_np != o_np || A.o_p != o_p || A.o_c >= A.o_sk) { failures++; fprintf(stderr, "round: the prefix the REFERENCE order reads moved\n"); }
    n_cases++;
  }
  // the cursor itself
  {
    Carve c;
    const size_t a0 = c.take(1), a1 = c.take_packed(16), a2 = c.take(0), a3 = c.take(257);
    if (a0 != 0 || a1 != 256 || a2 != 272 || a3 != 272 || c.at != 272 + 512) { failures++; fprintf(stderr, "Carve\n"); }
    n_cases++;
  }
  if (failures) { fprintf(stderr, "k3_layout: %d failures\n", failures); return 1; }
  printf("k3_layout: %d cases ok\n", n_cases);
  return 0;
}
