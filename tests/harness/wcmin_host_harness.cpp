// wcmin_host_harness.cpp — demi_amd/csrc/wcmin_host.hpp (host-only code of the product) driven by a file of recorded replays
// instead of demi_replay_wildcard_round.  TEST INFRASTRUCTURE: a stand-alone program, built with the sanitizers by
// tests/test_wcmin_host_cpu.py and run as a child process.  There is no C wildcard oracle: the Python side runs the mirror over
// the transliterated device and writes down every presence row it asked for, with its answer; a row the native loop asks for
// that is not in the file fails the case by name.
//
//   wcmin_host_harness CASE OUT
// CASE (little endian): u32 magic 'WCM1', clustering, policy, skip_clock_clusters, max_batch, clock_increment_types, n_msg_types,
//   n_payloads, n_rec; clock_field [32] u8; msg_class [n_msg_types] u8; the loaded execution [n_rec] demi_rec_event; u32 n_segments;
//   per segment (one per load of the mirror's oracle, in order): u32 n (events of the loaded trace), n_rows; the trace [n]
//   demi_rec_event; type_sets [n] u32; policies [n] u8; per row: u32 reproduces, executed_len, has_trace; present
//   [ceil(n / 64)] u64; kept [n] u8; the executed trace [executed_len] demi_rec_event if has_trace.
// OUT: u32 status, n_trace, n_sizes, n_batches, adoptions, rounds, u64 total_replays; then the trace (demi_rec_event), the sizes
//   (u32), the batches (u32).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../../demi_amd/csrc/wcmin_host.hpp"

namespace {

struct Reader {
  FILE* f;
  bool ok = true;
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) ok = false; }
  uint32_t u32() { uint32_t x = 0; get(&x, 1); return x; }
};

struct Row {
  bool reproduces = false, has_trace = false;
  uint32_t executed_len = 0;
  std::vector<uint8_t> kept;
  std::vector<demi_rec_event> trace;
};
struct Segment {
  std::vector<demi_rec_event> trace;
  std::vector<uint32_t> type_sets;
  std::vector<uint8_t> policies;
  std::map<std::vector<uint64_t>, Row> rows;
};

// the rounds answered from the recorded replays of the current segment, in proposal order, as the sequential loop asks
struct RecordedRounds {
  std::vector<Segment> segments;
  size_t cur = 0;
  bool selected = false;
  const Segment& seg() const { return segments[cur]; }
  int selectors(const uint32_t* ts, const uint8_t* po) {
    if (cur >= segments.size()) { fprintf(stderr, "selectors: no segment left in the case file\n"); return DEMI_ERR_INVALID_ARG; }
    const Segment& s = seg();
    const size_t n = s.trace.size();
    if ((n && memcmp(ts, s.type_sets.data(), sizeof(uint32_t) * n)) || (n && memcmp(po, s.policies.data(), n))) {
      fprintf(stderr, "selectors: not the selectors the mirror loaded for segment %zu\n", cur);
      return DEMI_ERR_INVALID_ARG;
    }
    selected = true;
    return DEMI_OK;
  }
  const Row* find(const uint64_t* present, const char* who) const {
    const size_t words = (seg().trace.size() + 63) / 64;
    const std::vector<uint64_t> key(present, present + words);
    auto it = seg().rows.find(key);
    if (it == seg().rows.end()) { fprintf(stderr, "%s: a presence row of segment %zu is not in the case file\n", who, cur); return nullptr; }
    return &it->second;
  }
  int round(const uint64_t* present, uint32_t n, uint32_t words, uint8_t* out_kept, demi_wildcard_round_result* r) {
    memset(r, 0, sizeof *r);
    r->first_hit = 0xFFFFFFFFu;
    r->launches = 1;
    if (!selected) { fprintf(stderr, "round: no selectors loaded\n"); return DEMI_ERR_NO_TRACE; }
    if (words != (seg().trace.size() + 63) / 64) { fprintf(stderr, "round: rows of %u words\n", words); return DEMI_ERR_INVALID_ARG; }
    for (uint32_t i = 0; i < n; i++) {
      const Row* row = find(present + (size_t)i * words, "round");
      if (!row) return DEMI_ERR_INVALID_ARG;
      if (!row->reproduces) continue;
      r->first_hit = i; r->executed_len = row->executed_len; r->verdict.flags = DEMI_V_VIOLATION;
      for (size_t k = 0; k < seg().trace.size(); k++) { out_kept[k] = row->kept[k]; r->n_kept += row->kept[k] != 0; }
      break;
    }
    return DEMI_OK;
  }
  int get_trace(const uint64_t* present, std::vector<demi_rec_event>* out) {
    const Row* row = find(present, "get_trace");
    if (!row) return DEMI_ERR_INVALID_ARG;
    if (!row->reproduces || !row->has_trace) { fprintf(stderr, "get_trace: the mirror fetched no trace for this row of segment %zu\n", cur); return DEMI_ERR_INVALID_ARG; }
    *out = row->trace;
    return DEMI_OK;
  }
  int load(const demi_rec_event* trace, uint32_t n) {
    cur++;
    selected = false;
    if (cur >= segments.size() || seg().trace.size() != n || (n && memcmp(trace, seg().trace.data(), sizeof(demi_rec_event) * n))) {
      fprintf(stderr, "load: not the trace the mirror loaded for segment %zu\n", cur);
      return DEMI_ERR_INVALID_ARG;
    }
    return DEMI_OK;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Reader in{f};
  if (in.u32() != 0x314D4357u) { fprintf(stderr, "bad magic\n"); return 2; }
  demi_wcmin_params par;
  memset(&par, 0, sizeof par);
  par.clustering = in.u32(); par.policy = in.u32(); par.skip_clock_clusters = in.u32(); par.max_batch = in.u32();
  par.clock_increment_types = in.u32();
  const uint32_t n_msg_types = in.u32(), n_payloads = in.u32(), n_rec = in.u32();
  if (!in.ok || n_msg_types > DEMI_MAX_MSG_TYPES || n_payloads > DEMI_MAX_PAYLOADS || n_rec > DEMI_MAX_REC_EVENTS) { fprintf(stderr, "bad header\n"); return 2; }
  in.get(par.clock_field, DEMI_MAX_MSG_TYPES);
  std::vector<uint8_t> msg_class(n_msg_types);
  std::vector<demi_rec_event> rec(n_rec);
  in.get(msg_class.data(), msg_class.size());
  in.get(rec.data(), rec.size());
  RecordedRounds oracle;
  const uint32_t n_segments = in.u32();
  if (!in.ok || n_segments > 16) { fprintf(stderr, "bad segment count\n"); return 2; }
  oracle.segments.resize(n_segments);
  for (Segment& s : oracle.segments) {
    const uint32_t n = in.u32(), n_rows = in.u32();
    if (!in.ok || n > DEMI_MAX_REC_EVENTS || n_rows > (1u << 20)) { fprintf(stderr, "bad segment\n"); return 2; }
    s.trace.resize(n); s.type_sets.resize(n); s.policies.resize(n);
    in.get(s.trace.data(), n); in.get(s.type_sets.data(), n); in.get(s.policies.data(), n);
    for (uint32_t k = 0; k < n_rows; k++) {
      Row row;
      row.reproduces = in.u32() != 0; row.executed_len = in.u32(); row.has_trace = in.u32() != 0;
      if (!in.ok || row.executed_len > DEMI_MAX_REC_EVENTS) { fprintf(stderr, "bad row\n"); return 2; }
      std::vector<uint64_t> present((n + 63) / 64);
      in.get(present.data(), present.size());
      row.kept.resize(n);
      in.get(row.kept.data(), n);
      if (row.has_trace) { row.trace.resize(row.executed_len); in.get(row.trace.data(), row.trace.size()); }
      s.rows[present] = row;
    }
  }
  fclose(f);
  if (!in.ok) { fprintf(stderr, "short case file\n"); return 2; }
  if (oracle.segments.empty() || oracle.segments[0].trace.size() != n_rec ||
      (n_rec && memcmp(oracle.segments[0].trace.data(), rec.data(), sizeof(demi_rec_event) * n_rec))) {
    fprintf(stderr, "the first segment is not the loaded execution\n");
    return 2;
  }

  const demi_host::WcModel model{msg_class.data(), n_msg_types, n_payloads, par.clock_increment_types, par.clock_field};
  demi_host::WcminOutcome o;
  const int rc = demi_host::wildcard_minimize(rec.data(), n_rec, model, &par, oracle, &o);
  if (!rc && oracle.cur + 1 != oracle.segments.size()) {
    fprintf(stderr, "the mirror loaded %zu traces, the native loop %zu\n", oracle.segments.size(), oracle.cur + 1);
    return 3;
  }

  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  const uint32_t head[6] = {(uint32_t)rc, (uint32_t)o.trace.size(), (uint32_t)o.sizes.size(), (uint32_t)o.batches.size(),
                            o.stats.adoptions, o.stats.rounds};
  fwrite(head, sizeof head, 1, g);
  fwrite(&o.stats.total_replays, sizeof(uint64_t), 1, g);
  if (!o.trace.empty()) fwrite(o.trace.data(), sizeof(demi_rec_event), o.trace.size(), g);
  if (!o.sizes.empty()) fwrite(o.sizes.data(), sizeof(uint32_t), o.sizes.size(), g);
  if (!o.batches.empty()) fwrite(o.batches.data(), sizeof(uint32_t), o.batches.size(), g);
  fclose(g);
  return 0;
}
