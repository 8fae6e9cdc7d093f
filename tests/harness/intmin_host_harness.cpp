// intmin_host_harness.cpp — demi_amd/csrc/intmin_host.hpp (host-only code of the product) driven by the CPU oracle's removal
// replay instead of demi_replay_removal_round.  TEST INFRASTRUCTURE: a stand-alone program, built with the sanitizers by
// tests/test_intmin_host_cpu.py and run as a child process.
//
//   intmin_host_harness CASE OUT
// CASE (little endian): u32 magic 'IMH1', strategy, max_batch, looking_for, n_ext, n_rec, then the demi_model scalars n_actors,
//   n_msg_types, n_classes, code_len, inv_kind, inv_fa, inv_va, inv_fb, fp_match_mask, flags, n_init (words of init_state); then
//   msg_class [n_msg_types] u8, actor_class [n_actors] u8, handler_start [n_classes * n_msg_types] u16, code [code_len] u32,
//   init_state [n_init] u64, externals [n_ext] demi_ext_event, recorded events [n_rec] demi_rec_event.
// OUT: u32 status, n_trace, n_sizes, n_batches, unignorable, adoptions, u64 total_replays; then the trace (demi_rec_event),
//   the sizes (u32), the batches (u32).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../demi_amd/csrc/intmin_host.hpp"
#include "../../oracle/demi_oracle.h"

namespace {

struct Reader {
  FILE* f;
  bool ok = true;
  template <class T> void get(T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) ok = false; }
  uint32_t u32() { uint32_t x = 0; get(&x, 1); return x; }
};

// a round answered one replay at a time, in proposal order, as the sequential loop asks
struct OracleRounds {
  const demi_model* model;
  const std::vector<demi_ext_event>* ext;
  std::vector<demi_rec_event> loaded;
  demi_limits lim;
  int round(const uint32_t* skip, uint32_t n, uint8_t* out_kept, demi_removal_round_result* r) {
    memset(r, 0, sizeof *r);
    r->first_hit = 0xFFFFFFFFu;
    r->launches = 1;
    std::vector<uint8_t> kept(loaded.size() + 1);
    for (uint32_t i = 0; i < n; i++) {
      demi_verdict v;
      memset(&v, 0, sizeof v);
      std::fill(kept.begin(), kept.end(), 0);
      const int rc = orc_sts_removal(model, ext->data(), (uint32_t)ext->size(), loaded.data(), (uint32_t)loaded.size(), nullptr, skip[i],
                                     &lim, &v, kept.data());
      if (rc) return rc;
      if (v.flags & (DEMI_V_PENDING_OVF | DEMI_V_QUEUE_OVF)) return DEMI_ERR_CAPACITY;
      if (v.flags & DEMI_V_VIOLATION) {
        r->first_hit = i; r->verdict = v;
        for (size_t k = 0; k < loaded.size(); k++) { out_kept[k] = kept[k]; r->n_kept += kept[k] != 0; }
        break;
      }
    }
    return DEMI_OK;
  }
  int load(const demi_rec_event* trace, uint32_t n) { loaded.assign(trace, trace + n); return DEMI_OK; }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Reader in{f};
  if (in.u32() != 0x31484D49u) { fprintf(stderr, "bad magic\n"); return 2; }
  demi_intmin_params par;
  par.strategy = in.u32(); par.max_batch = in.u32();
  const uint32_t looking_for = in.u32(), n_ext = in.u32(), n_rec = in.u32();
  demi_model m;
  memset(&m, 0, sizeof m);
  m.n_actors = in.u32(); m.n_msg_types = in.u32(); m.n_classes = in.u32(); m.code_len = in.u32();
  m.inv_kind = in.u32(); m.inv_fa = in.u32(); m.inv_va = in.u32(); m.inv_fb = in.u32(); m.fp_match_mask = in.u32(); m.flags = in.u32();
  const uint32_t n_init = in.u32();
  if (!in.ok || m.n_actors > DEMI_MAX_ACTORS_BIG || m.n_msg_types > DEMI_MAX_MSG_TYPES || m.n_classes > DEMI_MAX_CLASSES ||
      m.code_len > DEMI_MAX_CODE || n_init > 2 * DEMI_MAX_ACTORS_BIG || n_ext > DEMI_MAX_EXT_EVENTS || n_rec > DEMI_MAX_REC_EVENTS) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<uint8_t> msg_class(m.n_msg_types), actor_class(m.n_actors);
  std::vector<uint16_t> handler_start((size_t)m.n_classes * m.n_msg_types);
  std::vector<uint32_t> code(m.code_len);
  std::vector<uint64_t> init_state(n_init);
  std::vector<demi_ext_event> ext(n_ext);
  std::vector<demi_rec_event> rec(n_rec);
  in.get(msg_class.data(), msg_class.size()); in.get(actor_class.data(), actor_class.size());
  in.get(handler_start.data(), handler_start.size()); in.get(code.data(), code.size()); in.get(init_state.data(), init_state.size());
  in.get(ext.data(), ext.size()); in.get(rec.data(), rec.size());
  fclose(f);
  if (!in.ok) { fprintf(stderr, "short case file\n"); return 2; }
  m.msg_class = msg_class.data(); m.actor_class = actor_class.data(); m.handler_start = handler_start.data();
  m.code = code.data(); m.init_state = init_state.data();

  OracleRounds oracle;
  oracle.model = &m; oracle.ext = &ext; oracle.loaded = rec;
  memset(&oracle.lim, 0, sizeof oracle.lim);
  oracle.lim.p_max = 64; oracle.lim.looking_for_valid = 1; oracle.lim.looking_for = looking_for;
  demi_host::IntminOutcome o;
  const int rc = demi_host::sts_sched_minimize(rec.data(), n_rec, msg_class.data(), m.n_msg_types,
                                               m.n_actors > DEMI_MAX_ACTORS ? DEMI_DEADLETTERS_BIG : DEMI_DEADLETTERS, &par, oracle, &o);
  // the minimized execution is what the oracle holds loaded at the end
  if (!rc && (o.trace.size() != oracle.loaded.size() ||
              (!o.trace.empty() && memcmp(o.trace.data(), oracle.loaded.data(), sizeof(demi_rec_event) * o.trace.size())))) {
    fprintf(stderr, "the loaded execution is not the result\n");
    return 3;
  }

  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  const uint32_t head[6] = {(uint32_t)rc, (uint32_t)o.trace.size(), (uint32_t)o.sizes.size(), (uint32_t)o.batches.size(),
                            o.stats.unignorable, o.stats.adoptions};
  fwrite(head, sizeof head, 1, g);
  fwrite(&o.stats.total_replays, sizeof(uint64_t), 1, g);
  if (!o.trace.empty()) fwrite(o.trace.data(), sizeof(demi_rec_event), o.trace.size(), g);
  if (!o.sizes.empty()) fwrite(o.sizes.data(), sizeof(uint32_t), o.sizes.size(), g);
  if (!o.batches.empty()) fwrite(o.batches.data(), sizeof(uint32_t), o.batches.size(), g);
  fclose(g);
  return 0;
}
