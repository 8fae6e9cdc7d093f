// fuzz_pipeline_harness.cpp — demi_amd/csrc/fuzz_pipeline_host.hpp driven by scripted launch outcomes, no GPU and no emulator
// (tests/test_fuzz_pipeline_cpu.py builds it with -fsanitize=address,undefined and runs it as a child process).
// A script: n launches, in_flight, the launch that holds the hit (or none), a launch whose submit fails (or none), a launch whose
// wait fails (or none).  Checked after every run: every submitted launch got exactly one wait or drain before the driver returned,
// launches are submitted and waited for in order, never more than in_flight are outstanding, and the counts are the expected ones.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../demi_amd/csrc/fuzz_pipeline_host.hpp"

namespace {
constexpr uint32_t kNone = 0xFFFFFFFFu;
int g_cases = 0;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); std::exit(1); } \
  } while (0)

struct Script { uint32_t n, in_flight, hit_at, submit_fails_at, wait_fails_at; };

void run(const Script& s) {
  std::vector<int> submitted(s.n, 0), waited(s.n, 0), drained(s.n, 0);
  uint32_t outstanding = 0, max_outstanding = 0, next_submit = 0, next_finish = 0;
  demi_host::FuzzPipelineCounts c;
  const int rc = demi_host::run_fuzz_pipeline(
      s.n, s.in_flight,
      [&](uint32_t k) {
        CHECK(k < s.n && k == next_submit);                 // in order, each once
        if (k == s.submit_fails_at) return -6;
        next_submit++;
        submitted[k]++;
        outstanding++;
        if (outstanding > max_outstanding) max_outstanding = outstanding;
        return 0;
      },
      [&](uint32_t k, bool* hit) {
        CHECK(k == next_finish && submitted[k] == 1 && !waited[k] && !drained[k]);      // the oldest outstanding launch
        next_finish++;
        waited[k]++;
        outstanding--;
        if (k == s.wait_fails_at) return -7;
        *hit = k == s.hit_at;
        return 0;
      },
      [&](uint32_t k) {
        CHECK(k == next_finish && submitted[k] == 1 && !waited[k] && !drained[k]);
        next_finish++;
        drained[k]++;
        outstanding--;
      },
      &c);
  const uint32_t eff = s.in_flight ? s.in_flight : 1u;
  // every submitted launch was waited for exactly once before the return, nothing else was
  CHECK(outstanding == 0);
  for (uint32_t k = 0; k < s.n; k++) CHECK(waited[k] + drained[k] == submitted[k]);
  CHECK(max_outstanding <= eff);
  // what the sequential campaign would have done decides the answer: it ends at the first of hit / failing wait / failing submit
  // it reaches.  A launch is reached by wait k only after submit min(k + eff, n) - 1 .. have been made.
  uint32_t end = s.n;                  // the first launch whose wait ends the campaign
  if (s.hit_at < end) end = s.hit_at;
  if (s.wait_fails_at < end) end = s.wait_fails_at;
  const bool submit_first = s.submit_fails_at != kNone && s.submit_fails_at < s.n && (end == s.n || s.submit_fails_at < end + eff);
  if (submit_first) {
    CHECK(rc == -6);
    // the waits before the failing submit was attempted: launches 0 .. submit_fails_at - eff
    const uint32_t before = s.submit_fails_at >= eff ? s.submit_fails_at - eff + 1 : 0;
    CHECK(c.submitted == s.submit_fails_at && c.committed == before && c.discarded == c.submitted - before && !c.hit);
  } else if (end == s.n) {
    CHECK(rc == 0 && !c.hit && c.submitted == s.n && c.committed == s.n && c.discarded == 0);
  } else {
    const uint32_t ahead = (end + eff < s.n ? end + eff : s.n);      // launches submitted when wait(end) is made
    CHECK(c.submitted == ahead);
    if (end == s.wait_fails_at) {
      CHECK(rc == -7 && !c.hit && c.committed == end && c.discarded == ahead - end - 1);
    } else {
      CHECK(rc == 0 && c.hit && c.committed == end + 1 && c.discarded == ahead - end - 1);
      CHECK(c.submitted - c.discarded == c.committed && c.discarded <= eff - 1);
    }
  }
  if (eff == 1) CHECK(c.discarded == 0);
  g_cases++;
}
}  // namespace

int main() {
  for (uint32_t in_flight = 1; in_flight <= 3; in_flight++) {
    run({5, in_flight, kNone, kNone, kNone});                                   // no hit: every launch committed
    for (uint32_t L = 0; L < 5; L++) run({5, in_flight, L, kNone, kNone});      // the hit at launch L
    for (uint32_t L = 0; L < 5; L++) run({5, in_flight, kNone, L, kNone});      // an error at submit L
    for (uint32_t L = 0; L < 5; L++) run({5, in_flight, kNone, kNone, L});      // an error at wait L
    for (uint32_t L = 0; L < 5; L++)
      for (uint32_t E = 0; E < 5; E++) {
        run({5, in_flight, L, E, kNone});                                       // a hit and a failing submit: whichever is reached first
        run({5, in_flight, L, kNone, E});
      }
    run({1, in_flight, 0, kNone, kNone});
    run({1, in_flight, kNone, kNone, kNone});
    run({0, in_flight, kNone, kNone, kNone});                                   // nothing to do
  }
  run({5, 0, 2, kNone, kNone});                                                 // in_flight 0 is taken as 1 by the driver itself
  std::printf("fuzz_pipeline_host: %d cases ok\n", g_cases);
  return 0;
}
