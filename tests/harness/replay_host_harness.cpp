// Stand-alone driver of demi_amd/csrc/replay_host.hpp (TEST INFRASTRUCTURE): the capacity rule over a batch and the first-hit
// round, answered from scripts instead of replays.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_replay_host_cpu.py; exits non-zero at the first expectation that does not hold.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../demi_amd/csrc/replay_host.hpp"

using namespace demi_host;

static int g_cases = 0;
static demi_limits limits(uint32_t p_max) {
  demi_limits l = {};
  l.p_max = p_max;
  l.looking_for = 0x1234;      // (must reach the callables unchanged)
  return l;
}
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

// ----------------------------------------------------------------------------- the round
// a proposal's answer at the caller's capacity and at the largest: '.' does not reproduce, 'H' reproduces, 'O' aborts
struct Call { uint32_t off, count, p_max; };
struct Result { uint32_t launches = 0, retried = 0, first_hit = kNone; };
struct Round {
  std::string small, big;
  std::vector<Call> calls;
  Result r;
  uint32_t failed = 0;
  int run(uint32_t per, uint32_t p_max) {
    const uint32_t n = (uint32_t)small.size();
    return first_hit_round(n, per, limits(p_max), [&](uint32_t off, uint32_t count, const demi_limits& l, RoundAnswer* a) {
      CHECK(count >= 1 && off + count <= n && l.looking_for == 0x1234);
      calls.push_back({off, count, l.p_max});
      const std::string& s = p_max_is_largest(l.p_max) ? big : small;
      for (uint32_t i = 0; i < count; i++) {
        if (s[off + i] == 'H' && a->first_hit == kNone) a->first_hit = i;
        if (s[off + i] == 'O' && a->first_ovf == kNone) a->first_ovf = i;
      }
      return DEMI_OK;
    }, &r, &failed);
  }
};

static void round_cases() {
  {  // n = 0: nothing is launched
    Round t{"", ""};
    CHECK(t.run(4, 8) == DEMI_OK && t.calls.empty() && t.r.launches == 0 && t.r.retried == 0 && t.r.first_hit == kNone);
    g_cases++;
  }
  {  // width 1: a launch per proposal, up to the hit
    Round t{"..H.", "..H."};
    CHECK(t.run(1, 8) == DEMI_OK && t.r.first_hit == 2 && t.r.launches == 3 && t.r.retried == 0 && t.calls.size() == 3);
    CHECK(t.calls[2].off == 2 && t.calls[2].count == 1 && t.calls[2].p_max == 8);
    g_cases++;
  }
  {  // a hit in the first chunk: the round stops there
    Round t{".H...H..", ".H...H.."};
    CHECK(t.run(3, 0) == DEMI_OK && t.r.first_hit == 1 && t.r.launches == 1 && t.r.retried == 0);
    g_cases++;
  }
  {  // a hit in the last (short) chunk
    Round t{"......H", "......H"};
    CHECK(t.run(3, 8) == DEMI_OK && t.r.first_hit == 6 && t.r.launches == 3 && t.r.retried == 0);
    CHECK(t.calls[2].off == 6 && t.calls[2].count == 1);
    g_cases++;
  }
  {  // no hit at all
    Round t{".....", "....."};
    CHECK(t.run(2, 8) == DEMI_OK && t.r.first_hit == kNone && t.r.launches == 3 && t.r.retried == 0);
    g_cases++;
  }
  {  // an abort after the hit: the sequential loop never gets there, no retry
    Round t{"..HO", "..H."};
    CHECK(t.run(4, 8) == DEMI_OK && t.r.first_hit == 2 && t.r.launches == 1 && t.r.retried == 0);
    g_cases++;
  }
  {  // an abort before the hit: first_hit + 1 proposals once more, at the largest capacity; the aborted one turns out to be the hit
    Round t{"...O.H.", "...H.H."};
    CHECK(t.run(7, 8) == DEMI_OK && t.r.first_hit == 3 && t.r.launches == 2 && t.r.retried == 6);
    CHECK(t.calls[1].off == 0 && t.calls[1].count == 6 && t.calls[1].p_max == DEMI_MAX_PENDING);
    g_cases++;
  }
  {  // the same in a later chunk, the aborted proposal failing: retry of first_hit + 1 = 2 of the chunk's proposals
    Round t{"....OH..", ".....H.."};
    CHECK(t.run(4, 0) == DEMI_OK && t.r.first_hit == 5 && t.r.launches == 3 && t.r.retried == 2);
    CHECK(t.calls[2].off == 4 && t.calls[2].count == 2 && t.calls[2].p_max == DEMI_MAX_PENDING);
    g_cases++;
  }
  {  // an abort without a hit: the whole chunk once more, then the round goes on at the caller's capacity
    Round t{".O...H", ".....H"};
    CHECK(t.run(3, 8) == DEMI_OK && t.r.first_hit == 5 && t.r.launches == 3 && t.r.retried == 3);
    CHECK(t.calls[1].off == 0 && t.calls[1].count == 3 && t.calls[1].p_max == DEMI_MAX_PENDING);
    CHECK(t.calls[2].off == 3 && t.calls[2].count == 3 && t.calls[2].p_max == 8);
    g_cases++;
  }
  {  // still aborted after the retry: an error that names the proposal by its index in the round
    Round t{"....O.H", "....O.H"};
    CHECK(t.run(3, 8) == DEMI_ERR_CAPACITY && t.failed == 4 && t.r.launches == 3 && t.r.retried == 3 && t.r.first_hit == kNone);
    g_cases++;
  }
  {  // the capacity is already the largest: an error at once, after one launch
    Round t{".O.H", ".O.H"};
    CHECK(t.run(4, DEMI_MAX_PENDING) == DEMI_ERR_CAPACITY && t.failed == 1 && t.calls.size() == 1 && t.r.launches == 1 && t.r.retried == 0);
    g_cases++;
  }
  {  // a launch's own error ends the round as it is, and names no proposal
    Result r;
    uint32_t failed = 0;
    CHECK(first_hit_round(5, 2, limits(8), [](uint32_t off, uint32_t, const demi_limits&, RoundAnswer*) { return off ? DEMI_ERR_DEVICE : DEMI_OK; }, &r, &failed) == DEMI_ERR_DEVICE);
    CHECK(failed == kNone && r.launches == 1);
    g_cases++;
  }
}

// ----------------------------------------------------------------------------- the batch
// an item's answer at the caller's capacity and at the largest: a number, negative = undecided
struct Batch {
  std::vector<int> small, big;
  std::vector<std::vector<uint32_t>> asked;
  std::vector<uint32_t> asked_p;
  std::vector<bool> asked_all;
  std::vector<int> answers;
  BatchOutcome o;
  int run(uint32_t p_max) {
    answers.assign(small.size(), 0);
    return decide_batch((uint32_t)small.size(), limits(p_max), answers.data(), [&](const uint32_t* idx, uint32_t m, const demi_limits& l, int* out) {
      CHECK(l.looking_for == 0x1234 && (idx || m == small.size()));      // (no index list: every item)
      asked.emplace_back();
      for (uint32_t k = 0; k < m; k++) asked.back().push_back(idx ? idx[k] : k);
      asked_all.push_back(idx == nullptr);
      asked_p.push_back(l.p_max);
      for (uint32_t k = 0; k < m; k++) out[k] = (p_max_is_largest(l.p_max) ? big : small)[asked.back()[k]];
      return DEMI_OK;
    }, [](int a) { return a < 0; }, &o);
  }
};

static void batch_cases() {
  {  // nothing undecided: one evaluation of every item
    Batch t{{1, 2, 3}, {7, 7, 7}};
    CHECK(t.run(8) == DEMI_OK && t.asked.size() == 1 && t.asked_all[0] && t.asked[0] == std::vector<uint32_t>({0, 1, 2}) && t.asked_p[0] == 8);
    CHECK(t.answers == std::vector<int>({1, 2, 3}) && t.o.retried == 0 && t.o.undecided == 0);
    g_cases++;
  }
  {  // some undecided: exactly those, in order, at the largest capacity; their answers scattered back
    Batch t{{1, -1, 3, -1, 5}, {10, 20, 30, 40, 50}};
    CHECK(t.run(0) == DEMI_OK && t.asked.size() == 2 && t.asked_all[0] && !t.asked_all[1] && t.asked[1] == std::vector<uint32_t>({1, 3}));
    CHECK(t.asked_p[0] == 0 && t.asked_p[1] == DEMI_MAX_PENDING);
    CHECK(t.answers == std::vector<int>({1, 20, 3, 40, 5}) && t.o.retried == 2 && t.o.undecided == 0);
    g_cases++;
  }
  {  // still undecided after the retry: an error, and how many
    Batch t{{-1, 2, -1}, {-1, 20, 30}};
    CHECK(t.run(8) == DEMI_ERR_CAPACITY && t.asked.size() == 2 && t.o.retried == 2 && t.o.undecided == 1);
    g_cases++;
  }
  {  // the capacity is already the largest: an error after one evaluation
    Batch t{{1, -1}, {1, -1}};
    CHECK(t.run(DEMI_MAX_PENDING) == DEMI_ERR_CAPACITY && t.asked.size() == 1 && t.o.retried == 0 && t.o.undecided == 1);
    g_cases++;
  }
  {  // an empty batch
    Batch t{{}, {}};
    CHECK(t.run(8) == DEMI_OK && t.o.retried == 0 && t.o.undecided == 0);
    g_cases++;
  }
  {  // the evaluation's own error is returned as it is, and blames no item
    int a[2] = {0, 0};
    BatchOutcome o;
    int calls = 0;
    CHECK(decide_batch(2u, limits(8), a, [&](const uint32_t*, uint32_t, const demi_limits&, int* out) { out[0] = out[1] = -1; return calls++ ? DEMI_ERR_DEVICE : DEMI_OK; },
                       [](int v) { return v < 0; }, &o) == DEMI_ERR_DEVICE);
    CHECK(calls == 2 && o.undecided == 0 && o.retried == 0);
    g_cases++;
  }
  {  // one item: run again once, and the answer is the second one; an error of the second run is the callable's, not the rule's
    Batch t{{-1}, {9}};
    CHECK(t.run(8) == DEMI_OK && t.answers[0] == 9 && t.asked.size() == 2 && t.o.retried == 1);
    int a = 0, runs = 0;
    BatchOutcome o;
    CHECK(decide_batch(1u, limits(8), &a, [&](const uint32_t*, uint32_t, const demi_limits&, int* out) { *out = -1; return runs++ ? DEMI_ERR_CAPACITY : DEMI_OK; },
                       [](int v) { return v < 0; }, &o) == DEMI_ERR_CAPACITY);
    CHECK(runs == 2 && o.undecided == 0);
    g_cases++;
  }
  // the default and the ceiling
  CHECK(p_max_of(0) == 64 && p_max_of(5) == 5 && !p_max_is_largest(0) && !p_max_is_largest(DEMI_MAX_PENDING - 1) && p_max_is_largest(DEMI_MAX_PENDING) && at_largest(limits(3)).p_max == DEMI_MAX_PENDING);
  g_cases++;
}

int main() {
  round_cases();
  batch_cases();
  printf("replay_host: %d cases ok\n", g_cases);
  return 0;
}
