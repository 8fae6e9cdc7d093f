// fuzz_pipeline_host.hpp — the bookkeeping of a fuzz campaign whose launches are in flight (demi_fuzz_campaign_pipelined, DESIGN.md
// section 0.16): which launch is committed, which launches are discarded, and what is waited for when something fails.
// Host control only, and no HIP: what a launch IS is the callables' business (the library: generate, explore and reduce on a stream
// of the context; the harness tests/harness/fuzz_pipeline_harness.cpp: scripted outcomes).
//
// A campaign is launches 0 .. n_launches - 1 in order; it ends at the first launch that holds a violating test.  Up to `in_flight`
// launches are submitted ahead of the one whose answer is read, so the launches behind the one that ends the campaign were
// speculated: they are waited for, nothing is read from them, and they are counted as discarded.
//   int submit(uint32_t k)             puts launch k on the device.  A submit that fails has itself waited for whatever it started;
//                                      launch k then does not count as submitted.
//   int wait(uint32_t k, bool* hit)    blocks until launch k is done and reads its answer: *hit = it holds a violating test.  Called
//                                      for the oldest outstanding launch only.  A wait that fails has still waited.
//   void drain(uint32_t k)             blocks until launch k is done and reads nothing.  It cannot fail: it is what an exit path does.
// Every submitted launch gets exactly one wait or one drain before run_fuzz_pipeline returns, whatever it returns.  A callable's
// non-zero status ends the campaign and is returned as it is.
#pragma once

#include <cstdint>

namespace demi_host {

struct FuzzPipelineCounts {
  uint32_t submitted = 0;      // launches put on the device
  uint32_t committed = 0;      // launches whose answer was read, the one that holds the hit included
  uint32_t discarded = 0;      // launches drained unread
  bool hit = false;            // the last committed launch holds a violating test
};

template <class Submit, class Wait, class Drain>
int run_fuzz_pipeline(uint32_t n_launches, uint32_t in_flight, Submit&& submit, Wait&& wait, Drain&& drain, FuzzPipelineCounts* c) {
  *c = FuzzPipelineCounts();
  if (in_flight < 1) in_flight = 1;
  uint32_t head = 0, next = 0;      // the oldest outstanding launch; the next one to submit: head <= next <= head + in_flight
  int rc = 0;
  while (head < n_launches && rc == 0 && !c->hit) {
    while (rc == 0 && next < n_launches && next - head < in_flight) {
      rc = submit(next);
      if (rc == 0) { next++; c->submitted++; }
    }
    if (rc) break;
    bool hit = false;
    rc = wait(head, &hit);
    head++;
    if (rc) break;
    c->committed++;
    c->hit = hit;
  }
  for (; head < next; head++) { drain(head); c->discarded++; }
  return rc;
}

}  // namespace demi_host
