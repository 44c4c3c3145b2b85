// tests/test_staging_ring_host.py: csrc/staging_ring.h as a stand-alone program built with the thread sanitizer.  Every
// scenario checks that no item is staged before its buffer's previous user (item i - depth) was consumed, that every item
// the caller waited for was staged exactly once, and that the run ends; prints one "ok <scenario>" line each.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

#include "staging_ring.h"

using rgbdfe::StagingRing;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static void nap(int us) { if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us)); }

struct Run {
  int n, depth;
  std::vector<int> staged_times;       // how often item i was staged
  std::vector<int> consumed_at_stage;  // items consumed when item i's staging began
  std::vector<int> buffer;             // the ring's buffers: which item each holds
  std::atomic<int> consumed{0};
  Run(int n_, int depth_) : n(n_), depth(depth_), staged_times((size_t)n_, 0), consumed_at_stage((size_t)n_, -1), buffer((size_t)depth_, -1) {}
};

// consume_upto items are waited for, read and consumed; then the caller leaves -- by an exception when `throws`
static void pipeline(Run& r, int stage_us, int consume_us, int consume_upto, bool throws) {
  try {
    StagingRing ring(r.n, r.depth, [&](int i) {
      r.consumed_at_stage[(size_t)i] = r.consumed.load();
      nap(stage_us);
      r.buffer[(size_t)(i % r.depth)] = i;   // (a data race here is the sanitizer's to report: the ring's rule forbids it)
      r.staged_times[(size_t)i]++;
    });
    for (int i = 0; i < consume_upto; ++i) {
      ring.wait_staged(i);
      CHECK(r.buffer[(size_t)(i % r.depth)] == i);   // not overwritten by item i + depth
      nap(consume_us);
      r.consumed.store(i + 1);
      ring.mark_consumed(i);
    }
    if (throws) throw std::runtime_error("on the way to the ABI barrier");
    ring.stop();
    ring.stop();   // the destructor stops again: harmless
  } catch (const std::runtime_error&) {
  }
  // the helper has been joined: its writes are visible
  for (int i = 0; i < r.n; ++i) {
    if (i < consume_upto) CHECK(r.staged_times[(size_t)i] == 1);
    else CHECK(r.staged_times[(size_t)i] <= 1);
    if (r.staged_times[(size_t)i]) CHECK(r.consumed_at_stage[(size_t)i] >= i - r.depth + 1);
    if (i >= consume_upto + r.depth) CHECK(r.staged_times[(size_t)i] == 0);   // its buffer was never released
  }
}

int main() {
  { Run r(12, 3); pipeline(r, 0, 200, 12, false); printf("ok slow consumer\n"); }
  { Run r(12, 3); pipeline(r, 200, 0, 12, false); printf("ok slow stager\n"); }
  { Run r(10, 2); pipeline(r, 0, 0, 1, true); printf("ok destroyed with the helper blocked\n"); }
  { Run r(10, 2); pipeline(r, 300, 0, 0, true); printf("ok destroyed while staging\n"); }
  { Run r(1, 2); pipeline(r, 0, 0, 1, false); printf("ok one item\n"); }
  { Run r(0, 4); pipeline(r, 0, 0, 0, false); printf("ok no item, no thread\n"); }
  { Run r(5, 8); pipeline(r, 0, 50, 5, false); printf("ok fewer items than buffers\n"); }
  return failures ? 1 : 0;
}
