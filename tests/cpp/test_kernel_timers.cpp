// The kernel timing table (simple_pbft_amd/csrc/host/kernel_timers.h) on the
// host alone: counting fake events, scripted failures of each operation, and
// after EVERY step the conservation rule -- each event ever created was
// destroyed exactly once or is in a pending pair -- and sums and counts equal
// to what the script computed by hand.  Built with -fsanitize=address,undefined
// by tests/test_kernel_timers.py.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "kernel_timers.h"

namespace {

int g_checks = 0, g_failed = 0;

#define CHECK(cond, ...)                                           \
  do {                                                             \
    ++g_checks;                                                    \
    if (!(cond)) {                                                 \
      ++g_failed;                                                  \
      if (g_failed <= 20) {                                        \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                                  \
        std::printf("\n");                                         \
      }                                                            \
    }                                                              \
  } while (0)

constexpr int kSlots = 11;  // as Device::timers: ids 0..5, DER, four sign stages
struct World;
World* g_world = nullptr;  // the one the fake event operations book into
struct Ops {
  static int create(int* e);
  static int destroy(int e);
  static int record(int e, int st);
  static int synchronize(int e);
  static int elapsed(float* ms, int a, int b);
};
using Timers = pbftv::KernelTimers<int, kSlots, Ops>;

// One table under test with its books.  Events are 1, 2, 3, ... in creation
// order; an error is any nonzero int.
struct World {
  Timers t;
  int created = 0, launches_run = 0;
  std::map<int, int> destroyed;       // event -> times destroyed
  std::map<int, float> ms_of;         // start event -> what elapsed answers for its pair
  std::vector<std::string> log;       // "rec <ev> <stream>" / "launch"
  int fail_create_at = 0;             // the k-th create from now fails (1-based; 0: none)
  int fail_sync_of = 0, fail_elapsed_of = 0;  // stop event whose synchronize / elapsed fails
  double want_ms[kSlots] = {};        // by hand: what the table must hold
  unsigned long long want_n[kSlots] = {};
  size_t want_pending[kSlots] = {};

  World() { g_world = this; }

  // one launch of `ms` milliseconds (a multiple of 0.25: the sums are exact) that returns `ret`
  int launch(bool on, int slot, int stream, float ms, int ret = 0) {
    const int before = created;
    const size_t log0 = log.size();
    const int rc = t.timed(on, slot, stream, [&] {
      ++launches_run;
      log.push_back("launch");
      return ret;
    });
    if (created == before + 2) {  // a pair was made: start, launch, stop, in that order, and it is pending
      ms_of[before + 1] = ms;
      ++want_pending[slot];
      CHECK(log.size() == log0 + 3 && log[log0] == "rec " + std::to_string(before + 1) + " " + std::to_string(stream) &&
                log[log0 + 1] == "launch" && log[log0 + 2] == "rec " + std::to_string(before + 2) + " " + std::to_string(stream),
            "slot %d: events not recorded around the launch", slot);
    }
    return rc;
  }

  // collect; `stop_at`: the stop event whose failure ends it (0: none)
  int collect(int stop_at = 0) {
    // by hand: pairs leave in slot order, then in launch order, until the failing one
    std::vector<std::pair<int, int>> order;  // (slot, start event)
    for (int k = 0; k < kSlots; ++k)
      for (int a : pending_of[k]) order.push_back({k, a});
    bool stopped = false;
    for (auto& pr : order) {
      if (pr.second + 1 == stop_at) stopped = true;
      if (stopped) continue;
      want_ms[pr.first] += ms_of[pr.second];
      want_n[pr.first] += 1;
      --want_pending[pr.first];
      auto& v = pending_of[pr.first];
      v.erase(v.begin());
    }
    return t.collect();
  }
  std::vector<int> pending_of[kSlots];  // start events the script expects pending, per slot

  void check(const char* what) {
    size_t pend = 0;
    for (int k = 0; k < kSlots; ++k) {
      CHECK(t.ms(k) == want_ms[k], "%s: slot %d holds %f ms, by hand %f", what, k, t.ms(k), want_ms[k]);
      CHECK(t.launches(k) == want_n[k], "%s: slot %d counts %llu, by hand %llu", what, k,
            (unsigned long long)t.launches(k), want_n[k]);
      CHECK(t.pending(k) == want_pending[k], "%s: slot %d has %zu pending, by hand %zu", what, k, t.pending(k),
            want_pending[k]);
      pend += t.pending(k);
    }
    size_t gone = 0;
    for (auto& kv : destroyed) {
      CHECK(kv.second == 1, "%s: event %d destroyed %d times", what, kv.first, kv.second);
      CHECK(kv.first >= 1 && kv.first <= created, "%s: event %d destroyed but never created", what, kv.first);
      ++gone;
    }
    CHECK(gone + 2 * pend == (size_t)created, "%s: %d created, %zu destroyed, %zu pairs pending", what, created, gone,
          pend);
  }

  // a timed launch that is expected to leave a pair
  void good(int slot, int stream, float ms, int ret = 0) {
    const int a = created + 1;
    CHECK(launch(true, slot, stream, ms, ret) == ret, "slot %d: wrong return value", slot);
    pending_of[slot].push_back(a);
  }
};

int Ops::create(int* e) {
  World* w = g_world;
  if (w->fail_create_at && --w->fail_create_at == 0) return 7;
  *e = ++w->created;
  return 0;
}
int Ops::destroy(int e) {
  ++g_world->destroyed[e];
  return 0;
}
int Ops::record(int e, int st) {
  g_world->log.push_back("rec " + std::to_string(e) + " " + std::to_string(st));
  return 0;
}
int Ops::synchronize(int e) { return e == g_world->fail_sync_of ? 8 : 0; }
int Ops::elapsed(float* ms, int a, int b) {
  World* w = g_world;
  if (b == w->fail_elapsed_of) return 9;
  CHECK(b == a + 1 && w->ms_of.count(a), "elapsed over (%d, %d): not one launch's pair", a, b);
  *ms = w->ms_of[a];
  return 0;
}

void timing_off() {
  World w;
  for (int k = 0; k < kSlots; ++k) CHECK(w.launch(false, k, 3, 1.0f) == 0, "off: launch failed");
  CHECK(w.launch(false, 2, 3, 1.0f, 5) == 5, "off: the launch's error was not returned");
  CHECK(w.created == 0 && w.log.size() == (size_t)w.launches_run && w.launches_run == kSlots + 1,
        "off: %d events created, %d launches", w.created, w.launches_run);
  w.check("timing off");
  CHECK(w.collect() == 0, "off: collect failed");
  w.check("timing off, collected");
}

void several_slots_collect_reset() {
  World w;
  // slot k gets k % 3 + 1 launches of (k + 1) * 0.25 ms each, interleaved over streams
  for (int round = 0; round < 3; ++round)
    for (int k = 0; k < kSlots; ++k)
      if (round <= k % 3) w.good(k, 10 + round, (float)(k + 1) * 0.25f);
  w.check("launched");
  CHECK(w.collect() == 0, "collect failed");
  w.check("collected");
  for (int k = 0; k < kSlots; ++k)
    CHECK(w.want_n[k] == (unsigned long long)(k % 3 + 1) && w.want_ms[k] == (k % 3 + 1) * (k + 1) * 0.25,
          "the script's own books are off at slot %d", k);
  CHECK(w.collect() == 0, "second collect failed");
  w.check("collected twice");
  // more launches, then a reset without collecting: sums go, pending pairs stay and count afterwards
  w.good(6, 1, 2.0f);
  w.good(7, 1, 0.5f);
  w.t.reset();
  for (int k = 0; k < kSlots; ++k) w.want_ms[k] = 0, w.want_n[k] = 0;
  w.check("reset");
  CHECK(w.collect() == 0, "collect after reset failed");
  w.check("collected after reset");
  CHECK(w.t.ms(6) == 2.0 && w.t.launches(7) == 1, "launches pending over a reset were lost");
}

void drop_at_close() {
  World w;
  w.good(0, 1, 1.0f);
  w.good(6, 2, 1.0f);
  w.good(6, 2, 1.0f);
  for (int s = 7; s < kSlots; ++s) w.good(s, 3, 0.25f);
  w.check("before close");
  w.t.drop();
  for (int k = 0; k < kSlots; ++k) w.want_pending[k] = 0, w.pending_of[k].clear();
  w.check("dropped");
  CHECK((int)w.destroyed.size() == w.created && w.created == 14, "drop left events behind");
  w.t.drop();
  w.check("dropped twice");
}

void create_fails() {
  for (int at = 1; at <= 2; ++at) {
    World w;
    w.good(4, 1, 0.5f);
    w.fail_create_at = at;
    const int runs = w.launches_run;
    CHECK(w.launch(true, 4, 1, 0.5f) == 7, "create %d failing: its error was not returned", at);
    CHECK(w.launches_run == runs, "create %d failing: the launch ran", at);
    CHECK(w.created == 2 + (at - 1) && (int)w.destroyed.size() == at - 1,
          "create %d failing: %d created, %zu destroyed", at, w.created, w.destroyed.size());
    w.check("a create failed");
    w.good(4, 1, 0.5f);  // and the table goes on working
    CHECK(w.collect() == 0, "collect failed");
    w.check("a create failed, collected");
  }
}

void launch_fails() {
  World w;
  w.good(1, 1, 0.75f, /*ret=*/3);  // the pair is recorded all the same
  w.good(1, 1, 0.25f);
  w.check("a launch failed");
  CHECK(w.collect() == 0, "collect failed");
  w.check("a launch failed, collected");
  CHECK(w.t.launches(1) == 2 && w.t.ms(1) == 1.0, "the failed launch's pair was not counted");
}

// synchronize or elapsed fails at each pair of a list spread over three slots
void collect_fails_mid_list() {
  for (int kind = 0; kind < 2; ++kind)
    for (int at = 0; at < 6; ++at) {
      World w;
      const int slot_of[6] = {2, 2, 6, 9, 9, 9};
      std::vector<int> stops;
      for (int i = 0; i < 6; ++i) {
        w.good(slot_of[i], 1, (float)(i + 1) * 0.5f);
        stops.push_back(w.created);
      }
      (kind ? w.fail_elapsed_of : w.fail_sync_of) = stops[at];
      char what[64];
      std::snprintf(what, sizeof what, "%s fails at pair %d", kind ? "elapsed" : "synchronize", at);
      CHECK(w.collect(stops[at]) == (kind ? 9 : 8), "%s: wrong return value", what);
      w.check(what);
      CHECK(w.collect(stops[at]) != 0, "%s (again): no error", what);
      w.check(what);
      w.fail_sync_of = w.fail_elapsed_of = 0;  // the error clears: a later collect finishes the job
      CHECK(w.collect() == 0, "%s (cleared): reported an error", what);
      w.check(what);
      CHECK((int)w.destroyed.size() == w.created && w.t.launches(9) == 3 && w.t.ms(2) == 1.5 && w.t.ms(6) == 1.5,
            "%s: not everything was counted in the end", what);
    }
}

}  // namespace

int main() {
  timing_off();
  several_slots_collect_reset();
  drop_at_close();
  create_fails();
  launch_fails();
  collect_fails_mid_list();
  std::printf("kernel_timers: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
