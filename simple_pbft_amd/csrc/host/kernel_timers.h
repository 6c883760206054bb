// The kernel timing table of one device: per slot, the event pairs recorded
// around launches and not yet read, the summed time of those read and their
// count.  No HIP here: the caller supplies the event operations, so the table
// compiles and is tested on the host alone (tests/cpp/test_kernel_timers.cpp).
//   Ops::create(Event*)  Ops::destroy(Event)  Ops::record(Event, Stream)
//   Ops::synchronize(Event)  Ops::elapsed(float* ms, Event start, Event stop)
// each returning the caller's error type (value-initialised: success).  After
// any call every event ever created is in one pending pair or was destroyed once.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace pbftv {

template <class Event, int N, class Ops>
class KernelTimers {
 public:
  // launch(), between two events on st when `on`.  Off: the launch and nothing
  // else (no event, no allocation).  A create that fails means no launch (and
  // no event left behind); a launch that fails still leaves its pair pending.
  template <class Stream, class F>
  auto timed(bool on, int slot, Stream st, F&& launch) -> decltype(launch()) {
    using Err = decltype(launch());
    if (!on) return launch();
    Event a{}, b{};
    Err e = Ops::create(&a);
    if (e != Err{}) return e;
    e = Ops::create(&b);
    if (e != Err{}) {
      (void)Ops::destroy(a);
      return e;
    }
    (void)Ops::record(a, st);
    e = launch();
    (void)Ops::record(b, st);
    pending_[slot].push_back({a, b});
    return e;
  }

  // Every pending pair into its slot's sum and count and its events destroyed,
  // in slot order.  Stops at the first synchronize / elapsed error and returns
  // it: that pair and those after it stay pending, those before it have left.
  auto collect() -> decltype(Ops::synchronize(Event{})) {
    using Err = decltype(Ops::synchronize(Event{}));
    for (int k = 0; k < N; ++k) {
      auto& list = pending_[k];
      size_t done = 0;
      Err e{};
      for (; done < list.size(); ++done) {
        float t = 0;
        e = Ops::synchronize(list[done].second);
        if (e == Err{}) e = Ops::elapsed(&t, list[done].first, list[done].second);
        if (e != Err{}) break;
        ms_[k] += t;
        launches_[k] += 1;
        (void)Ops::destroy(list[done].first);
        (void)Ops::destroy(list[done].second);
      }
      list.erase(list.begin(), list.begin() + (std::ptrdiff_t)done);
      if (e != Err{}) return e;
    }
    return {};
  }

  // the sums and counts back to zero (pending pairs stay: collect first)
  void reset() {
    for (int k = 0; k < N; ++k) ms_[k] = 0, launches_[k] = 0;
  }

  // every pending pair destroyed unread (the context closes)
  void drop() {
    for (auto& list : pending_) {
      for (auto& pr : list) (void)Ops::destroy(pr.first), (void)Ops::destroy(pr.second);
      list.clear();
    }
  }

  double ms(int slot) const { return ms_[slot]; }
  uint64_t launches(int slot) const { return launches_[slot]; }
  size_t pending(int slot) const { return pending_[slot].size(); }

 private:
  std::vector<std::pair<Event, Event>> pending_[N];
  double ms_[N] = {};
  uint64_t launches_[N] = {};
};

}  // namespace pbftv
