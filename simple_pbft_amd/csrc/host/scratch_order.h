// The order in which streams use one device's shared scratch: the mutex orders
// the enqueues, this state orders the execution.  A use on another stream than
// the last user's first waits for an event recorded on the last user's stream
// after its work.  A caller stream's use is fenced by an event recorded right
// after it.  The library's own stream (which lives as long as the context) is
// fenced lazily: its event is recorded only when another stream next wants the
// scratch -- recording later on the same stream covers at least the scratch
// work -- so back-to-back uses on it queue no marker between batches (each
// marker costs the GPU a ~6 us gap between kernels, rocprof timeline).
// No HIP here: the caller supplies the two operations, so the state machine
// compiles and is tested on the host alone (tests/cpp/test_scratch_order.cpp).
//   record(Event&, Stream)  record the event on the stream (created at first use)
//   wait(Stream, Event)     the stream waits for the event
// each returning the caller's error type (value-initialised: success).
#pragma once

#include <utility>

namespace pbftv {

template <class Stream, class Event>
class ScratchOrder {
 public:
  void set_own(Stream own) { own_ = own; }

  // before enqueueing scratch work on st
  template <class Record, class Wait>
  auto acquire(Stream st, Record record, Wait wait) -> decltype(wait(st, Event{})) {
    using Err = decltype(wait(st, Event{}));
    if (last_ == Stream{} || last_ == st) return {};
    if (unrecorded_) {
      const Err e = record(ev_, last_);
      if (e != Err{}) return e;
      unrecorded_ = false;
    }
    return wait(st, ev_);
  }

  // after it: st is the last user from here on, whatever record answers
  template <class Record>
  auto release(Stream st, Record record) -> decltype(record(std::declval<Event&>(), st)) {
    using Err = decltype(record(std::declval<Event&>(), st));
    last_ = st;
    unrecorded_ = true;
    if (st == own_) return {};
    const Err e = record(ev_, st);
    if (e == Err{}) unrecorded_ = false;  // (else the next acquire tries again, as for the own stream)
    return e;
  }

  Stream last() const { return last_; }
  Event event() const { return ev_; }
  // the event covering the last use if a stream other than the own one made
  // it: what a host-side wait for caller-stream scratch work waits for
  Event caller_fence() const { return last_ != Stream{} && last_ != own_ && !unrecorded_ ? ev_ : Event{}; }

 private:
  Stream own_{}, last_{};
  Event ev_{};
  bool unrecorded_ = false;  // ev_ not yet recorded for last_'s last use
};

// One use of the scratch on one stream: acquire() before the first enqueue,
// release() on the success path (it returns the error); any other exit after
// a successful acquire releases in the destructor, best effort, so enqueued
// work is never left attributed to the stream before it.  release() again:
// the same fence, moved behind work enqueued since.  shared == false (a
// stream with scratch of its own): both do nothing.
template <class Stream, class Event, class Ops>
class ScratchLease {
 public:
  using Err = decltype(Ops::wait(Stream{}, Event{}));
  ScratchLease(ScratchOrder<Stream, Event>& order, Stream st, bool shared = true)
      : order_(order), st_(st), shared_(shared) {}
  ScratchLease(const ScratchLease&) = delete;
  ~ScratchLease() {
    if (held_) (void)order_.release(st_, Ops::record);
  }
  Err acquire() {
    if (!shared_) return {};
    const Err e = order_.acquire(st_, Ops::record, Ops::wait);
    held_ = e == Err{};
    return e;
  }
  Err release() {
    if (!shared_) return {};
    held_ = false;
    return order_.release(st_, Ops::record);
  }

 private:
  ScratchOrder<Stream, Event>& order_;
  Stream st_;
  bool shared_, held_ = false;
};

}  // namespace pbftv
