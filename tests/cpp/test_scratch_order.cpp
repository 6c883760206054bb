// The scratch order and its lease (simple_pbft_amd/csrc/host/scratch_order.h)
// on the host alone: the two supplied operations are logged, and every
// sequence of up to 5 uses over three streams -- the library's own and two
// others -- is enumerated, each use ending by an explicit release or by an
// early exit after its work was enqueued.  Built with
// -fsanitize=address,undefined by tests/test_scratch_order.py.
#include <cstdio>
#include <vector>

#include "scratch_order.h"

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

constexpr int kOwn = 1;                       // the library's stream; 0 is "no stream"
constexpr int kStreams[3] = {kOwn, 2, 3};

// What was put on the streams, in order.  A wait refers to the record of the
// event that was the latest when the wait was issued (an event wait's meaning).
enum Kind { kWork, kRecord, kWait };
struct Op {
  Kind kind;
  int stream;
  int ref;  // kWork: the use's number; kWait: index of the record waited for (-1: never recorded)
};
std::vector<Op> g_log;
int g_last_record = -1;

struct Ops {
  static int record(int& ev, int st) {
    if (!ev) ev = 1;  // created at first use
    g_last_record = (int)g_log.size();
    g_log.push_back({kRecord, st, 0});
    return 0;
  }
  static int wait(int st, int ev) {
    CHECK(ev != 0, "a wait for an event that was never created");
    g_log.push_back({kWait, st, g_last_record});
    return 0;
  }
};
using Order = pbftv::ScratchOrder<int, int>;
using Lease = pbftv::ScratchLease<int, int, Ops>;

// one use of the scratch on st; released: by release(), else by leaving early
void use(Order& o, int st, int number, bool released) {
  Lease lease(o, st);
  CHECK(lease.acquire() == 0, "acquire failed");
  g_log.push_back({kWork, st, number});
  if (released) CHECK(lease.release() == 0, "release failed");
}

int last_work_of(int number) {
  int at = -1;
  for (size_t i = 0; i < g_log.size(); ++i)
    if (g_log[i].kind == kWork && g_log[i].ref == number) at = (int)i;
  return at;
}
int first_work_of(int number) {
  for (size_t i = 0; i < g_log.size(); ++i)
    if (g_log[i].kind == kWork && g_log[i].ref == number) return (int)i;
  return -1;
}

// Use `number` on st follows use `number - 1` on prev: it runs after it.
void check_follows(int prev, int st, int number, const char* what) {
  const int prev_end = last_work_of(number - 1), mine = first_work_of(number);
  CHECK(prev_end >= 0 && mine > prev_end, "%s: use %d not enqueued after use %d", what, number, number - 1);
  if (prev == st) return;  // stream order
  bool fenced = false;
  for (int i = prev_end + 1; i < mine; ++i) {
    const Op& w = g_log[i];
    if (w.kind != kWait || w.stream != st || w.ref < 0) continue;
    const Op& r = g_log[w.ref];
    if (r.kind == kRecord && r.stream == prev && w.ref > prev_end) fenced = true;
  }
  CHECK(fenced, "%s: use %d on stream %d does not wait for use %d on stream %d", what, number, st, number - 1, prev);
}

void every_sequence() {
  for (int len = 1; len <= 5; ++len) {
    int total = 1;
    for (int i = 0; i < len; ++i) total *= 6;
    for (int code = 0; code < total; ++code) {
      g_log.clear();
      g_last_record = -1;
      Order o;
      o.set_own(kOwn);
      char what[64];
      std::snprintf(what, sizeof what, "sequence len=%d code=%d", len, code);
      int prev = 0, c = code;
      for (int i = 0; i < len; ++i, c /= 6) {
        const int st = kStreams[c % 3];
        const bool released = (c % 6) < 3;
        const size_t log0 = g_log.size();
        use(o, st, i, released);
        // however it ended, the scratch is this stream's now, never an older one's
        CHECK(o.last() == st, "%s: after use %d on %d the last user is %d", what, i, st, o.last());
        if (i == 0) CHECK(g_log[log0].kind == kWork, "%s: the first use waited for something", what);
        if (i > 0) check_follows(prev, st, i, what);
        if (prev == kOwn && st == kOwn) {
          // back-to-back on the library's stream: no marker, from the previous
          // use's work to the end of this use
          for (size_t k = (size_t)last_work_of(i - 1); k < g_log.size(); ++k)
            CHECK(g_log[k].kind == kWork, "%s: use %d put a marker between batches on the own stream", what, i);
        }
        if (st == kOwn) {
          for (size_t k = (size_t)first_work_of(i); k < g_log.size(); ++k)
            CHECK(g_log[k].kind != kRecord, "%s: use %d on the own stream recorded after itself", what, i);
        } else {
          // a caller stream's use is fenced right after it
          CHECK(g_log.back().kind == kRecord && g_log.back().stream == st,
                "%s: use %d on stream %d left no record behind", what, i, st);
          CHECK(o.caller_fence() != 0, "%s: no fence to wait for on the host after use %d", what, i);
        }
        if (st == kOwn) CHECK(o.caller_fence() == 0, "%s: a host-side fence for the own stream", what);
        prev = st;
      }
    }
  }
}

// a lease inside a lease on one stream (a signer inside the DER signer), work
// after the inner one, and a second release behind later work (the DER verify)
void nested_and_again() {
  for (int st : {2, kOwn}) {
    g_log.clear();
    g_last_record = -1;
    Order o;
    o.set_own(kOwn);
    use(o, 3, 0, true);
    {
      Lease outer(o, st);
      CHECK(outer.acquire() == 0, "outer acquire failed");
      {
        Lease inner(o, st);
        CHECK(inner.acquire() == 0, "inner acquire failed");
        g_log.push_back({kWork, st, 1});
        CHECK(inner.release() == 0, "inner release failed");
      }
      g_log.push_back({kWork, st, 1});
      CHECK(outer.release() == 0, "outer release failed");
      g_log.push_back({kWork, st, 1});
      CHECK(outer.release() == 0, "second release failed");
    }
    check_follows(3, st, 1, "nested");
    use(o, 3, 2, false);
    check_follows(st, 3, 2, "after nested");  // (behind the LAST work of use 1)
    use(o, 2, 3, true);
    check_follows(3, 2, 3, "after an early exit");
  }
}

// a stream with scratch of its own: the lease does nothing
void not_shared() {
  g_log.clear();
  Order o;
  o.set_own(kOwn);
  use(o, 2, 0, true);
  const size_t n = g_log.size();
  {
    Lease lease(o, 3, /*shared=*/false);
    CHECK(lease.acquire() == 0 && lease.release() == 0, "an unshared lease reported an error");
  }
  CHECK(g_log.size() == n && o.last() == 2, "an unshared lease touched the order");
}

}  // namespace

int main() {
  every_sequence();
  nested_and_again();
  not_shared();
  std::printf("scratch_order: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
