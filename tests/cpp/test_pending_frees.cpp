// The pending-free list of pbftv_dev_free (simple_pbft_amd/csrc/host/pending_frees.h)
// on the host alone: integer marks, a scripted "has it passed" table, and after
// EVERY call the conservation rule -- each entry is either still in the list, in
// order, with all its marks, or was released exactly once with every mark handed
// back exactly once.  Built with -fsanitize=address,undefined by
// tests/test_pending_frees.py.
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "pending_frees.h"

namespace {

using pbftv::MarkState;

struct Entry {
  int id;
  std::vector<int> ev;
};

int g_checks = 0, g_failed = 0;

#define CHECK(cond, ...)                     \
  do {                                       \
    ++g_checks;                              \
    if (!(cond)) {                           \
      ++g_failed;                            \
      if (g_failed <= 20) {                  \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);            \
        std::printf("\n");                   \
      }                                      \
    }                                        \
  } while (0)

// One list under test with its books.
struct World {
  std::vector<Entry> original, list;
  std::map<int, MarkState> state;     // mark -> scripted answer
  std::map<int, int> handed_back;     // mark -> times handed back
  std::map<int, int> released;        // entry id -> times released
  int fail_release_of = -1;           // entry id whose release reports an error
  int polls = 0;

  // n entries; entry i has 1 + i % 3 marks, numbered from 100 * (i + 1)
  explicit World(int n) {
    for (int i = 0; i < n; ++i) {
      Entry e{i, {}};
      for (int k = 0; k <= i % 3; ++k) {
        e.ev.push_back(100 * (i + 1) + k);
        state[e.ev.back()] = MarkState::kNotReady;
      }
      original.push_back(e);
    }
    list = original;
  }

  void set_entry(int i, MarkState st, int which = -1) {  // which: one mark of the entry (-1: all)
    const Entry& e = original[i];
    for (size_t k = 0; k < e.ev.size(); ++k)
      if (which < 0 || (size_t)which % e.ev.size() == k) state[e.ev[k]] = st;
  }

  bool reap() {
    return pbftv::reap_pending(
        list,
        [&](int m) {
          ++polls;
          return state.at(m);
        },
        [&](Entry& e) {
          for (int m : e.ev) ++handed_back[m];
        },
        [&](Entry& e) {
          ++released[e.id];
          return e.id != fail_release_of;
        });
  }

  // the first non-passed answer among the entry's marks, in order
  MarkState entry_state(const Entry& e) const {
    for (int m : e.ev)
      if (state.at(m) != MarkState::kPassed) return state.at(m);
    return MarkState::kPassed;
  }

  // The conservation rule, and (want_gone: ids expected to have left by now)
  // exactly which entries left.
  void check(const std::vector<int>& want_gone, const char* what) {
    size_t marks_total = 0, marks_in_list = 0, marks_back = 0;
    for (const Entry& e : original) marks_total += e.ev.size();
    for (const Entry& e : list) marks_in_list += e.ev.size();
    for (const auto& kv : handed_back) marks_back += (size_t)kv.second;
    CHECK(marks_in_list + marks_back == marks_total, "%s: %zu in list + %zu back != %zu", what, marks_in_list,
          marks_back, marks_total);
    int last_id = -1;
    for (const Entry& e : list) {
      CHECK(e.id > last_id, "%s: entry %d out of order or duplicated", what, e.id);
      last_id = e.id;
      CHECK(e.id >= 0 && e.id < (int)original.size() && e.ev == original[e.id].ev,
            "%s: entry %d in the list without all its marks (%zu of them)", what, e.id, e.ev.size());
    }
    for (const Entry& e : original) {
      const bool in_list = std::any_of(list.begin(), list.end(), [&](const Entry& x) { return x.id == e.id; });
      const bool gone = std::find(want_gone.begin(), want_gone.end(), e.id) != want_gone.end();
      CHECK(in_list == !gone, "%s: entry %d %s", what, e.id, in_list ? "still listed" : "left the list");
      const int rel = released.count(e.id) ? released.at(e.id) : 0;
      CHECK(rel == (in_list ? 0 : 1), "%s: entry %d released %d times, listed %d", what, e.id, rel, (int)in_list);
      for (int m : e.ev) {
        const int back = handed_back.count(m) ? handed_back.at(m) : 0;
        CHECK(back == (in_list ? 0 : 1), "%s: mark %d handed back %d times, entry listed %d", what, m, back,
              (int)in_list);
      }
    }
  }
};

// every done / not-done pattern of 0..6 entries ("first entry not done", the
// case where a compaction would move an entry onto itself, is every pattern
// with bit 0 clear)
void all_patterns() {
  for (int n = 0; n <= 6; ++n)
    for (int pat = 0; pat < (1 << n); ++pat)
      for (int hole = 0; hole < 3; ++hole) {  // which mark of a not-done entry has not passed
        World w(n);
        std::vector<int> gone;
        for (int i = 0; i < n; ++i) {
          w.set_entry(i, MarkState::kPassed);
          if ((pat >> i) & 1) gone.push_back(i);
          else w.set_entry(i, MarkState::kNotReady, hole);
        }
        char what[64];
        std::snprintf(what, sizeof what, "pattern n=%d done=0x%x hole=%d", n, pat, hole);
        CHECK(w.reap(), "%s: reported an error", what);
        w.check(gone, what);
        // a second pass changes nothing
        CHECK(w.reap(), "%s (again): reported an error", what);
        w.check(gone, what);
        // and once everything has passed, everything leaves
        for (int i = 0; i < n; ++i) {
          w.set_entry(i, MarkState::kPassed);
          if (!((pat >> i) & 1)) gone.push_back(i);
        }
        CHECK(w.reap(), "%s (all passed): reported an error", what);
        w.check(gone, what);
        CHECK(w.list.empty(), "%s: list not empty at the end", what);
      }
}

// an error at each position (a mark's, then a release's), over every pattern
void errors_everywhere() {
  for (int n = 1; n <= 6; ++n)
    for (int pat = 0; pat < (1 << n); ++pat)
      for (int at = 0; at < n; ++at)
        for (int kind = 0; kind < 2; ++kind) {
          World w(n);
          for (int i = 0; i < n; ++i) {
            w.set_entry(i, MarkState::kPassed);
            if (!((pat >> i) & 1)) w.set_entry(i, MarkState::kNotReady, i);
          }
          char what[80];
          std::snprintf(what, sizeof what, "%s error n=%d done=0x%x at=%d", kind ? "release" : "mark", n, pat, at);
          bool expect_ok = true;
          std::vector<int> gone;
          if (kind == 0) {
            w.set_entry(at, MarkState::kError, at + 1);
            // entries before the first one whose first unpassed mark is the error leave if done
            int stop = n;
            for (int i = 0; i < n && stop == n; ++i)
              if (w.entry_state(w.original[i]) == MarkState::kError) stop = i;
            expect_ok = stop == n;  // (the error mark may hide behind a not-ready one)
            for (int i = 0; i < stop; ++i)
              if (w.entry_state(w.original[i]) == MarkState::kPassed) gone.push_back(i);
          } else {
            w.fail_release_of = at;
            const bool hit = (pat >> at) & 1;  // only a done entry is released
            expect_ok = !hit;
            for (int i = 0; i < (hit ? at + 1 : n); ++i)
              if ((pat >> i) & 1) gone.push_back(i);
          }
          CHECK(w.reap() == expect_ok, "%s: wrong return value", what);
          w.check(gone, what);
          // the error clears: a later pass finishes the job
          w.fail_release_of = -1;
          for (int i = 0; i < n; ++i) w.set_entry(i, MarkState::kPassed);
          gone.clear();
          for (int i = 0; i < n; ++i) gone.push_back(i);
          CHECK(w.reap(), "%s (cleared): reported an error", what);
          w.check(gone, what);
        }
}

// marks pass one at a time, in three orders, with a reap after each
void one_mark_at_a_time() {
  for (int order = 0; order < 3; ++order) {
    World w(6);
    std::vector<int> marks;
    for (const Entry& e : w.original) marks.insert(marks.end(), e.ev.begin(), e.ev.end());
    if (order == 1) std::reverse(marks.begin(), marks.end());
    if (order == 2) {  // a fixed shuffle
      std::vector<int> m2;
      for (size_t i = 0; i < marks.size(); ++i) m2.push_back(marks[(i * 7 + 3) % marks.size()]);
      marks = m2;
    }
    for (size_t step = 0; step <= marks.size(); ++step) {
      if (step) w.state[marks[step - 1]] = MarkState::kPassed;
      std::vector<int> gone;
      for (const Entry& e : w.original)
        if (w.entry_state(e) == MarkState::kPassed) gone.push_back(e.id);
      char what[64];
      std::snprintf(what, sizeof what, "one at a time order=%d step=%zu", order, step);
      CHECK(w.reap(), "%s: reported an error", what);
      w.check(gone, what);
    }
    CHECK(w.list.empty(), "order %d: list not empty at the end", order);
  }
}

}  // namespace

int main() {
  all_patterns();
  errors_everywhere();
  one_mark_at_a_time();
  std::printf("pending_frees: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
