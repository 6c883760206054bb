// The list of device blocks whose free waits for marks (pbftv_dev_free:
// events recorded on the context's streams when the free was called).  No HIP
// here: the caller supplies what a mark is and how it is polled, so the list
// logic compiles and is tested on the host alone (tests/cpp/test_pending_frees.cpp).
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

namespace pbftv {

enum class MarkState { kNotReady, kPassed, kError };

// One pass over `list` (entries with a member `ev`, the entry's marks), in order:
//   passed(mark)     -> MarkState   has this mark passed: no / yes / error
//   give_back(entry)                hand every mark of the entry back (called once per released entry)
//   release(entry)   -> bool        release the entry's block (false: an error; the block counts as released)
// An entry whose marks have all passed is released and leaves the list; every
// other entry stays, in order, with all its marks.  The pass stops at the first
// error (a mark's or a release's) and returns false; the entries it did not
// reach stay as they are.  So after any call each entry is either still in the
// list with every mark, or was released exactly once with every mark handed
// back exactly once: none is moved from and left behind, none is duplicated.
template <class Entry, class Passed, class GiveBack, class Release>
bool reap_pending(std::vector<Entry>& list, Passed passed, GiveBack give_back, Release release) {
  size_t keep = 0, i = 0;
  bool ok = true;
  for (; i < list.size() && ok; ++i) {
    Entry& e = list[i];
    MarkState st = MarkState::kPassed;
    for (const auto& m : e.ev) {
      st = passed(m);
      if (st != MarkState::kPassed) break;
    }
    if (st == MarkState::kPassed) {
      give_back(e);
      ok = release(e);
      continue;
    }
    if (st == MarkState::kError) ok = false;
    if (keep != i) list[keep] = std::move(e);  // (never onto itself: a self-move would empty e.ev)
    ++keep;
  }
  for (; i < list.size(); ++i, ++keep)
    if (keep != i) list[keep] = std::move(list[i]);
  list.erase(list.begin() + (std::ptrdiff_t)keep, list.end());
  return ok;
}

}  // namespace pbftv
