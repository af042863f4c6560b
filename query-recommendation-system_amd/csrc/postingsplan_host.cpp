// postingsplan_host.cpp -- postingsplan.h on the CPU: the windows of a request over its sorted posting lists, driven as
// postings.hip's request kernel drives them (even cut, count by binary search from a cursor, halve, pass, advance) and
// held to a direct count of every id.  Built by `make postingsplan_host` with -fsanitize=address,undefined: the lists
// are exactly as long as they say, so a search past either end is reported.
// Exit status 0 and "postingsplan ok" when every case agrees.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "postingsplan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

static int fail(const char *what, long long a, long long b, long long c) {
  fprintf(stderr, "postingsplan: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

struct Stats {
  int64_t passes = 0, halvings = 0, single_over = 0, empty = 0;
};

// Plans and "runs" one request: every pass adds its window's entries to `seen`.  Checks: windows ascending, disjoint and
// tiling [0, nq); a pass holds at most C entries or one id; the multiplicities found equal a direct count.
static int run_case(const std::vector<std::vector<int32_t>> &lists, int64_t nq, int32_t C, Stats *st) {
  const size_t a = lists.size();
  uint64_t total = 0;
  std::map<int32_t, int64_t> want, seen;
  for (const auto &l : lists) {
    total += l.size();
    for (size_t i = 0; i < l.size(); ++i) {
      if (i && l[i - 1] >= l[i]) return fail("a list is not ascending", (long long)i, l[i - 1], l[i]);
      if (l[i] < 0 || l[i] >= nq) return fail("an id outside [0, nq)", (long long)i, l[i], (long long)nq);
      ++want[l[i]];
    }
  }
  const int64_t width = pp_width(total, nq, C);
  if (width < 1) return fail("width below 1", (long long)width, (long long)total, (long long)nq);
  std::vector<int64_t> cur(a, 0), wend(a, 0);
  int64_t lo = 0;
  uint64_t covered = 0;
  while (lo < nq) {
    int64_t hi = pp_window_end(lo, nq, width);
    if (hi <= lo || hi > nq) return fail("a window that does not advance", (long long)lo, (long long)hi, (long long)nq);
    uint64_t count;
    for (;;) {
      count = 0;
      for (size_t i = 0; i < a; ++i) {
        wend[i] = pp_lower_bound(lists[i].data(), cur[i], (int64_t)lists[i].size(), hi);
        count += (uint64_t)(wend[i] - cur[i]);
      }
      if (pp_is_pass(count, lo, hi, C)) break;
      const int64_t mid = pp_halve(lo, hi);
      if (mid <= lo || mid >= hi) return fail("a halving that does not shrink", (long long)lo, (long long)mid, (long long)hi);
      hi = mid;
      ++st->halvings;
    }
    if (count > (uint64_t)C) {
      if (hi - lo != 1) return fail("a pass over C that is no single id", (long long)lo, (long long)hi, (long long)count);
      ++st->single_over;
    }
    size_t distinct = 0;
    std::map<int32_t, int64_t> in_pass;
    for (size_t i = 0; i < a; ++i)
      for (int64_t p = cur[i]; p < wend[i]; ++p) {
        const int32_t id = lists[i][(size_t)p];
        if (id < lo || id >= hi) return fail("an entry outside its window", id, (long long)lo, (long long)hi);
        ++in_pass[id];
      }
    distinct = in_pass.size();
    if (distinct > (size_t)C && hi - lo != 1) return fail("more keys than half the table", (long long)distinct, C, 0);
    if (pp_slot((uint32_t)lo) >= (uint32_t)PP_TABLE_SLOTS) return fail("a slot outside the table", (long long)lo, 0, 0);
    for (const auto &kv : in_pass) seen[kv.first] += kv.second;
    covered += count;
    if (!count) ++st->empty;
    ++st->passes;
    for (size_t i = 0; i < a; ++i) cur[i] = wend[i];
    lo = hi;
  }
  if (lo != nq) return fail("the windows do not end at nq", (long long)lo, (long long)nq, 0);
  if (covered != total) return fail("entries left out", (long long)covered, (long long)total, 0);
  for (size_t i = 0; i < a; ++i)
    if (cur[i] != (int64_t)lists[i].size()) return fail("a list not read to its end", (long long)i, (long long)cur[i], 0);
  if (seen != want) return fail("multiplicities differ", (long long)seen.size(), (long long)want.size(), 0);
  return 0;
}

// `len` distinct ids of [first, first + span), ascending
static std::vector<int32_t> draw(int64_t first, int64_t span, int64_t len) {
  std::vector<int32_t> out;
  if (len >= span) {
    for (int64_t j = 0; j < span; ++j) out.push_back((int32_t)(first + j));
    return out;
  }
  std::vector<char> hit((size_t)span, 0);
  for (int64_t n = 0; n < len;) {
    const int64_t j = rnd() % (uint64_t)span;
    if (!hit[(size_t)j]) hit[(size_t)j] = 1, ++n;
  }
  for (int64_t j = 0; j < span; ++j)
    if (hit[(size_t)j]) out.push_back((int32_t)(first + j));
  return out;
}

int main() {
  Stats st;
  // the lower bound itself, on exactly sized lists
  for (int len = 0; len <= 9; ++len) {
    std::vector<int32_t> l;
    for (int i = 0; i < len; ++i) l.push_back(3 * i + 1);
    for (int id = -2; id <= 3 * len + 3; ++id) {
      const int64_t got = pp_lower_bound(l.data(), 0, len, id);
      const int64_t ref = std::lower_bound(l.begin(), l.end(), id) - l.begin();
      if (got != ref) return fail("lower bound", len, id, (long long)got);
    }
  }
  // widths: no list, one pass, on both sides of a multiple of C, more passes than ids
  if (pp_width(0, 100, 8) != 100 || pp_width(8, 100, 8) != 100 || pp_width(9, 100, 8) != 50 || pp_width(16, 100, 8) != 50 ||
      pp_width(17, 100, 8) != 34 || pp_width(1000000, 100, 8) != 1 || pp_width(5, 0, 8) != 1 || pp_width(50, 1, 8) != 1 ||
      pp_width(~0ull, 2147483647, PP_PASS_ENTRIES) != 1)
    return fail("width", 0, 0, 0);
  if (pp_window_end(0, 10, 4) != 4 || pp_window_end(8, 10, 4) != 10 || pp_window_end(6, 10, 4) != 10 ||
      pp_window_end(0, 2147483647, 2147483647) != 2147483647 || pp_halve(4, 6) != 5 || pp_halve(4, 7) != 5)
    return fail("window ends", 0, 0, 0);
  for (uint32_t id = 0; id < 200000; id += 7)
    if (pp_slot(id) >= (uint32_t)PP_TABLE_SLOTS || pp_slot(~id) >= (uint32_t)PP_TABLE_SLOTS) return fail("slot", id, 0, 0);

  const int32_t C = 64;   // a small C: many passes from small lists
  // no list at all, empty lists only, one id
  if (run_case({}, 50, C, &st) || run_case({{}, {}}, 50, C, &st) || run_case({{0}}, 1, C, &st)) return 1;
  // one list on both sides of C; a list of every id
  for (int len : {C - 1, C, C + 1, 2 * C, 2 * C + 1})
    if (run_case({draw(0, 1000, len)}, 1000, C, &st)) return 1;
  if (run_case({draw(0, 500, 500)}, 500, C, &st)) return 1;
  // more lists than C holding one id: a single id over C
  {
    std::vector<std::vector<int32_t>> ls((size_t)(C + 5), std::vector<int32_t>{7});
    const int64_t before = st.single_over;
    if (run_case(ls, 20, C, &st)) return 1;
    if (st.single_over == before) return fail("the single id over C did not occur", 0, 0, 0);
  }
  // everything inside a narrow range of a wide id space: the even cut overflows, the halving runs
  {
    const int64_t before = st.halvings;
    if (run_case({draw(70000, 90, 80), draw(70010, 90, 80)}, 1 << 20, C, &st)) return 1;
    if (st.halvings == before) return fail("the narrow range did not halve", 0, 0, 0);
  }
  // random shapes
  for (int round = 0; round < 300; ++round) {
    const int64_t nq = 1 + rnd() % 5000;
    const int a = (int)(rnd() % 40);
    std::vector<std::vector<int32_t>> ls;
    for (int i = 0; i < a; ++i) {
      const int64_t span = 1 + rnd() % (uint64_t)nq, first = rnd() % (uint64_t)(nq - span + 1);
      ls.push_back(draw(first, span, rnd() % (uint64_t)(span + 1)));
    }
    if (run_case(ls, nq, 1 + (int32_t)(rnd() % 200), &st)) return fail("random round", round, (long long)nq, a);
  }
  // the library's own C on a list that needs three passes
  if (run_case({draw(0, 40000, 2 * PP_PASS_ENTRIES + 1)}, 40000, PP_PASS_ENTRIES, &st)) return 1;
  printf("postingsplan ok: %lld passes, %lld halvings, %lld single ids over C, %lld empty windows\n", (long long)st.passes,
         (long long)st.halvings, (long long)st.single_over, (long long)st.empty);
  return 0;
}
