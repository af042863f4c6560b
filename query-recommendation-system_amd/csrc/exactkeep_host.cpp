// exactkeep_host.cpp -- exactkeep.h on the CPU: the kept-list insert, the threshold word and the merge comparison of
// exactlists.hip's kernels, held to std::sort over exact fractions.  Built by `make exactkeep_host` with
// -fsanitize=address,undefined: the arrays are exactly K words long, so a move past either end is reported.
// Exit status 0 and "exactkeep ok" when every case agrees.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "exactkeep.h"

struct Entry {
  int32_t inter, uni, id;
};

static bool before(const Entry &a, const Entry &b) {   // the order restated: 128-bit products, then the id
  const __int128 l = (__int128)a.inter * b.uni, r = (__int128)b.inter * a.uni;
  return l != r ? l > r : a.id < b.id;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

static int fail(const char *what, int a, int b, int c) {
  fprintf(stderr, "exactkeep: %s (%d, %d, %d)\n", what, a, b, c);
  return 1;
}

// n candidates with unions up to max_union and only `levels` distinct intersections (many ties), ids 0 .. n - 1 shuffled
static std::vector<Entry> candidates(int n, int max_union, int levels) {
  std::vector<Entry> c(n);
  for (int i = 0; i < n; ++i) {
    const int32_t uni = 1 + (int32_t)(rnd() % (uint32_t)max_union);
    int32_t inter = 1 + (int32_t)(rnd() % (uint32_t)levels);
    if (inter > uni) inter = uni;
    c[i] = Entry{inter, uni, i};
  }
  for (int i = n - 1; i > 0; --i) std::swap(c[i], c[rnd() % (uint32_t)(i + 1)]);
  return c;
}

// one kept list of exactly K words per array, fed through the threshold as the sweep feeds it; stale_every > 0 makes
// every such candidate read a threshold that is `lag` updates old
static int keep_case(int n, int K, int max_union, int levels, int stale_every, std::vector<Entry> *kept_out) {
  const std::vector<Entry> c = candidates(n, max_union, levels);
  std::vector<uint32_t> in(K), un(K), ids(K);
  std::vector<uint64_t> history(1, ek_threshold(EK_NONE_INTER, EK_NONE_UNION));
  int cnt = 0, entered = 0;
  for (int i = 0; i < n; ++i) {
    const size_t lag = stale_every && i % stale_every == 0 ? std::min<size_t>(history.size() - 1, 5) : 0;
    const uint64_t thr = history[history.size() - 1 - lag];
    if (!ek_may_enter(c[i].inter, c[i].uni, thr)) continue;
    ++entered;
    cnt = ek_insert(in.data(), un.data(), ids.data(), cnt, K, c[i].inter, c[i].uni, c[i].id);
    if (cnt == K) {
      const uint64_t now = ek_threshold((int32_t)in[K - 1], (int32_t)un[K - 1]);
      if (ek_cmp_j((int32_t)(now >> 32), (int32_t)now, (int32_t)(history.back() >> 32), (int32_t)history.back()) > 0)
        return fail("the threshold fell", n, K, i);
      history.push_back(now);
    }
  }
  std::vector<Entry> want(c);
  std::sort(want.begin(), want.end(), before);
  const int L = std::min(n, K);
  if (cnt != L) return fail("count", n, K, cnt);
  for (int e = 0; e < L; ++e)
    if ((int32_t)in[e] != want[e].inter || (int32_t)un[e] != want[e].uni || (int32_t)ids[e] != want[e].id)
      return fail("kept list differs from the sort", n, K, e);
  if (n > 4 * K && levels > 8 && entered >= n) return fail("the threshold filtered nothing", n, K, entered);
  if (kept_out) {
    kept_out->clear();
    for (int e = 0; e < L; ++e) kept_out->push_back(Entry{(int32_t)in[e], (int32_t)un[e], (int32_t)ids[e]});
  }
  return 0;
}

// the finish: S partial lists (the ids dealt to slices by range, each kept on its own), K rounds over their heads
static int merge_case(int n, int K, int S, int max_union, int levels) {
  std::vector<Entry> c = candidates(n, max_union, levels);
  std::vector<std::vector<Entry>> part(S);
  const int per = (n + S - 1) / S;
  for (int y = 0; y < S; ++y) {
    std::vector<uint32_t> in(K), un(K), ids(K);
    int cnt = 0;
    for (const Entry &e : c)
      if (e.id / per == y) cnt = ek_insert(in.data(), un.data(), ids.data(), cnt, K, e.inter, e.uni, e.id);
    for (int e = 0; e < K; ++e)
      part[y].push_back(e < cnt ? Entry{(int32_t)in[e], (int32_t)un[e], (int32_t)ids[e]}
                                : Entry{EK_NONE_INTER, EK_NONE_UNION, EK_NONE_ID});
  }
  std::sort(c.begin(), c.end(), before);
  std::vector<int> at(S, 0);
  for (int e = 0; e < K; ++e) {
    Entry best{EK_NONE_INTER, EK_NONE_UNION, EK_NONE_ID};
    int own = -1;
    for (int y = 0; y < S; ++y) {
      if (at[y] >= K) continue;
      const Entry &h = part[y][at[y]];
      if (ek_before(h.inter, h.uni, h.id, best.inter, best.uni, best.id)) {
        best = h;
        own = y;
      }
    }
    if (e < n) {
      if (own < 0 || best.id != c[e].id || best.inter != c[e].inter || best.uni != c[e].uni)
        return fail("merged list differs from the sort", n, K, e);
      ++at[own];
    } else if (own >= 0) {
      return fail("an entry past the candidates", n, K, e);
    }
  }
  return 0;
}

int main() {
  int bad = 0;
  const int Ks[] = {1, 2, 3, 63, 64};
  for (int K : Ks) {
    for (int n : {0, 1, K - 1, K, K + 1, 5 * K + 3, 2000}) {
      if (n < 0) continue;
      bad += keep_case(n, K, 1 << 21, 1 << 20, 0, nullptr);   // spread fractions, the largest unions
      bad += keep_case(n, K, 12, 3, 0, nullptr);              // few distinct fractions: ties decided by the id
      bad += keep_case(n, K, 1, 1, 0, nullptr);               // all J = 1
      bad += keep_case(n, K, 1 << 21, 1 << 20, 3, nullptr);   // stale thresholds
      bad += keep_case(n, K, 12, 3, 2, nullptr);
      for (int S : {1, 2, 7, 256}) {
        bad += merge_case(n, K, S, 12, 3);
        bad += merge_case(n, K, S, 1 << 21, 1 << 20);
      }
    }
  }
  // neighbours in the Farey sequence at the largest unions (a / b - c / d = 1 / (b d)): the closest distinct fractions
  // there are, a before b in each pair, the ids the other way round
  const int32_t q = 1 << 21;
  struct {
    Entry a, b;
  } close[] = {{{1, q - 1, 1}, {1, q, 0}}, {{q - 1, q, 5}, {q - 2, q - 1, 4}}, {{1, 2, 9}, {(q - 2) / 2, q - 1, 3}}};
  for (auto &p : close) {
    if (!before(p.a, p.b)) bad += fail("the Farey pair is not ordered as stated", p.a.id, p.b.id, 0);
    if (!ek_before(p.a.inter, p.a.uni, p.a.id, p.b.inter, p.b.uni, p.b.id) ||
        ek_before(p.b.inter, p.b.uni, p.b.id, p.a.inter, p.a.uni, p.a.id))
      bad += fail("ek_before on a Farey pair", p.a.id, p.b.id, 0);
    if (ek_may_enter(p.b.inter, p.b.uni, ek_threshold(p.a.inter, p.a.uni)) ||
        !ek_may_enter(p.a.inter, p.a.uni, ek_threshold(p.b.inter, p.b.uni)) ||
        !ek_may_enter(p.a.inter, p.a.uni, ek_threshold(p.a.inter, p.a.uni)))
      bad += fail("ek_may_enter on a Farey pair", p.a.id, p.b.id, 0);
  }
  if (bad) return 1;
  printf("exactkeep ok\n");
  return 0;
}
