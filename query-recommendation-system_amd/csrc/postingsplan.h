// postingsplan.h -- the window rule of the exact lists from postings (postings.hip's request kernel;
// postingsplan_host.cpp runs the same functions on the CPU under the host sanitizers).  Plain integer code with no device
// intrinsics: it compiles for the host without HIP.
//
// A request reads a sorted posting lists (ids ascending in each).  Its candidates are counted in a hash table of
// PP_TABLE_SLOTS slots, filled in PASSES over disjoint id windows [lo, hi) that tile [0, nq) in ascending order.  A window
// is a pass when it holds at most PP_PASS_ENTRIES list entries -- so at most that many distinct ids: the table stays at
// most half full -- or when it is a single id, which is one key however many lists hold it.  The first cut is even:
// ceil(total / PP_PASS_ENTRIES) windows of equal width.  A window that is neither is halved, from the same lo, until it
// is one of the two; the width ends at 1, so this terminates, and every pass advances lo by at least 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PP_HD __host__ __device__ static inline
#else
#define PP_HD static inline
#endif

constexpr int32_t PP_TABLE_SLOTS = 16384;                 // (id, count) slots, a power of two
constexpr int32_t PP_PASS_ENTRIES = PP_TABLE_SLOTS / 2;   // C: list entries per pass

// the width of the even cut: ceil(total / C) windows over [0, nq); at least 1
PP_HD int64_t pp_width(uint64_t total, int64_t nq, int32_t C) {
  const uint64_t passes = total / (uint64_t)C + (total % (uint64_t)C ? 1 : 0);
  if (passes <= 1 || nq <= 1) return nq < 1 ? 1 : nq;
  const uint64_t w = ((uint64_t)nq + passes - 1) / passes;
  return w < 1 ? 1 : (int64_t)w;
}

// the end of the window that starts at lo
PP_HD int64_t pp_window_end(int64_t lo, int64_t nq, int64_t width) { return nq - lo < width ? nq : lo + width; }

// a window of `count` entries runs as it is
PP_HD bool pp_is_pass(uint64_t count, int64_t lo, int64_t hi, int32_t C) { return count <= (uint64_t)C || hi - lo <= 1; }

// the end of the lower half of a window that is no pass (hi - lo >= 2)
PP_HD int64_t pp_halve(int64_t lo, int64_t hi) { return lo + (hi - lo) / 2; }

// first position p in [b, e) with list[p] >= id, e when there is none; stays inside [b, e] whatever the list holds
PP_HD int64_t pp_lower_bound(const int32_t *list, int64_t b, int64_t e, int64_t id) {
  while (b < e) {
    const int64_t mid = b + (e - b) / 2;
    if ((int64_t)list[mid] < id) b = mid + 1;
    else e = mid;
  }
  return b;
}

// the table slot an id starts probing at
PP_HD uint32_t pp_slot(uint32_t id) { return (id * 2654435761u) >> 18; }
static_assert(PP_TABLE_SLOTS == 1 << 14, "pp_slot keeps the top 14 bits of the product");
