// exactkeep.h -- the total order of exact neighbours and the kept list of the best K under it (exactlists.hip's sweep
// and finish; exactkeep_host.cpp exercises the same functions on the CPU under the host sanitizers).  Plain integer code
// with no device intrinsics: it compiles for the host without HIP.
//
// An entry is (inter, union, id) with 1 <= inter <= union, J = inter / union.  a comes BEFORE b when J_a > J_b, decided by
// inter_a * union_b > inter_b * union_a in int64 (inter, union <= 2^21: the products stay below 2^42), ties by the
// smaller id: a total order over distinct ids.  EK_NONE (J = 0, the largest id) comes after every entry.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EK_HD __host__ __device__ static inline
#else
#define EK_HD static inline
#endif

constexpr int32_t EK_NONE_INTER = 0, EK_NONE_UNION = 1, EK_NONE_ID = 2147483647;

// -1 / 0 / +1: J_a above, equal to, below J_b
EK_HD int ek_cmp_j(int32_t ia, int32_t ua, int32_t ib, int32_t ub) {
  const int64_t l = (int64_t)ia * ub, r = (int64_t)ib * ua;
  return l > r ? -1 : (l < r ? 1 : 0);
}

// a before b in the total order
EK_HD bool ek_before(int32_t ia, int32_t ua, int32_t da, int32_t ib, int32_t ub, int32_t db) {
  const int c = ek_cmp_j(ia, ua, ib, ub);
  return c < 0 || (c == 0 && da < db);
}

// The threshold word of a kept list: inter << 32 | union of its K-th entry once it holds K, (0, 1) before.  A candidate
// whose J is not BELOW the word's may belong to the list (an equal J is decided by the ids, under the lock).  The word
// only ever rises, so a stale one lets more through and drops nothing.
EK_HD uint64_t ek_threshold(int32_t inter, int32_t uni) { return (uint64_t)(uint32_t)inter << 32 | (uint32_t)uni; }
EK_HD bool ek_may_enter(int32_t inter, int32_t uni, uint64_t threshold) {
  return ek_cmp_j(inter, uni, (int32_t)(threshold >> 32), (int32_t)(threshold & 0xFFFFFFFFull)) <= 0;
}

// Insert (inter, uni, id) into the list kept in order in in[0, n) / un / ids (arrays of at least K words; volatile-free
// plain words: the caller holds whatever lock guards them), n <= K.  The list keeps the best K: a candidate that does
// not come before the K-th entry of a full list is dropped.  -> the new n.  At most K moves.
template <typename W>
EK_HD int ek_insert(W *in, W *un, W *ids, int n, int K, int32_t inter, int32_t uni, int32_t id) {
  int e = n;   // the slot the candidate would take
  if (n == K) {
    if (!ek_before(inter, uni, id, (int32_t)in[K - 1], (int32_t)un[K - 1], (int32_t)ids[K - 1])) return n;
    e = K - 1;   // the K-th entry leaves
  }
  for (; e > 0 && ek_before(inter, uni, id, (int32_t)in[e - 1], (int32_t)un[e - 1], (int32_t)ids[e - 1]); --e) {
    in[e] = in[e - 1];
    un[e] = un[e - 1];
    ids[e] = ids[e - 1];
  }
  in[e] = (W)inter;
  un[e] = (W)uni;
  ids[e] = (W)id;
  return n < K ? n + 1 : K;
}
