// fidelitywalk.h -- what the sweeps over the CSR answer sets share (fidelity.hip, exactlists.hip): the group rule and the
// LDS budget, the interleaved bitmap of a workgroup's G answer sets, the walk that fetches one swept query ahead, a
// request's chosen query and the slice rule.  One copy: the two sweeps stage and test the bitmap in the same way.
#pragma once
#include "common.h"

namespace {

constexpr int FD_W = 16;                         // lanes per edge / per swept query
constexpr int FD_MAXK = QRLSH_FIDELITY_MAX_K;    // entries per list row
constexpr int FD_SWEEP_THREADS = 1024;           // one workgroup per CU (its LDS is the CU's): 16 waves hide the row reads
constexpr int FD_SWEEP_GROUPS = FD_SWEEP_THREADS / FD_W;
constexpr int FD_LDS_WORDS = 160 * 1024 / 4;     // the LDS of a gfx950 CU
constexpr int FD_MAXG = 32;                      // requests per workgroup: the bits of one LDS word
constexpr int FD_FIXED_WORDS = 4 * FD_MAXG;      // per request: four words of the sweep's own
constexpr int FD_REQ_WORDS = 4 * FD_MAXK;        // per request: the sweep's entries
constexpr int64_t FD_MAX_D = 1ll << 20;
constexpr int64_t FD_MAX_M = 1ll << 24;
constexpr int FD_MAXS = 256;                     // slices of the ids
constexpr int64_t FD_AUTO_BLOCKS = 1024;         // slices = auto: about four workgroups per CU in all ...
constexpr int64_t FD_MIN_SLICE = 4096;           // ... of at least this many ids each (a workgroup first stages its bitmap)

// requests per workgroup at D table rows: the widest power of two whose interleaved bitmap, entries and fixed words fit
// the LDS (host and device; exported as qrlsh_list_fidelity_group)
__host__ __device__ constexpr int fd_group(int64_t D) {
  for (int g = FD_MAXG; g > 1; g >>= 1)
    if ((D * g + 31) / 32 + (int64_t)g * FD_REQ_WORDS + FD_FIXED_WORDS <= FD_LDS_WORDS) return g;
  return 1;
}
static_assert(fd_group(0) == FD_MAXG && fd_group(FD_MAX_D) == 1, "G from 32 down to 1");
static_assert((FD_MAX_D + 31) / 32 + FD_REQ_WORDS + FD_FIXED_WORDS <= FD_LDS_WORDS, "D = 2^20 fits at G = 1");

// request x's chosen query, or -1 when it is outside [0, nq) or its list row is longer than FD_MAXK (bits: the flags);
// q_off == nullptr: there are no list rows, len stays 0
__device__ static inline int64_t fd_request(const int32_t *__restrict__ queries, int64_t x, int64_t nq,
                                            const int64_t *__restrict__ q_off, int64_t &len, uint32_t &bits) {
  const int64_t s = queries ? (int64_t)queries[x] : x;
  len = 0;
  bits = 0;
  if (s < 0 || s >= nq) {
    bits = 4u;
    return -1;
  }
  if (!q_off) return s;
  len = q_off[s + 1] - q_off[s];
  if (len > FD_MAXK) {
    bits = 1u;
    len = 0;
    return -1;
  }
  return s;
}

// the G bits of table row r (r inside [0, D)): bit g = request g of the workgroup holds r
__device__ static inline uint32_t fd_mask(const uint32_t *bits, uint32_t r, int G) {
  const uint32_t at = r * (uint32_t)G, w = bits[at >> 5];
  return G == 32 ? w : (w >> (at & 31)) & ((1u << G) - 1u);
}

// fd_mask of a row id as it comes from the CSR: one outside [0, D) raises flag bit 3 and is never tested
__device__ static inline uint32_t fd_test(const uint32_t *bits, uint32_t r, int64_t D, int G, uint32_t *flags) {
  if (r >= (uint64_t)D) {
    atomicOr(flags, 8u);
    return 0;
  }
  return fd_mask(bits, r, G);
}

// the rows of swept query j (none when j >= j1) and the lane's row ids of the first two trips over them
__device__ static inline void fd_fetch(const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t j,
                                       int64_t j1, int sub, int64_t &lo, int64_t &hi, uint32_t &r0, uint32_t &r1) {
  lo = hi = 0;
  r0 = r1 = 0;
  if (j < j1) {
    lo = off[j];
    hi = off[j + 1];
    if (lo + sub < hi) r0 = (uint32_t)rows[lo + sub];
    if (lo + FD_W + sub < hi) r1 = (uint32_t)rows[lo + FD_W + sub];
  }
}

// the bitmap of the answer sets of requests 0 .. ng - 1 (sid[g] = the chosen query, < 0: none) over bits[0, bitw), zeroed
// here; every thread of the workgroup calls it, the caller puts the barriers around it
__device__ static inline void fd_stage(const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t D, int G,
                                       const int32_t *sid, int ng, uint32_t *bits, uint32_t *flags) {
  const int tid = threadIdx.x;
  for (int g = 0; g < ng; ++g) {
    const int64_t s = sid[g];
    if (s < 0) continue;
    const int64_t lo = off[s], hi = off[s + 1];
    for (int64_t p = lo + tid; p < hi; p += FD_SWEEP_THREADS) {
      const uint32_t r = (uint32_t)rows[p];
      if (r >= (uint64_t)D) {
        atomicOr(flags, 8u);   // never set, never tested
      } else {
        const uint32_t at = r * (uint32_t)G + (uint32_t)g;
        atomicOr(&bits[at >> 5], 1u << (at & 31));
      }
    }
  }
}

// slices of the ids: the caller's, or (0) automatic
static inline int64_t fd_slices(int64_t groups, int64_t nq, int32_t slices) {
  if (slices > 0) return slices;
  int64_t S = FD_AUTO_BLOCKS / (groups > 0 ? groups : 1);
  const int64_t most = ceil_div64(nq, FD_MIN_SLICE);
  if (S > most) S = most;
  if (S > FD_MAXS) S = FD_MAXS;
  return S < 1 ? 1 : S;
}

}  // namespace
