// diversify.hip -- rerank served lists by the stored neighbour lists, and the redundancy of any served list
// (qrlsh_diversify, qrlsh_list_redundancy in include/qrlsh.h).  The project's own rule; integer arithmetic only.
//
// sim(a, b) = the largest stored milli among the list entries a -> b and b -> a, 0 when neither is stored.
// Per request a pool of n candidates (col, val) in served order; greedily, for t = 0 .. k - 1: among the unpicked
// candidates c with r_c = max over picked s of sim(c, s) below max_sim, take the one with the largest
// 1000 * val_c - penalty * r_c (int64), ties to the smaller pool position; stop when none is eligible.
//
// One 256-thread workgroup per request, two launches:
//   adjacency -- the pool's columns go into an LDS hash (2048 slots, <= 1024 keys); groups of 16 lanes walk the
//                candidates' list rows and look every neighbour up; the pool-internal edges, in both directions, become
//                a CSR in pool space in the workspace: a count per position in LDS, a scan, then the fill.  A half-edge
//                is one word: the other end's pool position (bits 0-9) and the milli value (bits 10-19);
//   select    -- r_c and the picked bit of every candidate in LDS, four candidates per thread; per step an argmax of
//                (score, -position) by wave shuffles then across the waves in LDS, and a walk of the pick's half-edges
//                alone that raises r with LDS max: a step costs the pick's pool degree;
//   grid      -- (qrlsh_diversify_grid) one adjacency per request, then a workgroup per (request, setting): the same
//                greedy loop (dv_select, the one copy), the picks held to the truth, and the in-list pairs folded out
//                of the POOL's adjacency by the picks' ranks -- no second adjacency;
//   reduce    -- (redundancy) the adjacency of the list itself, then per position the pairs towards later positions:
//                a wave folds the half-edges of a pair (one per stored direction) through a per-wave LDS row.
// Edges past the workspace's capacity raise a flag and none is written; nothing is read or written outside the
// request's pool, list rows and workspace slice.
#include "common.h"

namespace {
constexpr int DV_THREADS = 256;
constexpr int DV_WAVES = DV_THREADS / WAVE;
constexpr int DV_MAXN = QRLSH_DIVERSIFY_MAX_POOL;   // 1024 candidates: 10 bits of pool position
constexpr int DV_PER = DV_MAXN / DV_THREADS;        // candidates per thread
constexpr int DV_SLOTS = 2 * DV_MAXN;               // hash slots
constexpr int DV_GROUP = 16;                        // lanes that walk one list row together
constexpr int DV_MAX_MILLI = 1000;
constexpr int64_t DV_MAX_M = 1ll << 24;

constexpr uint32_t DV_BAD_NEIGHBOUR = 1, DV_BAD_CANDIDATE = 2, DV_DUPLICATE = 4, DV_OVERFLOW = 8;

static_assert(DV_MAXN == 1024 && DV_PER == 4, "a half-edge holds 10 bits of position; the select keeps 4 per thread");

struct DvAdjLds {
  int32_t key[DV_SLOTS];        // -1 = empty
  uint16_t key_pos[DV_SLOTS];   // pool position of the slot's key
  int64_t beg[DV_MAXN];         // list row of the candidate: first entry ...
  uint32_t len[DV_MAXN];        // ... and length (0: no row is walked)
  uint32_t cnt[DV_MAXN];        // half-edges per position, then the fill cursors
  uint32_t wsum[DV_WAVES];
};

__device__ __forceinline__ uint32_t dv_hash(int32_t col) { return ((uint32_t)col * 2654435761u) >> 21; }

// pool position of column d, -1 when it is not in the pool
__device__ __forceinline__ int dv_lookup(const DvAdjLds &s, int32_t d) {
  uint32_t slot = dv_hash(d);
  for (;;) {
    const int32_t key = s.key[slot];
    if (key == d) return s.key_pos[slot];
    if (key == -1) return -1;
    slot = (slot + 1) & (DV_SLOTS - 1);
  }
}

// f(c, q, milli) for every stored entry c -> q with both ends in the pool, c != q (positions); groups of DV_GROUP
// lanes take the candidates in turn.  Returns the flag bits met.
template <typename F>
__device__ __forceinline__ uint32_t dv_walk(const DvAdjLds &s, int n, int64_t nq, const int32_t *__restrict__ q_idx,
                                            const int32_t *__restrict__ q_milli, bool with_milli, F &&f) {
  uint32_t fl = 0;
  const int g = threadIdx.x / DV_GROUP, l = threadIdx.x % DV_GROUP;
  for (int c = g; c < n; c += DV_THREADS / DV_GROUP) {
    const uint32_t len = s.len[c];
    const int64_t beg = s.beg[c];
    for (uint32_t e = l; e < len; e += DV_GROUP) {
      const int32_t d = q_idx[beg + e];
      if (d < 0 || d >= nq) {
        fl |= DV_BAD_NEIGHBOUR;
        continue;
      }
      const int q = dv_lookup(s, d);
      if (q < 0 || q == c) continue;
      int32_t mi = with_milli ? q_milli[beg + e] : 0;
      mi = mi < 0 ? 0 : mi > DV_MAX_MILLI ? DV_MAX_MILLI : mi;
      f(c, q, (uint32_t)mi);
    }
  }
  return fl;
}

// The adjacency of one pool: cols[0 .. n) (n <= n_off <= DV_MAXN) -> offs[0 .. n_off] and at most `cap` half-edges.
// pad_ok: a column of -1 is an empty position (a padded list), not a bad candidate.  Every thread of the block calls it.
__device__ void dv_adjacency(DvAdjLds &s, const int32_t *__restrict__ cols, int n, int n_off, bool pad_ok, int64_t nq,
                             const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx,
                             const int32_t *__restrict__ q_milli, uint32_t cap, uint32_t *__restrict__ offs,
                             uint32_t *__restrict__ edges, uint32_t *__restrict__ flag) {
  const int tid = threadIdx.x;
  for (int i = tid; i < DV_SLOTS; i += DV_THREADS) s.key[i] = -1;
  __syncthreads();
  uint32_t fl = 0;
  for (int c = tid; c < DV_MAXN; c += DV_THREADS) {
    int64_t beg = 0;
    uint32_t len = 0;
    if (c < n) {
      const int32_t col = cols[c];
      if (col >= 0 && col < nq) {
        uint32_t slot = dv_hash(col);
        bool mine = false;
        for (;;) {
          const int32_t old = atomicCAS(&s.key[slot], -1, col);
          if (old == -1) {
            s.key_pos[slot] = (uint16_t)c;
            mine = true;
            break;
          }
          if (old == col) {
            fl |= DV_DUPLICATE;
            break;
          }
          slot = (slot + 1) & (DV_SLOTS - 1);
        }
        if (mine) {
          beg = q_off[col];
          const int64_t L = q_off[col + 1] - beg;
          if (L < 0 || L > 0x7FFFFFFFll) fl |= DV_OVERFLOW;
          else len = (uint32_t)L;
        }
      } else if (!(pad_ok && col == -1)) {
        fl |= DV_BAD_CANDIDATE;
      }
    }
    s.beg[c] = beg;
    s.len[c] = len;
    s.cnt[c] = 0;
  }
  __syncthreads();
  fl |= dv_walk(s, n, nq, q_idx, q_milli, false, [&](int c, int q, uint32_t) {
    atomicAdd(&s.cnt[c], 1u);
    atomicAdd(&s.cnt[q], 1u);
  });
  __syncthreads();
  // thread t scans positions 4 t .. 4 t + 3; counts saturate far above any capacity
  uint32_t own[DV_PER], sum = 0;
#pragma unroll
  for (int j = 0; j < DV_PER; ++j) {
    own[j] = min(s.cnt[DV_PER * tid + j], 1u << 21);
    sum += own[j];
  }
  uint32_t total;
  uint32_t run = block_excl_scan<DV_THREADS>(sum, s.wsum, total);
  const bool fits = total <= cap;
  if (!fits) fl |= DV_OVERFLOW;
#pragma unroll
  for (int j = 0; j < DV_PER; ++j) {
    const int p = DV_PER * tid + j;
    if (p <= n_off) offs[p] = fits ? run : 0u;
    s.cnt[p] = run;
    run += own[j];
  }
  if (tid == DV_THREADS - 1 && n_off == DV_MAXN) offs[DV_MAXN] = fits ? total : 0u;
  __syncthreads();
  if (fits && total > 0) {
    dv_walk(s, n, nq, q_idx, q_milli, true, [&](int c, int q, uint32_t mi) {
      const uint32_t a = atomicAdd(&s.cnt[c], 1u), b = atomicAdd(&s.cnt[q], 1u);
      if (a < cap) edges[a] = (uint32_t)q | mi << 10;
      if (b < cap) edges[b] = (uint32_t)c | mi << 10;
    });
  }
  if (fl) atomicOr(flag, fl);
}

// workspace of one request: [offs: n_off + 1 words, rounded to 4][half-edges: cap words]
__host__ __device__ inline size_t dv_offs_words(int n_off) { return ((size_t)n_off + 1 + 3) & ~(size_t)3; }

__global__ __launch_bounds__(DV_THREADS) void diversify_adjacency_kernel(
    const int32_t *__restrict__ cand_idx, const int32_t *__restrict__ avail, int N, int64_t nq,
    const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli,
    uint32_t cap, uint32_t *__restrict__ ws, uint32_t *__restrict__ flag) {
  __shared__ DvAdjLds s;
  const int64_t x = blockIdx.x;
  const int32_t av = avail[x];
  const int n = av < 0 ? 0 : av > N ? N : av;
  uint32_t *offs = ws + (size_t)x * (dv_offs_words(N) + cap);
  dv_adjacency(s, cand_idx + x * N, n, N, false, nq, q_off, q_idx, q_milli, cap, offs, offs + dv_offs_words(N), flag);
}

__global__ __launch_bounds__(DV_THREADS) void list_adjacency_kernel(
    const int32_t *__restrict__ idx, int k, int64_t nq, const int64_t *__restrict__ q_off,
    const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli, uint32_t cap, uint32_t *__restrict__ ws,
    uint32_t *__restrict__ flag) {
  __shared__ DvAdjLds s;
  const int64_t x = blockIdx.x;
  uint32_t *offs = ws + (size_t)x * (dv_offs_words(k) + cap);
  dv_adjacency(s, idx + x * k, k, k, true, nq, q_off, q_idx, q_milli, cap, offs, offs + dv_offs_words(k), flag);
}

__device__ __forceinline__ uint64_t dv_wave_max(uint64_t v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
    const uint64_t o = __shfl_xor(v, d, WAVE);
    v = o > v ? o : v;
  }
  return v;
}

struct DvSelLds {
  uint32_t r[DV_MAXN];          // r_c, bit 31 = picked
  uint32_t offs[DV_MAXN + 1];
  uint32_t picks[DV_MAXN];      // position | r << 10 of every pick
  uint64_t wmax[2][DV_WAVES];
};

// The greedy loop over the adjacency (offs, edges) of a pool of n candidates with values vals[0 .. n): the one copy of
// the rule.  Every thread of the block calls it; -> the picks t, the same in every thread, s.picks[0 .. t) filled and
// visible to the block on return.
__device__ __forceinline__ int dv_select(DvSelLds &s, const int32_t *__restrict__ vals, int n, int N, int k,
                                         int64_t penalty, uint32_t max_sim, const uint32_t *__restrict__ offs,
                                         const uint32_t *__restrict__ edges) {
  const int tid = threadIdx.x;
  int64_t base[DV_PER];   // 1000 * val of positions tid + 256 j
#pragma unroll
  for (int j = 0; j < DV_PER; ++j) {
    const int p = tid + DV_THREADS * j;
    base[j] = p < n ? 1000ll * (int64_t)vals[p] : 0;
    s.r[p] = 0;
    if (p <= N) s.offs[p] = offs[p];
  }
  if (tid == 0 && N == DV_MAXN) s.offs[DV_MAXN] = offs[DV_MAXN];
  __syncthreads();
  int t = 0;
  for (; t < k; ++t) {
    // key = (score + 2^43) << 10 | (1023 - position) > 0; |score| < 2^42 + 2^30
    uint64_t best = 0;
#pragma unroll
    for (int j = 0; j < DV_PER; ++j) {
      const int p = tid + DV_THREADS * j;
      const uint32_t rc = s.r[p];
      if (p < n && rc < max_sim) {   // a picked candidate has bit 31 set
        const int64_t score = base[j] - penalty * (int64_t)rc;
        const uint64_t key = (uint64_t)(score + (1ll << 43)) << 10 | (uint64_t)(DV_MAXN - 1 - p);
        best = key > best ? key : best;
      }
    }
    best = dv_wave_max(best);
    if (lane_id() == 0) s.wmax[t & 1][tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DV_WAVES; ++w) {
      const uint64_t o = s.wmax[t & 1][w];
      best = o > best ? o : best;
    }
    if (best == 0) break;   // nobody is eligible: the same word in every thread
    const int p = DV_MAXN - 1 - (int)(best & (DV_MAXN - 1));
    if (tid == 0) {   // the keys were read before the barrier, and no half-edge of p points at p
      const uint32_t rp = s.r[p];
      s.picks[t] = (uint32_t)p | rp << 10;
      s.r[p] = rp | 0x80000000u;
    }
    for (uint32_t e = s.offs[p] + tid, end = s.offs[p + 1]; e < end; e += DV_THREADS) {
      const uint32_t he = edges[e];
      atomicMax(&s.r[he & (DV_MAXN - 1)], he >> 10);
    }
    __syncthreads();
  }
  // t picks (the same in every thread); `picks` was written by thread 0 before the last barrier passed
  __syncthreads();
  return t;
}

// the greedy selection over the adjacency of diversify_adjacency_kernel
__global__ __launch_bounds__(DV_THREADS) void diversify_select_kernel(
    const int32_t *__restrict__ cand_idx, const int32_t *__restrict__ cand_val, const int32_t *__restrict__ avail, int N,
    int k, int64_t penalty, uint32_t max_sim, uint32_t cap, const uint32_t *__restrict__ ws,
    int32_t *__restrict__ idx_out, int32_t *__restrict__ val_out, int32_t *__restrict__ red_out,
    int32_t *__restrict__ count_out) {
  __shared__ DvSelLds s;
  const int tid = threadIdx.x;
  const int64_t x = blockIdx.x;
  const int32_t av = avail[x];
  const int n = av < 0 ? 0 : av > N ? N : av;
  const uint32_t *offs = ws + (size_t)x * (dv_offs_words(N) + cap);
  const int t = dv_select(s, cand_val + x * N, n, N, k, penalty, max_sim, offs, offs + dv_offs_words(N));
  for (int j = tid; j < k; j += DV_THREADS) {
    const bool in = j < t;
    const uint32_t w = in ? s.picks[j] : 0;
    const int p = (int)(w & (DV_MAXN - 1));
    idx_out[x * k + j] = in ? cand_idx[x * N + p] : -1;
    val_out[x * k + j] = in ? cand_val[x * N + p] : 0;
    red_out[x * k + j] = in ? (int32_t)(w >> 10) : 0;
  }
  if (tid == 0) count_out[x] = t;
}

// The selection under S settings over ONE adjacency per request, each list held to the truth and to the pool's
// adjacency: workgroup (x, s) = (request, setting).  After the loop the picks' truth is gathered (at most four picks per
// thread), and a wave per pick folds that pick's half-edges towards later-ranked picks through a per-wave LDS row, as
// list_redundancy_reduce_kernel does over a list's own adjacency: a pair stored in both directions counts once, at the
// larger milli.  The rank of every pool position in the list is kept in LDS (DV_NO_RANK: not picked).
constexpr uint32_t DV_BAD_SETTING = 16, DV_BAD_USER = 32, DV_BAD_GAIN = 64;
constexpr int DV_LINE = 12, DV_TOTALS = 24;
constexpr uint16_t DV_NO_RANK = 0xFFFF;

__global__ __launch_bounds__(DV_THREADS) void diversify_grid_select_kernel(
    const int32_t *__restrict__ cand_idx, const int32_t *__restrict__ cand_val, const int32_t *__restrict__ avail,
    int64_t m, int N, int64_t nq, int k, const int64_t *__restrict__ penalties, const int32_t *__restrict__ max_sims,
    const int32_t *__restrict__ truth, int64_t nu, const int32_t *__restrict__ users, int32_t relevant,
    const int64_t *__restrict__ gain, const int64_t *__restrict__ gain_prefix,
    const int64_t *__restrict__ request_counts, uint32_t cap, const uint32_t *__restrict__ ws,
    int32_t *__restrict__ idx_out, int32_t *__restrict__ val_out, int32_t *__restrict__ red_out,
    int32_t *__restrict__ count_out, int64_t *__restrict__ per_request_out, unsigned long long *__restrict__ totals_out,
    uint32_t *__restrict__ flag) {
  __shared__ DvSelLds s;
  __shared__ uint32_t fold[DV_WAVES][DV_MAXN];   // per wave: the largest milli towards each later-ranked pick; 0 between picks
  __shared__ uint16_t rank[DV_MAXN];             // the pick step of a pool position
  __shared__ unsigned long long acc[6];          // hits, known, dcg, sum red, pairs, sum sim
  __shared__ uint32_t acc_first, acc_max, acc_moved;
  const int tid = threadIdx.x, w = tid >> 6, lane = lane_id();
  const int64_t x = blockIdx.x, st = blockIdx.y;
  const int32_t av = avail[x];
  const int64_t penalty = penalties[st];
  const int32_t ms = max_sims[st];
  uint32_t fl = 0;
  if (penalty < 0 || penalty > QRLSH_DIVERSIFY_MAX_PENALTY || ms < 0 || ms > DV_MAX_MILLI + 1) fl |= DV_BAD_SETTING;
  int64_t u = 0;
  if (truth) {
    u = users ? (int64_t)users[x] : x;
    if (u < 0 || u >= nu) fl |= DV_BAD_USER;
    if (x == 0 && st == 0)
      for (int j = tid; j < k; j += DV_THREADS)
        if (gain[j] < 0) atomicOr(flag, DV_BAD_GAIN);
  }
  if (fl && tid == 0) atomicOr(flag, fl);
  const bool good = !(fl & DV_BAD_SETTING), served = good && av >= 0 && !(fl & DV_BAD_USER);
  const int n = !served ? 0 : av > N ? N : av;
  for (int i = tid; i < DV_WAVES * DV_MAXN; i += DV_THREADS) (&fold[0][0])[i] = 0;
  for (int p = tid; p < DV_MAXN; p += DV_THREADS) rank[p] = DV_NO_RANK;
  if (tid == 0) {
    acc[0] = acc[1] = acc[2] = acc[3] = acc[4] = acc[5] = 0;
    acc_first = 0xFFFFFFFFu;
    acc_max = acc_moved = 0;
  }
  const uint32_t *offs = ws + (size_t)x * (dv_offs_words(N) + cap);
  const uint32_t *edges = offs + dv_offs_words(N);
  // the barriers inside order the initialisation above before everything below
  const int t = dv_select(s, cand_val + x * N, n, N, k, good ? penalty : 0, good ? (uint32_t)ms : 0u, offs, edges);
  const int64_t row = st * m + x;
  // the lists, and the picks held to the truth
  uint32_t hits = 0, known = 0, first = 0xFFFFFFFFu, moved = 0;
  unsigned long long dcg = 0, red = 0;
  for (int j = tid; j < k; j += DV_THREADS) {
    const bool in = j < t;
    const uint32_t pw = in ? s.picks[j] : 0;
    const int p = (int)(pw & (DV_MAXN - 1));
    const int32_t col = in ? cand_idx[x * N + p] : -1;
    if (idx_out) idx_out[row * k + j] = col;
    if (val_out) val_out[row * k + j] = in ? cand_val[x * N + p] : 0;
    if (red_out) red_out[row * k + j] = (int32_t)(pw >> 10);
    if (!in) continue;
    rank[p] = (uint16_t)j;
    red += pw >> 10;
    moved |= p != j;
    if (truth && col >= 0 && col < nq) {   // a column outside the lists' range was flagged by the adjacency
      const int32_t tv = truth[u * nq + col];
      known += tv != 0;
      if (tv >= relevant) {
        ++hits;
        dcg += (unsigned long long)gain[j];
        first = min(first, (uint32_t)j + 1);
      }
    }
  }
  if (red) atomicAdd(&acc[3], red);
  if (moved) atomicOr(&acc_moved, 1u);
  if (known) atomicAdd(&acc[1], (unsigned long long)known);
  if (hits) {
    atomicAdd(&acc[0], (unsigned long long)hits);
    atomicAdd(&acc[2], dcg);
    atomicMin(&acc_first, first);
  }
  __syncthreads();
  // the in-list pairs, from the pool's adjacency: pick j's half-edges towards the picks ranked after it
  uint32_t pairs = 0, largest = 0;
  unsigned long long sum = 0;
  for (int j = w; j < t; j += DV_WAVES) {
    const int p = (int)(s.picks[j] & (DV_MAXN - 1));
    const uint32_t beg = s.offs[p], end = s.offs[p + 1];
    if (beg == end) continue;
    for (uint32_t e = beg + lane; e < end; e += WAVE) {
      const uint32_t he = edges[e], q = he & (DV_MAXN - 1), rq = rank[q];
      if (rq != DV_NO_RANK && (int)rq > j) atomicMax(&fold[w][q], he >> 10);
    }
    // one wave: its LDS operations complete in program order; the fence keeps the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t e = beg + lane; e < end; e += WAVE) {
      const uint32_t he = edges[e], q = he & (DV_MAXN - 1), rq = rank[q];
      if (rq != DV_NO_RANK && (int)rq > j) {
        const uint32_t sim = atomicExch(&fold[w][q], 0u);   // the first half-edge of a pair takes it and clears the slot
        if (sim > 0) {
          ++pairs;
          sum += sim;
          largest = max(largest, sim);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (pairs) {
    atomicAdd(&acc[4], (unsigned long long)pairs);
    atomicAdd(&acc[5], sum);
    atomicMax(&acc_max, largest);
  }
  __syncthreads();
  if (tid != 0) return;
  if (count_out) count_out[row] = t;
  const int full = k < n ? k : n;
  int64_t line[DV_LINE] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (served) {
    line[0] = t;
    line[1] = (int64_t)acc[0];
    line[2] = (int64_t)acc[1];
    line[3] = acc_first == 0xFFFFFFFFu ? 0 : (int64_t)acc_first;
    line[4] = (int64_t)acc[2];
    if (truth && request_counts) {
      line[5] = request_counts[2 * x];
      line[6] = request_counts[2 * x + 1];
    }
    line[8] = (int64_t)acc[4];
    line[9] = (int64_t)acc[5];
    line[10] = (int64_t)acc_max;
    line[11] = (int64_t)acc[3];
  }
  if (good) line[7] = av;
  if (per_request_out) {
#pragma unroll
    for (int i = 0; i < DV_LINE; ++i) per_request_out[row * DV_LINE + i] = line[i];
  }
  if (!served) return;
  unsigned long long *tot = totals_out + st * DV_TOTALS;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (line[i]) atomicAdd(&tot[i], (unsigned long long)line[i]);
  atomicAdd(&tot[8], 1ull);
  if (truth) {
    if (line[5] > 0) atomicAdd(&tot[9], 1ull);
    if (line[1] > 0) atomicAdd(&tot[10], 1ull);
    const int64_t rel = line[5] < 0 ? 0 : line[5] > k ? k : line[5];
    if (gain_prefix[rel]) atomicAdd(&tot[11], (unsigned long long)gain_prefix[rel]);
  }
  if (line[8]) {
    atomicAdd(&tot[12], (unsigned long long)line[8]);
    atomicAdd(&tot[13], (unsigned long long)line[9]);
    atomicMax(&tot[14], (unsigned long long)line[10]);
  }
  if (line[11]) atomicAdd(&tot[15], (unsigned long long)line[11]);
  if (acc_moved || t < full) atomicAdd(&tot[16], 1ull);
  if (t < full) atomicAdd(&tot[17], 1ull);
}

// words[x] = {entries listed, pairs with sim > 0, sum of sim over them, largest sim}; totals += / max
__global__ __launch_bounds__(DV_THREADS) void list_redundancy_reduce_kernel(
    const int32_t *__restrict__ idx, int k, uint32_t cap, const uint32_t *__restrict__ ws, int64_t *__restrict__ words,
    unsigned long long *__restrict__ totals) {
  __shared__ uint32_t fold[DV_WAVES][DV_MAXN];   // per wave: the largest milli towards each later position; 0 between rows
  __shared__ uint32_t offs_s[DV_MAXN + 1];
  __shared__ unsigned long long acc[3];
  __shared__ uint32_t acc_max;
  const int tid = threadIdx.x, w = tid >> 6, lane = lane_id();
  const int64_t x = blockIdx.x;
  const uint32_t *offs = ws + (size_t)x * (dv_offs_words(k) + cap);
  const uint32_t *edges = offs + dv_offs_words(k);
  uint32_t listed = 0;
  for (int p = tid; p < DV_MAXN + 1; p += DV_THREADS) {
    if (p <= k) offs_s[p] = offs[p];
    if (p < k && idx[x * k + p] != -1) ++listed;
  }
  for (int i = tid; i < DV_WAVES * DV_MAXN; i += DV_THREADS) (&fold[0][0])[i] = 0;
  if (tid == 0) {
    acc[0] = acc[1] = acc[2] = 0;
    acc_max = 0;
  }
  __syncthreads();
  uint32_t pairs = 0, largest = 0;
  unsigned long long sum = 0;
  for (int p = w; p < k; p += DV_WAVES) {
    const uint32_t beg = offs_s[p], end = offs_s[p + 1];
    if (beg == end) continue;
    for (uint32_t e = beg + lane; e < end; e += WAVE) {
      const uint32_t he = edges[e], q = he & (DV_MAXN - 1);
      if ((int)q > p) atomicMax(&fold[w][q], he >> 10);
    }
    // one wave: its LDS operations complete in program order; the fence keeps the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t e = beg + lane; e < end; e += WAVE) {
      const uint32_t he = edges[e], q = he & (DV_MAXN - 1);
      if ((int)q > p) {
        const uint32_t sim = atomicExch(&fold[w][q], 0u);   // the first half-edge of a pair takes it and clears the slot
        if (sim > 0) {
          ++pairs;
          sum += sim;
          largest = max(largest, sim);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (listed) atomicAdd(&acc[0], (unsigned long long)listed);
  if (pairs) {
    atomicAdd(&acc[1], (unsigned long long)pairs);
    atomicAdd(&acc[2], sum);
    atomicMax(&acc_max, largest);
  }
  __syncthreads();
  if (tid == 0) {
    words[4 * x + 0] = (int64_t)acc[0];
    words[4 * x + 1] = (int64_t)acc[1];
    words[4 * x + 2] = (int64_t)acc[2];
    words[4 * x + 3] = (int64_t)acc_max;
    if (acc[0]) atomicAdd(&totals[0], acc[0]);
    if (acc[1]) {
      atomicAdd(&totals[1], acc[1]);
      atomicAdd(&totals[2], acc[2]);
      atomicMax(&totals[3], (unsigned long long)acc_max);
    }
  }
}

// half-edges per request that every well-formed pool of N with rows up to max_row needs at most
uint32_t dv_cap_for(int64_t N, int64_t max_row) {
  const int64_t per = max_row < N - 1 ? max_row : N - 1;
  const int64_t cap = 2 * N * (per > 0 ? per : 0);
  return (uint32_t)((cap + 3) & ~3ll);
}

// workspace: a slice per request, [offs: dv_offs_words(N)][half-edges: cap] (the kernels find theirs by the same rule)
uint32_t *dv_layout(QrCarve &c, int64_t m, int N, uint32_t cap) {
  return c.take<uint32_t>((size_t)m * (dv_offs_words(N) + cap), 4);
}

// the checks of a workspace of `bytes` for m > 0 requests; *cap = the half-edges it gives each of them (never above
// what any pool of N can hold; QRLSH_EWORKSPACE when not even the offsets fit)
int dv_workspace(const char *who, void *workspace, size_t bytes, int64_t m, int N, uint32_t *cap, uint32_t **ws) {
  QR_CHECK_ALIGNED(who, "the workspace", qr_addr(workspace), 16);
  QrCarve least(nullptr);
  dv_layout(least, m, N, 0);
  QR_CHECK_WORKSPACE(who, workspace, bytes, least.bytes());
  const size_t most = dv_cap_for(N, N), got = (bytes / sizeof(uint32_t) / (size_t)m - dv_offs_words(N)) & ~(size_t)3;
  *cap = (uint32_t)(got < most ? got : most);
  QrCarve c(workspace);
  *ws = dv_layout(c, m, N, *cap);
  return QRLSH_OK;
}
}  // namespace

QRLSH_EXPORT size_t qrlsh_diversify_workspace_bytes(int64_t m, int32_t N, int64_t max_row) {
  if (m <= 0 || m > DV_MAX_M || N < 1 || N > DV_MAXN || max_row < 0) return 0;
  return QR_LAYOUT_BYTES(dv_layout, m, N, dv_cap_for(N, max_row));
}

QRLSH_EXPORT int qrlsh_diversify(const int32_t *cand_idx, const int32_t *cand_val, const int32_t *avail, int64_t m,
                                 int32_t N, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                                 const int32_t *q_milli, int32_t k, int64_t penalty, int32_t max_sim, int32_t *idx_out,
                                 int32_t *val_out, int32_t *red_out, int32_t *count_out, uint32_t *flag_out,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(N >= 1 && N <= DV_MAXN, "qrlsh_diversify: N=%d outside 1..%d", N, DV_MAXN);
  QR_CHECK_ARG(k >= 1 && k <= N, "qrlsh_diversify: k=%d outside 1..N=%d", k, N);
  QR_CHECK_ARG(penalty >= 0 && penalty <= QRLSH_DIVERSIFY_MAX_PENALTY, "qrlsh_diversify: penalty=%lld outside 0..%d",
               (long long)penalty, QRLSH_DIVERSIFY_MAX_PENALTY);
  QR_CHECK_ARG(max_sim >= 0 && max_sim <= 1001, "qrlsh_diversify: max_sim=%d outside 0..1001", max_sim);
  QR_CHECK_ARG(m >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_diversify: bad sizes m=%lld nq=%lld", (long long)m,
               (long long)nq);
  QR_CHECK_ARG(flag_out, "qrlsh_diversify: flag_out is required");
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(cand_idx && cand_val && avail && idx_out && val_out && red_out && count_out,
               "qrlsh_diversify: null pointer");
  QR_CHECK_ARG(q_off && (nq == 0 || (q_idx && q_milli)), "qrlsh_diversify: null pointer among the lists");
  if (m > DV_MAX_M) {
    qrlsh_set_error("qrlsh_diversify: m=%lld above the %lld workgroups served", (long long)m, (long long)DV_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  uint32_t cap = 0, *ws = nullptr;
  const int wrc = dv_workspace("qrlsh_diversify", workspace, workspace_bytes, m, N, &cap, &ws);
  if (wrc != QRLSH_OK) return wrc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_LAUNCH("diversify_adjacency", diversify_adjacency_kernel, dim3((unsigned)m), dim3(DV_THREADS), 0, st, cand_idx,
            avail, (int)N, nq, q_off, q_idx, q_milli, cap, ws, flag_out);
  QR_LAUNCH("diversify_select", diversify_select_kernel, dim3((unsigned)m), dim3(DV_THREADS), 0, st, cand_idx, cand_val,
            avail, (int)N, (int)k, penalty, (uint32_t)max_sim, cap, (const uint32_t *)ws, idx_out, val_out, red_out,
            count_out);
  QR_LAUNCH_CHECK("qrlsh_diversify");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_diversify_grid(const int32_t *cand_idx, const int32_t *cand_val, const int32_t *avail, int64_t m,
                                      int32_t N, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                                      const int32_t *q_milli, int32_t k, const int64_t *penalties,
                                      const int32_t *max_sims, int32_t S, const int32_t *truth, int64_t nu,
                                      const int32_t *users, int32_t relevant, const int64_t *gain,
                                      const int64_t *gain_prefix, const int64_t *request_counts, int32_t *idx_out,
                                      int32_t *val_out, int32_t *red_out, int32_t *count_out, int64_t *per_request_out,
                                      int64_t *totals_out, uint32_t *flag_out, void *workspace, size_t workspace_bytes,
                                      void *stream) {
  QR_CHECK_ARG(N >= 1 && N <= DV_MAXN, "qrlsh_diversify_grid: N=%d outside 1..%d", N, DV_MAXN);
  QR_CHECK_ARG(k >= 1 && k <= N, "qrlsh_diversify_grid: k=%d outside 1..N=%d", k, N);
  QR_CHECK_ARG(S >= 1 && S <= QRLSH_GRID_MAX_SETTINGS, "qrlsh_diversify_grid: S=%d outside 1..%d", S,
               QRLSH_GRID_MAX_SETTINGS);
  QR_CHECK_ARG(m >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_diversify_grid: bad sizes m=%lld nq=%lld", (long long)m,
               (long long)nq);
  QR_CHECK_ARG(flag_out && totals_out, "qrlsh_diversify_grid: flag_out and totals_out are required");
  QR_CHECK_ARG(penalties && max_sims, "qrlsh_diversify_grid: the settings are required");
  if (truth) {
    QR_CHECK_ARG(nu >= 0 && nu <= 2147483647ll, "qrlsh_diversify_grid: bad size nu=%lld", (long long)nu);
    QR_CHECK_ARG(relevant >= 1, "qrlsh_diversify_grid: relevant=%d below 1", relevant);
    QR_CHECK_ARG(gain && gain_prefix, "qrlsh_diversify_grid: scoring needs gain and gain_prefix");
  }
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(cand_idx && cand_val && avail, "qrlsh_diversify_grid: null pointer");
  QR_CHECK_ARG(q_off && (nq == 0 || (q_idx && q_milli)), "qrlsh_diversify_grid: null pointer among the lists");
  if (m > DV_MAX_M) {
    qrlsh_set_error("qrlsh_diversify_grid: m=%lld above the %lld requests served", (long long)m, (long long)DV_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  uint32_t cap = 0, *ws = nullptr;
  const int wrc = dv_workspace("qrlsh_diversify_grid", workspace, workspace_bytes, m, N, &cap, &ws);
  if (wrc != QRLSH_OK) return wrc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_LAUNCH("diversify_adjacency", diversify_adjacency_kernel, dim3((unsigned)m), dim3(DV_THREADS), 0, st, cand_idx,
            avail, (int)N, nq, q_off, q_idx, q_milli, cap, ws, flag_out);
  QR_LAUNCH("diversify_grid_select", diversify_grid_select_kernel, dim3((unsigned)m, (unsigned)S), dim3(DV_THREADS), 0,
            st, cand_idx, cand_val, avail, m, (int)N, nq, (int)k, penalties, max_sims, truth, nu, users, relevant, gain,
            gain_prefix, request_counts, cap, (const uint32_t *)ws, idx_out, val_out, red_out, count_out,
            per_request_out, reinterpret_cast<unsigned long long *>(totals_out), flag_out);
  QR_LAUNCH_CHECK("qrlsh_diversify_grid");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_list_redundancy(const int32_t *idx, int64_t m, int32_t k, int64_t nq, const int64_t *q_off,
                                       const int32_t *q_idx, const int32_t *q_milli, int64_t *words_out,
                                       int64_t *totals_out, uint32_t *flag_out, void *workspace, size_t workspace_bytes,
                                       void *stream) {
  QR_CHECK_ARG(k >= 1 && k <= DV_MAXN, "qrlsh_list_redundancy: k=%d outside 1..%d", k, DV_MAXN);
  QR_CHECK_ARG(m >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_list_redundancy: bad sizes m=%lld nq=%lld",
               (long long)m, (long long)nq);
  QR_CHECK_ARG(flag_out && totals_out, "qrlsh_list_redundancy: flag_out and totals_out are required");
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(idx && words_out, "qrlsh_list_redundancy: null pointer");
  QR_CHECK_ARG(q_off && (nq == 0 || (q_idx && q_milli)), "qrlsh_list_redundancy: null pointer among the lists");
  if (m > DV_MAX_M) {
    qrlsh_set_error("qrlsh_list_redundancy: m=%lld above the %lld workgroups served", (long long)m,
                    (long long)DV_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  uint32_t cap = 0, *ws = nullptr;
  const int wrc = dv_workspace("qrlsh_list_redundancy", workspace, workspace_bytes, m, k, &cap, &ws);
  if (wrc != QRLSH_OK) return wrc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_LAUNCH("list_adjacency", list_adjacency_kernel, dim3((unsigned)m), dim3(DV_THREADS), 0, st, idx, (int)k, nq, q_off,
            q_idx, q_milli, cap, ws, flag_out);
  QR_LAUNCH("list_redundancy_reduce", list_redundancy_reduce_kernel, dim3((unsigned)m), dim3(DV_THREADS), 0, st, idx,
            (int)k, cap, (const uint32_t *)ws, words_out, reinterpret_cast<unsigned long long *>(totals_out));
  QR_LAUNCH_CHECK("qrlsh_list_redundancy");
  return QRLSH_OK;
}
