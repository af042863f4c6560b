// topk.hip -- a5 tail, select form: per-query top-K without sorting the directed edges.
//
// Reference: the per-query cut argsort(values)[::-1][:K], recommender.py:206-210.
//
// The sort form (qrlsh_topk_count / _fill, pairs.hip) orders all 2n directed edge keys on (src, 1000 - milli): ceil((id_bits + 11) / 8) radix
// passes over 2n words.  But the forward edges (src = i) ARE the scored pair list, already grouped by src and
// ordered by dst; only the n reverse edges (src = j) have to be brought together, and for that a stable sort on
// j's bits alone is enough (ceil(id_bits / 8) passes over n words -- under a third of the key-passes).  A query's
// neighbours are then two runs, [fstart[q], fstart[q+1]) of the pairs and [rstart[q], rstart[q+1]) of the sorted
// reverse words, and every directed edge finds its rank in its query's list by counting the edges of those two
// runs that order before it (value descending, then neighbour id ascending) -- stopping as soon as K of them
// have been seen.  Edge of rank r < K goes to out[off[q] + r], off = exclusive scan of min(K, list length): the
// output is the same (src, value desc, dst asc) COO the sort form writes, bit for bit.  Three kernels by list
// length: up to 16 neighbours (almost every query) a 16-lane group per query ranks by rotating the keys round
// its DPP row; 17 .. 64 a wave per query; longer lists a wave per query with a histogram of the 2001 possible
// values (O(length), see below).
// Reverse words: packed  j << (id_bits + 11) | inv << id_bits | i  (rdst == NULL), or key + payload
// (j << 11 | inv, i) for ids that do not fit.
#include "common.h"

#include <type_traits>

__device__ static inline uint32_t rev_src(uint64_t w, int id_bits, bool wide) {
  return (uint32_t)(wide ? w >> 11 : w >> (id_bits + 11));
}

// start[q] = first position of `a` whose src is >= q (q = 0 .. nq); a is ordered by src.  blockIdx.y = 0: a = the
// pairs, src = i -> fstart; 1: a = the sorted reverse words, src = j -> rstart.  The thread at a change of src
// fills the (usually 1 - 2) entries up to its src; a long stretch of queries without any edge (the ids beyond
// the last i, below the first j, ...) is left at SEL_UNSET for edge_bounds_fix_kernel, whose threads find their
// entry by binary search -- one thread walking a million-entry gap was the whole cost of this step.
// A thread takes EB_RUN consecutive words (16-byte loads) and walks the changes of src inside them: one thread per
// word read every word twice, 8 bytes at a time, and ran at under half the rate of the streaming kernels here.
constexpr uint32_t SEL_UNSET = 0xFFFFFFFFu;  // n < 2^31: never a position
constexpr int SEL_GAP = 32;
constexpr int EB_RUN = 4;   // (even: the loads are pairs of words)
__device__ static inline int64_t edge_src(const uint64_t *__restrict__ a, int64_t t, bool fwd, int id_bits, bool wide) {
  return (int64_t)(fwd ? (uint32_t)(a[t] >> 32) : rev_src(a[t], id_bits, wide));
}
__global__ __launch_bounds__(256) void edge_bounds_kernel(const uint64_t *__restrict__ pairs,
                                                          const uint64_t *__restrict__ rev, int64_t n, int64_t nq,
                                                          int id_bits, int wide, uint32_t *__restrict__ fstart,
                                                          uint32_t *__restrict__ rstart, int y0 = 0) {
  const bool fwd = blockIdx.y + y0 == 0;  // (y0 = 1: reverse words only, no forward list)
  const uint64_t *a = fwd ? pairs : rev;
  uint32_t *start = fwd ? fstart : rstart;
  const bool w = wide != 0;
  // positions t0 .. t0 + EB_RUN - 1 of 0 .. n (position n stands for the end: src = nq)
  const int64_t t0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * EB_RUN;
  uint64_t x[EB_RUN];
  if (t0 + EB_RUN <= n && ((uintptr_t)a & 15) == 0) {   // whole run inside the list: 16-byte loads
    const ulonglong2 *v = reinterpret_cast<const ulonglong2 *>(a + t0);
#pragma unroll
    for (int k = 0; k < EB_RUN; k += 2) {
      const ulonglong2 u = v[k >> 1];
      x[k] = u.x;
      x[k + 1] = u.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < EB_RUN; ++k) x[k] = t0 + k < n ? a[t0 + k] : 0ull;
  }
  int64_t s[EB_RUN];
#pragma unroll
  for (int k = 0; k < EB_RUN; ++k)
    s[k] = t0 + k < n ? (int64_t)(fwd ? (uint32_t)(x[k] >> 32) : rev_src(x[k], id_bits, w)) : nq;
  // the src in front of the run: the neighbouring lane's last, one more load for the first lane of a wave
  int64_t p = __shfl_up(s[EB_RUN - 1], 1, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) p = t0 > 0 && t0 <= n ? edge_src(a, t0 - 1, fwd, id_bits, w) : -1;
#pragma unroll
  for (int k = 0; k < EB_RUN; ++k) {
    const int64_t t = t0 + k;
    if (t > n) break;
    if (s[k] - p > SEL_GAP) {
      if (s[k] <= nq) start[s[k]] = (uint32_t)t;  // the entry of s itself; the stretch below it stays unset
    } else {
      for (int64_t q = p + 1; q <= s[k] && q <= nq; ++q) start[q] = (uint32_t)t;
    }
    p = s[k];
  }
}

__global__ __launch_bounds__(256) void edge_bounds_fix_kernel(const uint64_t *__restrict__ pairs,
                                                              const uint64_t *__restrict__ rev, int64_t n, int64_t nq,
                                                              int id_bits, int wide, uint32_t *__restrict__ fstart,
                                                              uint32_t *__restrict__ rstart, int y0 = 0) {
  const bool fwd = blockIdx.y + y0 == 0;
  const uint64_t *a = fwd ? pairs : rev;
  uint32_t *start = fwd ? fstart : rstart;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > nq || start[q] != SEL_UNSET) return;
  int64_t lo = 0, hi = n;  // first position whose src is >= q
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (edge_src(a, mid, fwd, id_bits, wide != 0) >= q) hi = mid;
    else lo = mid + 1;
  }
  start[q] = (uint32_t)lo;
}

constexpr int SEL_SHORT = 16;   // lists up to here: one 16-lane group per query (every query is visited)
constexpr int SEL_LONG = 64;    // lists up to here: one wave per query; beyond: the histogram kernel
constexpr int SEL_MAXK = 256;   // largest K of the select form (the sort form has no limit)
constexpr int SEL_LIST_GRID = 1024;
constexpr int64_t SEL_FORK_NQ = 1 << 22;   // from here on the medium and long lists run beside the short ones (qrlsh_topk_select_fill)

// list lengths -> output counts (min(K, length)); queries whose list does not fit a 16-lane group are put on
// the medium (17 .. 64) or the long list.  A workgroup classifies LEN_QPB consecutive queries, collects its two
// lists in LDS and reserves their room with ONE global atomic each: a popular counter word takes ~90 atomics per
// microsecond, and at 10 M queries nearly every wave holds a medium query.
constexpr int LEN_QPB = 4096;
__global__ __launch_bounds__(256) void topk_len_kernel(const uint32_t *__restrict__ fstart,
                                                       const uint32_t *__restrict__ rstart, int64_t nq, int K,
                                                       uint64_t *__restrict__ cnt, uint32_t *__restrict__ medlist,
                                                       uint32_t *__restrict__ longlist,
                                                       unsigned long long *__restrict__ nlists,
                                                       uint64_t *__restrict__ wgsum) {
  __shared__ uint32_t smed[LEN_QPB], slng[LEN_QPB], sval[LEN_QPB + LEN_QPB / 16];   // (sval: padded, see lpad)
  __shared__ uint64_t sscan[4];
  __shared__ uint32_t nmed, nlng;
  __shared__ unsigned long long bmed, blng;
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  auto lpad = [](int i) { return i + (i >> 4); };   // a word of padding per 16: a thread's 16 consecutive counts meet no bank twice
  if (threadIdx.x == 0) {
    nmed = 0;
    nlng = 0;
  }
  __syncthreads();
  const int64_t q0 = (int64_t)blockIdx.x * LEN_QPB;
#pragma unroll 4
  for (int it = 0; it < LEN_QPB / 256; ++it) {
    const int64_t q = q0 + it * 256 + threadIdx.x;
    uint64_t c = 0;
    if (q < nq) c = (uint64_t)(fstart[q + 1] - fstart[q]) + (rstart[q + 1] - rstart[q]);
    sval[lpad(it * 256 + threadIdx.x)] = (uint32_t)(c > (uint64_t)K ? (uint64_t)K : c);  // (0 past the end)
    const bool med = c > (uint64_t)SEL_SHORT && c <= (uint64_t)SEL_LONG, lng = c > (uint64_t)SEL_LONG;
    const uint64_t mm = __ballot(med), ml = __ballot(lng);
    uint32_t pm = 0, pl = 0;
    if (lane == 0) {
      if (mm) pm = atomicAdd(&nmed, (uint32_t)__popcll(mm));
      if (ml) pl = atomicAdd(&nlng, (uint32_t)__popcll(ml));
    }
    pm = __shfl(pm, 0, WAVE);
    pl = __shfl(pl, 0, WAVE);
    if (med) smed[pm + (uint32_t)__popcll(mm & lt_mask)] = (uint32_t)q;
    if (lng) slng[pl + (uint32_t)__popcll(ml & lt_mask)] = (uint32_t)q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bmed = nmed ? __hip_atomic_fetch_add(&nlists[0], (unsigned long long)nmed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    blng = nlng ? __hip_atomic_fetch_add(&nlists[1], (unsigned long long)nlng, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < nmed; k += 256) medlist[bmed + k] = smed[k];
  for (uint32_t k = threadIdx.x; k < nlng; k += 256) longlist[blng + k] = slng[k];
  // the workgroup's own exclusive scan of its counts (16 consecutive per thread; at most 4096 * 256: 32 bits hold
  // it), and its total next to them: topk_off_add_kernel adds the scanned totals, so the 10 M-entry array is
  // written once and rewritten once instead of written, scanned in chunks and rewritten
  constexpr int PER = LEN_QPB / 256;
  uint32_t v[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    v[k] = sval[lpad(threadIdx.x * PER + k)];
    sum += v[k];
  }
  uint64_t total;
  uint32_t run = (uint32_t)block_excl_scan_u64_256((uint64_t)sum, sscan, &total);   // (its barriers end the reads)
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    sval[lpad(threadIdx.x * PER + k)] = run;
    run += v[k];
  }
  __syncthreads();
  // cnt[nq], one word past the end: its count is 0, so the total ends up there
  for (int k = threadIdx.x; k < LEN_QPB; k += 256)
    if (q0 + k <= nq) cnt[q0 + k] = sval[lpad(k)];
  if (threadIdx.x == 0) wgsum[blockIdx.x] = total;
}

// off[q] += the scanned total of the workgroups in front of q's (wgsum after its exclusive scan)
__global__ __launch_bounds__(256) void topk_off_add_kernel(uint64_t *__restrict__ off, int64_t m,
                                                           const uint64_t *__restrict__ wgsum) {
  const uint64_t add = wgsum[blockIdx.x];
  const int64_t q0 = (int64_t)blockIdx.x * LEN_QPB;
  if (add == 0) return;   // (uniform)
#pragma unroll 4
  for (int k = threadIdx.x; k < LEN_QPB; k += 256)
    if (q0 + k < m) off[q0 + k] += add;
}

// Element x of a query's list of `len` entries: x < nr -> reverse run, else forward run.  sel_load fetches it and
// sel_key turns what was fetched into the key (inv << 32 | dst); x >= len -> ~0, the key of an absent element (never
// smaller than a real one; its inv is no value).
// One pair of 4-byte loads, without a branch, serves either run: (lo, hi) = the two halves of the reverse word, or
// (the low half of the pair word = dst, milli); an absent element reads the first reverse word (n > 0).  A caller
// that takes several keys (the queries of a 16-lane group, the register batch of a long list) calls sel_load for all
// of them and only then sel_key: all their loads are in flight at once, two registers per key.  Written as one
// function, `if (x < nr) return ...; return ...;`, the compiler waited for each key inside its branch: the keys of
// one thread came one memory round trip after the other.
struct SelRaw {
  uint32_t lo, hi, wd;
};
template <bool WIDE>
__device__ static inline SelRaw sel_load(uint32_t x, uint32_t len, uint32_t rs, uint32_t nr, uint32_t fs,
                                         const uint64_t *__restrict__ pairs, const int32_t *__restrict__ milli,
                                         const uint64_t *__restrict__ rev, const uint32_t *__restrict__ rdst) {
  const bool inr = x < nr, inf = !inr && x < len;
  const uint64_t r = inr ? (uint64_t)(rs + x) : 0ull, y = (uint64_t)(fs + (x - nr));
  const uint32_t *blo = inf ? reinterpret_cast<const uint32_t *>(pairs) : reinterpret_cast<const uint32_t *>(rev);
  const uint32_t *bhi = inf ? reinterpret_cast<const uint32_t *>(milli) : reinterpret_cast<const uint32_t *>(rev);
  SelRaw v;
  v.lo = blo[inf ? 2 * y : 2 * r];
  v.hi = bhi[inf ? y : 2 * r + 1];
  v.wd = WIDE ? rdst[r] : 0u;
  return v;
}
template <bool WIDE>
__device__ static inline uint64_t sel_key(SelRaw v, uint32_t x, uint32_t len, uint32_t nr, int id_bits, uint64_t idm) {
  const uint64_t w = (uint64_t)v.hi << 32 | v.lo;
  const uint64_t kr = WIDE ? (w & 0x7FFull) << 32 | v.wd : ((w >> id_bits) & 0x7FFull) << 32 | (w & idm);
  const uint64_t kf = (uint64_t)(uint32_t)(1000 - (int32_t)v.hi) << 32 | v.lo;
  return x < nr ? kr : x < len ? kf : ~0ull;
}

// 64-bit value of the lane S positions further round this lane's 16-lane row (DPP row_ror)
template <int S> __device__ static inline uint64_t row_ror64(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x120 + S, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x120 + S, 0xF, 0xF, false);
  return (uint64_t)(uint32_t)hi << 32 | (uint32_t)lo;
}
template <int S> __device__ static inline uint32_t row_rank(uint64_t mine) {
  uint32_t r = row_ror64<S>(mine) < mine;
  if constexpr (S > 1) r += row_rank<S - 1>(mine);
  return r;
}

// Lists of up to 16 neighbours (almost every query): one 16-lane group per query, lane l holds element l, and a
// lane's rank is the number of smaller keys met while the row rotates past it (15 DPP steps, no memory traffic).
// Absent elements carry the key ~0: never smaller than a real one.
constexpr int SEL_QPG = 4;  // queries per 16-lane group: their loads are issued together (latency-bound otherwise)
template <bool WIDE>
__global__ __launch_bounds__(256) void topk_select_short_kernel(const uint64_t *__restrict__ pairs,
                                                                const int32_t *__restrict__ milli,
                                                                const uint64_t *__restrict__ rev,
                                                                const uint32_t *__restrict__ rdst,
                                                                const uint32_t *__restrict__ fstart,
                                                                const uint32_t *__restrict__ rstart,
                                                                const uint64_t *__restrict__ off, int64_t nq, int K,
                                                                int id_bits, int32_t *__restrict__ src_out,
                                                                int32_t *__restrict__ dst_out,
                                                                int32_t *__restrict__ milli_out) {
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) >> 4;
  const uint32_t l = threadIdx.x & 15;
  const uint64_t idm = id_bits >= 32 ? 0xFFFFFFFFull : (1ull << id_bits) - 1ull;
  // query c of this group: group + c * ngroups (consecutive groups -> consecutive queries: the start arrays are read in runs)
  // Both load levels without a branch between the queries: a query past the end reads the last query's entries
  // (and gets length 0), so the 5 * SEL_QPG loads of the first level and then the keys of the second are each
  // issued together.  With `if (q < nq) { loads }` per query the compiler waited inside every branch.
  uint32_t fs[SEL_QPG], fe[SEL_QPG], rs[SEL_QPG], re[SEL_QPG], nr[SEL_QPG], len[SEL_QPG];
  uint64_t o0[SEL_QPG], mine[SEL_QPG];
  SelRaw raw[SEL_QPG];
#pragma unroll
  for (int c = 0; c < SEL_QPG; ++c) {
    const int64_t q = group + (int64_t)c * ngroups, qc = q < nq ? q : nq - 1;
    fs[c] = fstart[qc];
    fe[c] = fstart[qc + 1];
    rs[c] = rstart[qc];
    re[c] = rstart[qc + 1];
    o0[c] = off[qc];
  }
#pragma unroll
  for (int c = 0; c < SEL_QPG; ++c) {
    nr[c] = re[c] - rs[c];
    len[c] = (fe[c] - fs[c]) + nr[c];
    // (past the end, or another kernel's query)
    if (group + (int64_t)c * ngroups >= nq || len[c] > (uint32_t)SEL_SHORT) len[c] = 0;
  }
#pragma unroll
  for (int c = 0; c < SEL_QPG; ++c)
    raw[c] = sel_load<WIDE>(l, len[c], rs[c], nr[c], fs[c], pairs, milli, rev, rdst);
#pragma unroll
  for (int c = 0; c < SEL_QPG; ++c) mine[c] = sel_key<WIDE>(raw[c], l, len[c], nr[c], id_bits, idm);
#pragma unroll
  for (int c = 0; c < SEL_QPG; ++c) {
    const uint32_t rank = row_rank<15>(mine[c]);  // executed by every lane (all lanes of the wave are active here)
    if (l < len[c] && rank < (uint32_t)K) {
      const uint64_t o = o0[c] + rank;
      src_out[o] = (int32_t)(group + (int64_t)c * ngroups);
      dst_out[o] = (int32_t)(uint32_t)mine[c];
      milli_out[o] = 1000 - (int32_t)(uint32_t)(mine[c] >> 32);
    }
  }
}

// Lists of 17 .. 64 neighbours: one wave per query, from a fixed grid that walks the medium list.
template <bool WIDE>
__global__ __launch_bounds__(256) void topk_select_medium_kernel(const uint64_t *__restrict__ pairs,
                                                                 const int32_t *__restrict__ milli,
                                                                 const uint64_t *__restrict__ rev,
                                                                 const uint32_t *__restrict__ rdst,
                                                                 const uint32_t *__restrict__ fstart,
                                                                 const uint32_t *__restrict__ rstart,
                                                                 const uint64_t *__restrict__ off,
                                                                 const uint32_t *__restrict__ medlist,
                                                                 const unsigned long long *__restrict__ nlists, int K,
                                                                 int id_bits, int32_t *__restrict__ src_out,
                                                                 int32_t *__restrict__ dst_out,
                                                                 int32_t *__restrict__ milli_out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const uint64_t idm = id_bits >= 32 ? 0xFFFFFFFFull : (1ull << id_bits) - 1ull;
  const unsigned long long nm = nlists[0], nwaves = (unsigned long long)gridDim.x * (blockDim.x / WAVE);
  for (unsigned long long e = (unsigned long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6); e < nm;
       e += nwaves) {
    const uint32_t q = medlist[e];
    const uint32_t fs = fstart[q], nf = fstart[q + 1] - fs, rs = rstart[q], nr = rstart[q + 1] - rs;
    const uint32_t len = nf + nr;  // 17 .. 64
    const uint64_t mine = sel_key<WIDE>(sel_load<WIDE>(lane, len, rs, nr, fs, pairs, milli, rev, rdst), lane, len, nr, id_bits, idm);
    uint32_t rank = 0;
#pragma unroll 9
    for (int s = 1; s < WAVE; ++s) {  // every other lane's key once (absent elements: ~0, never smaller)
      const int from = (lane + s) & (WAVE - 1);
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)mine, from, WAVE), hi = (uint32_t)__shfl((int)(uint32_t)(mine >> 32), from, WAVE);
      rank += ((uint64_t)hi << 32 | lo) < mine;
    }
    if ((uint32_t)lane < len && rank < (uint32_t)K) {
      const uint64_t o = off[q] + rank;
      src_out[o] = (int32_t)q;
      dst_out[o] = (int32_t)(uint32_t)mine;
      milli_out[o] = 1000 - (int32_t)(uint32_t)(mine >> 32);
    }
  }
}

// Popular queries (lists beyond SEL_LONG): one wave per query, O(list length).  A histogram of the 2001
// possible values (inv = 1000 - milli) locates the value v* at which the K-th neighbour sits; the neighbours
// with inv < v* are all kept, and of those with inv == v* the first K - (number below) in list order -- the
// list order (reverse run, then forward run) IS ascending neighbour id, the tie-break.  The <= K survivors then
// rank themselves among each other.
// The wave holds a register batch of SEL_LK keys per lane (element base + k * 64 + lane in kk[k]): all SEL_LK loads
// of a batch are issued before the first histogram add, and a list of up to SEL_BATCH entries is read from memory
// ONCE -- the sweep in list order and the by_id rounds then read the registers.  A longer list is worked in
// batches of SEL_BATCH in every sweep (re-read, SEL_LK loads in flight).  One load per lane in flight and an LDS
// atomic behind each made every sweep a chain of len / 64 memory round trips.
constexpr int SEL_LK = 16;
constexpr int SEL_BATCH = WAVE * SEL_LK;
template <bool WIDE>
__global__ __launch_bounds__(256, 4) void topk_select_long_kernel(const uint64_t *__restrict__ pairs,
                                                               const int32_t *__restrict__ milli,
                                                               const uint64_t *__restrict__ rev,
                                                               const uint32_t *__restrict__ rdst,
                                                               const uint32_t *__restrict__ fstart,
                                                               const uint32_t *__restrict__ rstart,
                                                               const uint64_t *__restrict__ off,
                                                               const uint32_t *__restrict__ longlist,
                                                               const unsigned long long *__restrict__ nlists, int K,
                                                               int id_bits, int32_t *__restrict__ src_out,
                                                               int32_t *__restrict__ dst_out,
                                                               int32_t *__restrict__ milli_out, int by_id) {
  constexpr int NV = 2048;  // inv in [0, 2000]
  constexpr int OWN = NV / WAVE;  // lane l owns values [32 l, 32 l + 32)
  __shared__ __align__(16) uint32_t hist_all[4][NV];
  __shared__ uint64_t keep_all[4][SEL_MAXK];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  uint32_t *hist = hist_all[wv];
  uint64_t *keep = keep_all[wv];
  const uint64_t idm = id_bits >= 32 ? 0xFFFFFFFFull : (1ull << id_bits) - 1ull;
  const unsigned long long nl = nlists[1];
  const unsigned long long nwaves = (unsigned long long)gridDim.x * 4;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  // the wave's histogram to zero (16-byte stores), and the sum of a lane's OWN words: lane l starts at its word
  // l mod 32 and goes round, so the lanes of a 32-lane half read 32 different banks (straight, hist[32 l + v], they all
  // read the same one)
  auto hist_zero = [&]() {
    uint4 *h4 = reinterpret_cast<uint4 *>(hist);
    for (int v = lane; v < NV / 4; v += WAVE) h4[v] = make_uint4(0u, 0u, 0u, 0u);
  };
  auto own_sum = [&]() {
    uint32_t s = 0;
#pragma unroll 8
    for (int v = 0; v < OWN; ++v) s += hist[lane * OWN + ((v + lane) & (OWN - 1))];
    return s;
  };
  for (unsigned long long e = (unsigned long long)blockIdx.x * 4 + wv; e < nl; e += nwaves) {
    const uint32_t q = longlist[e];
    const uint32_t fs = fstart[q], nf = fstart[q + 1] - fs, rs = rstart[q], nr = rstart[q + 1] - rs;
    const uint32_t len = nf + nr;
    const uint64_t o0 = off[q];
    const bool fits = len <= (uint32_t)SEL_BATCH;  // (uniform) the registers hold the whole list after the first sweep
    uint64_t kk[SEL_LK];
    auto load = [&](uint32_t base) {
      SelRaw raw[SEL_LK];
#pragma unroll
      for (int k = 0; k < SEL_LK; ++k)
        raw[k] = sel_load<WIDE>(base + (uint32_t)(k * WAVE + lane), len, rs, nr, fs, pairs, milli, rev, rdst);
#pragma unroll
      for (int k = 0; k < SEL_LK; ++k)
        kk[k] = sel_key<WIDE>(raw[k], base + (uint32_t)(k * WAVE + lane), len, nr, id_bits, idm);
    };
    // (the sweeps leave a batch at the first row past the list's end: most lists are far shorter than a batch)
    hist_zero();
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < len; base += SEL_BATCH) {
      load(base);
#pragma unroll
      for (int k = 0; k < SEL_LK; ++k) {
        if (base + (uint32_t)(k * WAVE) >= len) break;
        const uint32_t inv = (uint32_t)(kk[k] >> 32);
        if (inv < (uint32_t)NV) atomicAdd(&hist[inv], 1u);   // (absent elements: inv = ~0)
      }
    }
    __builtin_amdgcn_wave_barrier();
    // v* = smallest v with count(inv <= v) >= K; below = count(inv < v*)
    const uint32_t mysum = own_sum();
    const uint32_t inc = wave_incl_scan(mysum);
    const uint64_t reach = __ballot(inc >= (uint32_t)K);  // len > SEL_LONG >= ... may still be < K: then keep all
    uint32_t vstar = NV, below = 0;
    if (reach) {
      const int owner = __ffsll((long long)reach) - 1;
      uint32_t run = __shfl(inc - mysum, owner, WAVE);   // count below the owner's first value
      uint32_t vs = NV, bl = 0;
      if (lane == owner) {
        for (int v = 0; v < OWN; ++v) {
          const uint32_t h = hist[lane * OWN + v];
          if (run + h >= (uint32_t)K) {
            vs = lane * OWN + v;
            bl = run;
            break;
          }
          run += h;
        }
      }
      vstar = __shfl(vs, owner, WAVE);
      below = __shfl(bl, owner, WAVE);
    }
    const uint32_t want_eq = reach ? (uint32_t)K - below : 0u;  // ties at v* kept, in list order
    // List order IS ascending neighbour id when the list is the query's two runs (smaller ids in the reverse run,
    // larger ones in the forward run, each ascending).  A list made of reverse words alone (by_id: edges that
    // arrived from several scoring ranks) has no such order: the ties to keep are then the want_eq SMALLEST ids
    // among the elements at v* -- found by a radix select on the id, 11 bits per round (ids are distinct in a list).
    uint32_t id_cut = 0xFFFFFFFFu;  // ties with id <= id_cut are kept
    if (by_id && reach && hist[vstar] > want_eq) {  // uniform
      uint32_t prefix = 0, need = want_eq;          // ids whose top bits equal `prefix` are still undecided
      for (int shift = 22; shift >= 0; shift -= 11) {
        __builtin_amdgcn_wave_barrier();
        hist_zero();
        __builtin_amdgcn_wave_barrier();
        for (uint32_t base = 0; base < len; base += SEL_BATCH) {
          if (!fits) load(base);
#pragma unroll
          for (int k = 0; k < SEL_LK; ++k) {
            if (base + (uint32_t)(k * WAVE) >= len) break;
            const uint32_t idv = (uint32_t)kk[k];
            if ((uint32_t)(kk[k] >> 32) == vstar && (shift == 22 || (idv >> (shift + 11)) == prefix))
              atomicAdd(&hist[(idv >> shift) & (NV - 1)], 1u);
          }
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t ms = own_sum();
        const uint32_t ic = wave_incl_scan(ms);
        const int owner = __ffsll((long long)__ballot(ic >= need)) - 1;  // (need <= the number of undecided ids)
        uint32_t run = __shfl(ic - ms, owner, WAVE), dg = 0, bl = 0;
        if (lane == owner) {
          for (int v = 0; v < OWN; ++v) {
            const uint32_t h = hist[lane * OWN + v];
            if (run + h >= need) {
              dg = lane * OWN + v;
              bl = run;
              break;
            }
            run += h;
          }
        }
        dg = __shfl(dg, owner, WAVE);
        bl = __shfl(bl, owner, WAVE);
        prefix = shift == 22 ? dg : (prefix << 11 | dg);
        need -= bl;                                  // ids below this digit are all kept
      }
      id_cut = prefix;                               // the need-th smallest undecided id itself (need == 1 by now)
    }
    // second sweep, in list order (k ascending, then lane, inside a batch): collect the survivors
    const uint32_t want = len < (uint32_t)K ? len : (uint32_t)K;
    uint32_t nkeep = 0, neq = 0;
    for (uint32_t base = 0; base < len && nkeep < want; base += SEL_BATCH) {   // (all `want` found: none follows)
      if (!fits) load(base);
#pragma unroll
      for (int k = 0; k < SEL_LK; ++k) {
        if (base + (uint32_t)(k * WAVE) >= len) break;
        const uint64_t key = kk[k];
        const uint32_t inv = (uint32_t)(key >> 32);
        const bool lt = inv < vstar;      // (absent elements: inv = ~0, neither below nor at v* <= NV)
        const bool eq = inv == vstar;
        const uint64_t meq = __ballot(eq);
        const bool take_eq = eq && (id_cut != 0xFFFFFFFFu ? (uint32_t)key <= id_cut
                                                          : neq + (uint32_t)__popcll(meq & lt_mask) < want_eq);
        const uint64_t mk = __ballot(lt || take_eq);
        if (lt || take_eq) keep[nkeep + (uint32_t)__popcll(mk & lt_mask)] = key;
        nkeep += (uint32_t)__popcll(mk);
        neq += (uint32_t)__popcll(meq);
      }
    }
    __builtin_amdgcn_wave_barrier();
    // nkeep == min(K, len); rank the survivors among themselves
    for (uint32_t a = lane; a < nkeep; a += WAVE) {
      const uint64_t k = keep[a];
      uint32_t r = 0;
      for (uint32_t c = 0; c < nkeep; ++c) r += keep[c] < k;
      src_out[o0 + r] = (int32_t)q;
      dst_out[o0 + r] = (int32_t)(uint32_t)k;
      milli_out[o0 + r] = 1000 - (int32_t)(uint32_t)(k >> 32);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// workspace: fstart u32[nq + 1] | rstart u32[nq + 1] | medlist u32[nq] | longlist u32[nq] | off u64[nq + 2] |
//            list lengths u64[2] | totals of topk_len_kernel's workgroups
struct SelWs {
  uint32_t *fstart, *rstart, *medlist, *longlist;
  uint64_t *off, *nlong, *sums;
};
static SelWs sel_layout(QrCarve &c, int64_t nq) {
  SelWs w;
  const size_t row = qr_al16((size_t)(nq + 1) * 4) / 4;   // words of one array, rounded
  w.fstart = c.take<uint32_t>(2 * row);                   // fstart | rstart: one memset covers both
  w.rstart = qr_within(w.fstart, row);
  w.medlist = c.take<uint32_t>(row);
  w.longlist = c.take<uint32_t>(row);
  w.off = c.take<uint64_t>((size_t)(nq + 2), 8);
  w.nlong = c.take<uint64_t>(2);
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(nq + 1, LEN_QPB) + 2), 8);   // (one per workgroup of topk_len_kernel)
  return w;
}
static SelWs sel_layout(const void *workspace, int64_t nq) {
  QrCarve c(workspace);
  return sel_layout(c, nq);
}

QRLSH_EXPORT size_t qrlsh_topk_select_workspace_bytes(int64_t nq) {
  if (nq <= 0) return 64;
  return QR_LAYOUT_BYTES(sel_layout, nq);
}

QRLSH_EXPORT int qrlsh_topk_select_count(const uint64_t *pairs, int64_t n, const uint64_t *rev_sorted,
                                         const uint32_t *rev_dst, int64_t nq, int32_t K, int32_t id_bits, void *workspace,
                                         size_t workspace_bytes, uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && nq > 0 && nq <= (1ll << 32) && K > 0 && K <= SEL_MAXK && id_bits >= 1 &&
                   id_bits <= 32,
               "qrlsh_topk_select_count: bad arguments (n=%lld nq=%lld K=%d (<= %d) id_bits=%d)", (long long)n,
               (long long)nq, K, SEL_MAXK, id_bits);
  // packed reverse words: src << (id_bits + 11) | inv << id_bits | neighbour must fit 64 bits
  QR_CHECK_ARG(rev_dst || id_bits <= 26 || (!pairs && ((uint64_t)(nq - 1) >> (53 - id_bits)) == 0),
               "qrlsh_topk_select_count: packed reverse words need id_bits <= 26 (or, without a forward list, src < 2^(53 - id_bits))");
  // pairs == NULL: the lists are made of the n reverse words alone (the sharded driver: every directed edge a rank
  // receives is such a word, src = its own query)
  QR_CHECK_ARG(total_out && workspace && (n == 0 || rev_sorted), "qrlsh_topk_select_count: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_topk_select_count", workspace, workspace_bytes, qrlsh_topk_select_workspace_bytes(nq));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SelWs w = sel_layout(workspace, nq);
  QR_MEMSET("qrlsh_topk_select_count", w.nlong, 0, 2 * sizeof(uint64_t), st);
  const dim3 blk(256);
  // both start arrays (contiguous in the workspace) to "unset", boundaries, then the long stretches
  QR_MEMSET("qrlsh_topk_select_count", w.fstart, 0xFF, (size_t)((char *)w.medlist - (char *)w.fstart), st);
  const int lists = pairs ? 2 : 1, y0 = pairs ? 0 : 1;
  if (!pairs) QR_MEMSET("qrlsh_topk_select_count", w.fstart, 0, (size_t)((char *)w.rstart - (char *)w.fstart), st);   // every forward run is empty
  QR_LAUNCH("topk_bounds", edge_bounds_kernel, dim3((unsigned)ceil_div64(n + 1, 256 * EB_RUN), lists), blk, 0, st, pairs,
            rev_sorted, n, nq, id_bits, rev_dst ? 1 : 0, w.fstart, w.rstart, y0);
  QR_LAUNCH("topk_bounds", edge_bounds_fix_kernel, dim3((unsigned)ceil_div64(nq + 1, 256), lists), blk, 0, st, pairs,
            rev_sorted, n, nq, id_bits, rev_dst ? 1 : 0, w.fstart, w.rstart, y0);
  QR_LAUNCH("topk_len", topk_len_kernel, dim3((unsigned)ceil_div64(nq + 1, LEN_QPB)), blk, 0, st, (const uint32_t *)w.fstart,
            (const uint32_t *)w.rstart, nq, K, w.off, w.medlist, w.longlist,
            reinterpret_cast<unsigned long long *>(w.nlong), w.sums);
  // offsets: the workgroups left their own exclusive scans in w.off and their totals in w.sums -- the small scan of
  // the totals (2 442 words at 10 M queries; one workgroup) and one add pass.  The fix kernel stays a pass of its
  // own: its binary searches must all be over before any length is taken.
  const int64_t nwg = ceil_div64(nq + 1, LEN_QPB);
  QR_LAUNCH("scan_blocks", scan_u64_kernel, dim3(1), dim3(1024), 0, st, w.sums, nwg, total_out);
  QR_LAUNCH("scan_blocks", topk_off_add_kernel, dim3((unsigned)nwg), blk, 0, st, w.off, nq + 1, (const uint64_t *)w.sums);
  QR_LAUNCH_CHECK("qrlsh_topk_select_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_topk_select_fill(const uint64_t *pairs, const int32_t *milli, int64_t n,
                                        const uint64_t *rev_sorted, const uint32_t *rev_dst, int64_t nq, int32_t K,
                                        int32_t id_bits, const void *workspace, int32_t *src_out, int32_t *dst_out,
                                        int32_t *milli_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && nq > 0 && K > 0 && K <= SEL_MAXK && id_bits >= 1 && id_bits <= 32,
               "qrlsh_topk_select_fill: bad arguments");
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG((pairs == nullptr) == (milli == nullptr) && rev_sorted && workspace && src_out && dst_out && milli_out,
               "qrlsh_topk_select_fill: null pointer (pairs and milli: both or neither)");
  const SelWs w = sel_layout(workspace, nq);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t *fsp = w.fstart, *rsp = w.rstart;
  const uint64_t *offp = w.off;
  const unsigned long long *nl = reinterpret_cast<const unsigned long long *>(w.nlong);
  // Every query belongs to exactly one of the three kernels and they write disjoint output rows: the two small
  // fixed grids of the medium and long lists run on the auxiliary stream (api.hip: qr_aux_fork; none with the
  // profiler on or overlap off -- then all three follow each other on `st`) beside the short kernel, which visits
  // every query.  Below SEL_FORK_NQ queries they stay on `st` too: the two cross-stream waits of a fork and join cost
  // about 0.03 ms, what the overlap gains at 3 M queries (0.1 ms of the 0.95 at 10 M; at 1 M the step was 0.027 ms
  // slower with the fork than without).
  auto launch = [&](auto wide) -> int {   // (packed or wide reverse words: the kernels' two forms)
    constexpr bool W = decltype(wide)::value;
    hipStream_t aux = nq >= SEL_FORK_NQ ? qr_aux_fork(st) : nullptr;
    hipStream_t sl = aux ? aux : st;
    QR_LAUNCH("topk_select_long", topk_select_long_kernel<W>, dim3(SEL_LIST_GRID), dim3(256), 0, sl, pairs, milli,
              rev_sorted, rev_dst, fsp, rsp, offp, (const uint32_t *)w.longlist, nl, K, id_bits, src_out, dst_out, milli_out,
              pairs ? 0 : 1);
    QR_LAUNCH("topk_select_medium", topk_select_medium_kernel<W>, dim3(SEL_LIST_GRID), dim3(256), 0, sl, pairs, milli,
              rev_sorted, rev_dst, fsp, rsp, offp, (const uint32_t *)w.medlist, nl, K, id_bits, src_out, dst_out, milli_out);
    QR_LAUNCH("topk_select", topk_select_short_kernel<W>, dim3((unsigned)ceil_div64(nq, 16 * SEL_QPG)), dim3(256), 0, st,
              pairs, milli, rev_sorted, rev_dst, fsp, rsp, offp, nq, K, id_bits, src_out, dst_out, milli_out);
    if (aux && qr_aux_join(st) != QRLSH_OK) return QRLSH_EHIP;
    return QRLSH_OK;
  };
  if ((rev_dst ? launch(std::true_type{}) : launch(std::false_type{})) != QRLSH_OK) return QRLSH_EHIP;
  QR_LAUNCH_CHECK("qrlsh_topk_select_fill");
  return QRLSH_OK;
}
