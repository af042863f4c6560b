// fidelity.hip -- how many of a query's true nearest neighbours its served list holds (qrlsh_edge_overlaps,
// qrlsh_list_fidelity; the contract is in include/qrlsh.h).  "True" = Jaccard over the CSR answer sets, the quantity
// MinHash estimates.  Integer arithmetic only: J_a > J_b is inter_a * union_b > inter_b * union_a in int64.
//
//   edge_overlaps     one group of FD_W lanes per edge: the lanes walk the shorter set (coalesced), each binary-searches
//                     the longer one, the group adds up.  FD_W = 16: the walked set is the SHORTER of two whose mean is
//                     about 20 rows, so one trip serves most edges and a wave holds four of them; longer sets loop.
//   fidelity_entries  the same intersection for the stored entries of the chosen queries -> inter / union [m][64]
//   fidelity_sweep    workgroup (group of G requests, slice of the ids j): the G answer sets as ONE interleaved bitmap in
//                     LDS -- row r owns G adjacent bits, bit g = "request g holds r" -- so a row id of the slice costs one
//                     LDS read for all G requests; beside it the G x 64 stored (inter, union) and their better / equal
//                     counters.  A group of FD_W lanes per j reads its rows once, ORs the masks, and only for the
//                     requests whose bit came up (inter > 0) counts the intersection and makes the <= 64 comparisons.
//                     The counters go out with integer atomics: exact in any launch order, for every slice count.
//   fidelity_finish   one wave per request: equal's share that the sweep cannot see (J = 0 ties, the entry's own target),
//                     words 0 - 7 and the totals.
#include "fidelitywalk.h"   // the group rule, the bitmap, the walk, fd_request, fd_slices: shared with exactlists.hip

namespace {

constexpr int FD_THREADS = 256;
constexpr int FD_EDGES = FD_THREADS / FD_W;      // edges per workgroup
// FD_FIXED_WORDS per request: its query id, entries listed, |A|, positives
// FD_REQ_WORDS per request: inter, union, better, equal of its entries

// |A(s) intersect A(d)|, s and d inside [0, nq): the group's FD_W lanes (sub = the lane's place in it) walk the shorter
// set, each binary-searches the longer; every lane of the group returns the sum
__device__ static inline int32_t fd_overlap(const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t s,
                                            int64_t d, int sub) {
  int64_t alo = off[s], ahi = off[s + 1], blo = off[d], bhi = off[d + 1];
  if (ahi - alo > bhi - blo) {
    int64_t t = alo; alo = blo; blo = t;
    t = ahi; ahi = bhi; bhi = t;
  }
  int32_t cnt = 0;
  for (int64_t p = alo + sub; p < ahi; p += FD_W) {
    const int32_t r = rows[p];
    int64_t lo = blo, hi = bhi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (rows[mid] < r) lo = mid + 1;
      else hi = mid;
    }
    if (lo < bhi && rows[lo] == r) ++cnt;
  }
#pragma unroll
  for (int dl = FD_W / 2; dl; dl >>= 1) cnt += __shfl_xor(cnt, dl, FD_W);
  return cnt;
}

__global__ __launch_bounds__(FD_THREADS) void edge_overlaps_kernel(const int64_t *__restrict__ off,
                                                                   const int32_t *__restrict__ rows, int64_t nq,
                                                                   const int32_t *__restrict__ src,
                                                                   const int32_t *__restrict__ dst, int64_t n,
                                                                   int32_t *__restrict__ inter_out,
                                                                   uint32_t *__restrict__ flags) {
  const int sub = threadIdx.x & (FD_W - 1);
  const int64_t e = (int64_t)blockIdx.x * FD_EDGES + threadIdx.x / FD_W;
  if (e >= n) return;
  const int64_t s = src[e], d = dst[e];
  int32_t cnt = 0;
  if (s < 0 || s >= nq || d < 0 || d >= nq) {
    if (sub == 0) atomicOr(flags, 1u);
  } else {
    cnt = fd_overlap(off, rows, s, d, sub);
  }
  if (sub == 0) inter_out[e] = cnt;
}

// one group per (request, entry slot): inter / union of the first min(len, K) stored entries, 0 in the other slots
__global__ __launch_bounds__(FD_THREADS) void fidelity_entries_kernel(
    const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t nq, const int64_t *__restrict__ q_off,
    const int32_t *__restrict__ q_idx, const int32_t *__restrict__ queries, int64_t m, int K,
    int32_t *__restrict__ inter_out, int32_t *__restrict__ union_out, uint32_t *__restrict__ flags) {
  const int sub = threadIdx.x & (FD_W - 1);
  const int64_t slot = (int64_t)blockIdx.x * FD_EDGES + threadIdx.x / FD_W;
  const int64_t x = slot / FD_MAXK;
  const int e = (int)(slot % FD_MAXK);
  if (x >= m) return;
  int64_t len;
  uint32_t bad;
  const int64_t s = fd_request(queries, x, nq, q_off, len, bad);
  int32_t in = 0, un = 0;
  if (s >= 0 && e < (len < K ? len : K)) {
    const int64_t d = q_idx[q_off[s] + e];
    if (d < 0 || d >= nq) {
      bad |= 2u;
    } else {
      in = fd_overlap(off, rows, s, d, sub);
      un = (int32_t)((off[s + 1] - off[s]) + (off[d + 1] - off[d]) - in);
    }
  }
  if (sub == 0) {
    if (bad) atomicOr(flags, bad);
    inter_out[slot] = in;
    union_out[slot] = un;
  }
}

__global__ __launch_bounds__(FD_SWEEP_THREADS) void fidelity_sweep_kernel(
    const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t nq, int64_t D,
    const int64_t *__restrict__ q_off, const int32_t *__restrict__ queries, int64_t m, int K, int G, int64_t per,
    const int32_t *__restrict__ inter_in, const int32_t *__restrict__ union_in, int32_t *__restrict__ better_out,
    int32_t *__restrict__ equal_out, int64_t *__restrict__ words_out, uint32_t *__restrict__ flags) {
  __shared__ uint32_t lds[FD_LDS_WORDS];
  int32_t *const sid = reinterpret_cast<int32_t *>(lds);   // [FD_MAXG] the chosen query, -1 = not served
  uint32_t *const listed = lds + FD_MAXG;                  // [FD_MAXG]
  uint32_t *const size_a = lds + 2 * FD_MAXG;              // [FD_MAXG]
  uint32_t *const positives = lds + 3 * FD_MAXG;           // [FD_MAXG]
  uint32_t *const ent = lds + FD_FIXED_WORDS;              // [G][inter, union, better, equal][FD_MAXK]
  uint32_t *const bits = ent + G * FD_REQ_WORDS;           // ceil(D G / 32) words
  const int tid = threadIdx.x;
  const int64_t x0 = (int64_t)blockIdx.x * G;
  const int ng = (int)(m - x0 < G ? m - x0 : G);
  const int64_t j0 = (int64_t)blockIdx.y * per, j1 = j0 + per < nq ? j0 + per : nq;
  if (j0 >= j1) return;   // uniform
  const int bitw = (int)((D * G + 31) / 32);
  for (int i = tid; i < bitw; i += FD_SWEEP_THREADS) bits[i] = 0;
  if (tid < FD_MAXG) {
    int64_t s = -1, len = 0;
    uint32_t bad;
    if (tid < ng) s = fd_request(queries, x0 + tid, nq, q_off, len, bad);   // the entries kernel has raised the flags
    sid[tid] = (int32_t)s;
    listed[tid] = s < 0 ? 0u : (uint32_t)(len < K ? len : K);
    size_a[tid] = s < 0 ? 0u : (uint32_t)(off[s + 1] - off[s]);
    positives[tid] = 0;
  }
  __syncthreads();
  for (int i = tid; i < G * FD_MAXK; i += FD_SWEEP_THREADS) {
    const int g = i / FD_MAXK, e = i % FD_MAXK;
    const bool in = (uint32_t)e < listed[g];
    uint32_t *const row = ent + g * FD_REQ_WORDS;
    row[e] = in ? (uint32_t)inter_in[(x0 + g) * FD_MAXK + e] : 0u;
    row[FD_MAXK + e] = in ? (uint32_t)union_in[(x0 + g) * FD_MAXK + e] : 0u;
    row[2 * FD_MAXK + e] = 0;
    row[3 * FD_MAXK + e] = 0;
  }
  fd_stage(off, rows, D, G, sid, ng, bits, flags);
  __syncthreads();

  // The walk is a chain of dependent reads (offsets -> rows -> LDS) with little work per link, so the bounds and the
  // first two trips of rows of the group's NEXT query are requested before the current one is worked on: sets of up to
  // 2 FD_W rows (the mean is about 20) then cost no read on the critical path (1502 -> 889 ms for 16 384 requests at
  // 10 M queries; requesting the bounds a second query ahead as well gave nothing more: 864 - 898 ms).
  const int sub = tid & (FD_W - 1);
  int64_t j = j0 + tid / FD_W, lo, hi;
  uint32_t r0, r1;
  fd_fetch(off, rows, j, j1, sub, lo, hi, r0, r1);
  for (; j < j1; j += FD_SWEEP_GROUPS) {
    int64_t nlo, nhi;
    uint32_t nr0, nr1;
    fd_fetch(off, rows, j + FD_SWEEP_GROUPS, j1, sub, nlo, nhi, nr0, nr1);
    const int64_t len = hi - lo;
    uint32_t mk0 = 0, mk1 = 0;   // the masks of the lane's rows of the first two trips
    if (sub < len) mk0 = fd_test(bits, r0, D, G, flags);
    if (FD_W + sub < len) mk1 = fd_test(bits, r1, D, G, flags);
    uint32_t any = mk0 | mk1;
    for (int64_t p = lo + 2 * FD_W + sub; p < hi; p += FD_W) any |= fd_test(bits, (uint32_t)rows[p], D, G, flags);
#pragma unroll
    for (int dl = FD_W / 2; dl; dl >>= 1) any |= (uint32_t)__shfl_xor((int)any, dl, FD_W);
    while (any) {   // uniform over the group
      const int g = __ffs((int)any) - 1;
      any &= any - 1;
      if ((int64_t)sid[g] == j) continue;
      int32_t cnt = (int32_t)(((mk0 >> g) & 1u) + ((mk1 >> g) & 1u));
      for (int64_t p = lo + 2 * FD_W + sub; p < hi; p += FD_W) {
        const uint32_t r = (uint32_t)rows[p];
        if (r < (uint64_t)D) cnt += (int32_t)((fd_mask(bits, r, G) >> g) & 1u);
      }
#pragma unroll
      for (int dl = FD_W / 2; dl; dl >>= 1) cnt += __shfl_xor(cnt, dl, FD_W);
      const int64_t inter = cnt, uni = (int64_t)size_a[g] + len - inter;
      if (sub == 0) atomicAdd(&positives[g], 1u);
      uint32_t *const row = ent + g * FD_REQ_WORDS;
      const int L = (int)listed[g];
      for (int e = sub; e < L; e += FD_W) {
        const int64_t a = inter * (int64_t)row[FD_MAXK + e], b = (int64_t)row[e] * uni;
        if (a > b) atomicAdd(&row[2 * FD_MAXK + e], 1u);
        else if (a == b) atomicAdd(&row[3 * FD_MAXK + e], 1u);
      }
    }
    lo = nlo;
    hi = nhi;
    r0 = nr0;
    r1 = nr1;
  }
  __syncthreads();
  for (int i = tid; i < ng * FD_MAXK; i += FD_SWEEP_THREADS) {
    const int g = i / FD_MAXK, e = i % FD_MAXK;
    const uint32_t *const row = ent + g * FD_REQ_WORDS;
    const uint32_t be = row[2 * FD_MAXK + e], eq = row[3 * FD_MAXK + e];
    if (be) atomicAdd(&better_out[(x0 + g) * FD_MAXK + e], (int32_t)be);
    if (eq) atomicAdd(&equal_out[(x0 + g) * FD_MAXK + e], (int32_t)eq);
  }
  if (tid < ng && positives[tid])
    atomicAdd(reinterpret_cast<unsigned long long *>(words_out + (x0 + tid) * 8 + 2), (unsigned long long)positives[tid]);
}

__device__ static inline int64_t fd_wave_sum(int64_t v) {
#pragma unroll
  for (int dl = WAVE / 2; dl; dl >>= 1) v += __shfl_xor(v, dl, WAVE);
  return v;
}

// one wave per request, lane e = stored entry e
__global__ __launch_bounds__(FD_THREADS) void fidelity_finish_kernel(
    const int64_t *__restrict__ off, int64_t nq, const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx,
    const int32_t *__restrict__ queries, int64_t m, int K, const int32_t *__restrict__ inter_in,
    const int32_t *__restrict__ union_in, const int32_t *__restrict__ better_in, int32_t *__restrict__ equal_io,
    int64_t *__restrict__ words_io, unsigned long long *__restrict__ totals) {
  const int lane = lane_id();
  const int64_t x = (int64_t)blockIdx.x * (FD_THREADS / WAVE) + threadIdx.x / WAVE;
  if (x >= m) return;   // the whole wave
  int64_t len;
  uint32_t bad;
  const int64_t s = fd_request(queries, x, nq, q_off, len, bad);
  if (s < 0) return;    // its words stay 0
  const int L = (int)(len < K ? len : K);
  const int64_t pos = words_io[x * 8 + 2];
  const bool in = lane < L;
  int64_t ie = 0, ue = 0, be = 0, eq = 0;
  if (in) {
    const int64_t at = x * FD_MAXK + lane;
    ie = inter_in[at];
    ue = union_in[at];
    be = better_in[at];
    eq = equal_io[at];
    if (ie == 0) eq = nq - 1 - pos;          // J_e = 0 ties with every j != s the sweep did not meet
    if ((int64_t)q_idx[q_off[s] + lane] != s) eq -= 1;   // the entry's own target is among the ties
    equal_io[at] = (int32_t)eq;
  }
  int64_t inv = 0;
  for (int f = 1; f < L; ++f) {
    const int64_t fi = __shfl(ie, f, WAVE), fu = __shfl(ue, f, WAVE);
    if (lane < f && ie * fu < fi * ue) ++inv;
  }
  const int64_t hits = fd_wave_sum(in && be < K), sure = fd_wave_sum(in && be + eq < K),
                disjoint = fd_wave_sum(in && ie == 0);
  inv = fd_wave_sum(inv);
  if (lane == 0) {
    const int64_t w[8] = {L, off[s + 1] - off[s], pos, hits, sure, pos < K ? pos : K, disjoint, inv};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      words_io[x * 8 + k] = w[k];
      if (w[k]) atomicAdd(totals + k, (unsigned long long)w[k]);
    }
  }
}

}  // namespace

QRLSH_EXPORT int32_t qrlsh_list_fidelity_group(int64_t D) { return D < 0 || D > FD_MAX_D ? 0 : fd_group(D); }

QRLSH_EXPORT int qrlsh_edge_overlaps(const int64_t *offsets, const int32_t *rows, int64_t nq, const int32_t *src,
                                     const int32_t *dst, int64_t n, int32_t *inter_out, uint32_t *flags_out,
                                     void *stream) {
  QR_CHECK_ARG(n >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_edge_overlaps: bad sizes n=%lld nq=%lld", (long long)n,
               (long long)nq);
  QR_CHECK_ARG(flags_out, "qrlsh_edge_overlaps: flags_out is required");
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(offsets && src && dst && inter_out, "qrlsh_edge_overlaps: null pointer");
  const int64_t blocks = ceil_div64(n, FD_EDGES);
  if (blocks > 2147483647ll) {
    qrlsh_set_error("qrlsh_edge_overlaps: n=%lld above the %lld edges served", (long long)n,
                    2147483647ll * FD_EDGES);
    return QRLSH_EUNSUPPORTED;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_LAUNCH("edge_overlaps", edge_overlaps_kernel, dim3((unsigned)blocks), dim3(FD_THREADS), 0, st, offsets, rows, nq,
            src, dst, n, inter_out, flags_out);
  QR_LAUNCH_CHECK("qrlsh_edge_overlaps");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_list_fidelity(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t D,
                                     const int64_t *q_off, const int32_t *q_idx, const int32_t *queries, int64_t m,
                                     int32_t K, int32_t slices, int32_t *inter_out, int32_t *union_out,
                                     int32_t *better_out, int32_t *equal_out, int64_t *words_out, int64_t *totals_out,
                                     uint32_t *flags_out, void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= FD_MAXK, "qrlsh_list_fidelity: K=%d outside 1..%d", K, FD_MAXK);
  QR_CHECK_ARG(m >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_list_fidelity: bad sizes m=%lld nq=%lld", (long long)m,
               (long long)nq);
  QR_CHECK_ARG(D >= 0 && D <= FD_MAX_D, "qrlsh_list_fidelity: D=%lld outside 0..%lld", (long long)D, (long long)FD_MAX_D);
  QR_CHECK_ARG(slices >= 0 && slices <= FD_MAXS, "qrlsh_list_fidelity: slices=%d outside 0..%d", slices, FD_MAXS);
  QR_CHECK_ARG(flags_out && totals_out, "qrlsh_list_fidelity: flags_out and totals_out are required");
  QR_CHECK_ARG(queries || m <= nq, "qrlsh_list_fidelity: m=%lld requests of %lld queries need `queries`", (long long)m,
               (long long)nq);
  if (m > FD_MAX_M) {
    qrlsh_set_error("qrlsh_list_fidelity: m=%lld above the %lld requests served", (long long)m, (long long)FD_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(offsets && q_off && inter_out && union_out && better_out && equal_out && words_out,
               "qrlsh_list_fidelity: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = fd_group(D);
  const int64_t groups = ceil_div64(m, G), S = fd_slices(groups, nq, slices);
  const int64_t per = nq > 0 ? ceil_div64(nq, S) : 1;
  QR_MEMSET("qrlsh_list_fidelity", better_out, 0, (size_t)m * FD_MAXK * sizeof(int32_t), st);
  QR_MEMSET("qrlsh_list_fidelity", equal_out, 0, (size_t)m * FD_MAXK * sizeof(int32_t), st);
  QR_MEMSET("qrlsh_list_fidelity", words_out, 0, (size_t)m * 8 * sizeof(int64_t), st);
  QR_LAUNCH("fidelity_entries", fidelity_entries_kernel, dim3((unsigned)ceil_div64(m * FD_MAXK, FD_EDGES)),
            dim3(FD_THREADS), 0, st, offsets, rows, nq, q_off, q_idx, queries, m, (int)K, inter_out, union_out,
            flags_out);
  QR_LAUNCH("fidelity_sweep", fidelity_sweep_kernel, dim3((unsigned)groups, (unsigned)S), dim3(FD_SWEEP_THREADS), 0, st,
            offsets, rows, nq, D, q_off, queries, m, (int)K, G, per, (const int32_t *)inter_out,
            (const int32_t *)union_out, better_out, equal_out, words_out, flags_out);
  QR_LAUNCH("fidelity_finish", fidelity_finish_kernel, dim3((unsigned)ceil_div64(m, FD_THREADS / WAVE)),
            dim3(FD_THREADS), 0, st, offsets, nq, q_off, q_idx, queries, m, (int)K, (const int32_t *)inter_out,
            (const int32_t *)union_out, (const int32_t *)better_out, equal_out, words_out,
            reinterpret_cast<unsigned long long *>(totals_out));
  QR_LAUNCH_CHECK("qrlsh_list_fidelity");
  return QRLSH_OK;
}
