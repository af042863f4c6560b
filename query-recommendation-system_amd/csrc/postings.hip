// postings.hip -- the exact neighbour lists served from a row -> queries index of the answer sets (the "postings"), and
// that index built on the device (qrlsh_answer_postings, qrlsh_exact_neighbours_postings; the contracts are in
// include/qrlsh.h).  The output is word for word exactlists.hip's; the work follows a request's own matches instead of a
// sweep over all queries: inter(s, j) is the number of posting lists of s's rows that hold j, |A(j)| a difference of two
// offsets, so A(j) is never walked.  Integer arithmetic only (exactkeep.h: the order and the threshold word;
// postingsplan.h: the windows).
//
//   postings_offsets_check   offsets is a CSR over nnz entries, or flag bit 5
//   postings_expand          one word row << 32 | query per CSR entry, in CSR order (a row id outside [0, D): flag bit 3, the
//                            word carries row 0).  qrlsh_sort_u64 over bits [32, 32 + bits(D)) then groups by row; the sort
//                            is stable, so the queries of a row stay ascending.
//   postings_unpack          p_qry from the low words, p_off[d] = the first sorted position whose row is >= d (a binary
//                            search per d: empty rows anywhere come out right, nnz = 0 writes zeros)
//   exact_postings           one workgroup per request ("Exact lists from postings"): windows of ids
//                            by postingsplan.h's rule, multiplicities counted in an LDS hash table, a walk over the slots
//                            that drops a candidate whose bound inter / |A(s)| is below the kept list's K-th entry before
//                            anything is gathered, survivors through an LDS queue (an atomic cursor; drained between
//                            workgroup barriers, the walk repeated for what did not fit), the kept list in the
//                            registers of one wave, under exactkeep.h's order.
// No lock and no wait on another thread anywhere: every loop around a barrier has a workgroup-uniform trip count, the table
// probe ends after at most PP_TABLE_SLOTS steps on its own.
#include "common.h"
#include "exactkeep.h"
#include "postingsplan.h"

namespace {

constexpr int PO_THREADS = 256;                    // the build's kernels
constexpr int PO_PER = 8;                          // CSR entries per thread of the expand
constexpr int PO_TILE = PO_THREADS * PO_PER;
constexpr int64_t PO_MAX_D = 1ll << 20;            // QRLSH_FIDELITY_MAX_D
constexpr int64_t PO_MAX_M = 1ll << 24;            // requests per call, as qrlsh_exact_neighbours
constexpr int PO_MAXK = QRLSH_FIDELITY_MAX_K;
constexpr uint32_t PO_FLAG_QUERY = 4u, PO_FLAG_ROW = 8u, PO_FLAG_POSTINGS = 16u, PO_FLAG_OFFSETS = 32u;

// ---- the build -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PO_THREADS) void postings_offsets_check_kernel(const int64_t *__restrict__ off, int64_t nq,
                                                                             int64_t nnz, uint32_t *__restrict__ flags) {
  const int64_t j = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x;
  if (j > nq) return;
  bool bad = j < nq && off[j] > off[j + 1];
  if (j == 0) bad |= off[0] != 0;
  if (j == nq) bad |= off[nq] != nnz;
  if (bad) atomicOr(flags, PO_FLAG_OFFSETS);
}

// the last j in [jlo, jhi] with off[j] <= p (jlo when there is none): the owner of CSR entry p; inside [jlo, jhi] whatever
// the offsets hold
__device__ static inline int64_t po_owner(const int64_t *__restrict__ off, int64_t jlo, int64_t jhi, int64_t p) {
  while (jlo < jhi) {
    const int64_t mid = jlo + (jhi - jlo + 1) / 2;
    if (off[mid] <= p) jlo = mid;
    else jhi = mid - 1;
  }
  return jlo;
}

// a workgroup takes PO_TILE consecutive entries: the owners of its first and last entry bound every search inside it
__global__ __launch_bounds__(PO_THREADS) void postings_expand_kernel(const int64_t *__restrict__ off,
                                                                      const int32_t *__restrict__ rows, int64_t nq,
                                                                      int64_t nnz, int64_t D, uint64_t *__restrict__ words,
                                                                      uint32_t *__restrict__ flags) {
  __shared__ int64_t range[2];
  const int64_t p0 = (int64_t)blockIdx.x * PO_TILE, p1 = p0 + PO_TILE < nnz ? p0 + PO_TILE : nnz;
  if (threadIdx.x < 2) range[threadIdx.x] = po_owner(off, 0, nq - 1, threadIdx.x ? p1 - 1 : p0);
  __syncthreads();
  const int64_t jlo = range[0], jhi = range[1] < range[0] ? range[0] : range[1];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PO_PER; ++k) {
    const int64_t p = p0 + (int64_t)k * PO_THREADS + threadIdx.x;
    if (p >= p1) break;
    const int64_t j = po_owner(off, jlo, jhi, p);
    uint32_t r = (uint32_t)rows[p];
    if (r >= (uint64_t)D) {
      bad = true;
      r = 0;
    }
    words[p] = (uint64_t)r << 32 | (uint32_t)j;
  }
  if (bad) atomicOr(flags, PO_FLAG_ROW);
}

__global__ __launch_bounds__(PO_THREADS) void postings_unpack_kernel(const uint64_t *__restrict__ words, int64_t nnz,
                                                                      int64_t D, int64_t *__restrict__ p_off,
                                                                      int32_t *__restrict__ p_qry) {
  const int64_t i = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x;
  if (i < nnz) p_qry[i] = (int32_t)(uint32_t)words[i];
  if (i <= D) {
    int64_t b = 0, e = nnz;
    while (b < e) {
      const int64_t mid = b + (e - b) / 2;
      if ((int64_t)(words[mid] >> 32) < i) b = mid + 1;
      else e = mid;
    }
    p_off[i] = b;
  }
}

struct PostingsWs {
  uint64_t *words_a, *words_b;   // [nnz] each: the sort's two sides
  void *sort_ws;
  size_t sort_bytes;
};
static PostingsWs postings_layout(QrCarve &c, int64_t nnz) {
  PostingsWs w;
  w.words_a = c.take<uint64_t>((size_t)nnz);
  w.words_b = c.take<uint64_t>((size_t)nnz);
  w.sort_bytes = qrlsh_sort_workspace_bytes(nnz, 1);
  w.sort_ws = c.take_bytes(w.sort_bytes);
  return w;
}

bool po_build_sizes_ok(int64_t nnz, int64_t D) { return nnz >= 0 && nnz < (1ll << 32) && D >= 0 && D <= PO_MAX_D; }

// ---- the request kernel ---------------------------------------------------------------------------------------------------
constexpr int PX_THREADS = 1024;                   // one workgroup per CU: its LDS is most of the CU's
constexpr int PX_LISTS = 512;                      // posting lists whose cursors stay in LDS; more are read from memory
constexpr int PX_QUEUE = 1024;                     // survivors between two drains
static_assert(PP_TABLE_SLOTS % PX_THREADS == 0 && PX_QUEUE % WAVE == 0, "whole rounds of the walk and of the drain");

struct PxShared {
  int32_t key[PP_TABLE_SLOTS];       // -1 = free
  uint32_t cnt[PP_TABLE_SLOTS];
  int64_t cur[PX_LISTS];             // per list: the first entry not yet served ...
  int64_t wend[PX_LISTS];            // ... the end of the current window ...
  int64_t lend[PX_LISTS];            // ... and of the list
  int32_t q_id[PX_QUEUE], q_in[PX_QUEUE], q_un[PX_QUEUE];   // the queue; q_un = 0: dropped at the exact comparison
  unsigned long long total;          // entries of the window being planned
  unsigned long long thr;            // ek_threshold of the kept list
  uint32_t q_n, positives, bad;
  int64_t s, a, lo_s, nnz;
};
static_assert(sizeof(PxShared) <= 160 * 1024, "the LDS of a gfx950 CU");

// the posting list of row i of the request: [b, e) inside p_qry, empty for a row id outside [0, D) (flag bit 3); the
// bounds are held inside [0, nnz] whatever p_off holds.  A first entry below 0 or a last one at or above nq is flag bit 4.
__device__ static inline void px_list(const int32_t *__restrict__ rows, int64_t lo_s, int64_t i, int64_t D,
                                      const int64_t *__restrict__ p_off, const int32_t *__restrict__ p_qry, int64_t nnz,
                                      int64_t nq, int64_t &b, int64_t &e, uint32_t &bad) {
  b = e = 0;
  const uint32_t r = (uint32_t)rows[lo_s + i];
  if (r >= (uint64_t)D) {
    bad |= PO_FLAG_ROW;
    return;
  }
  b = p_off[r];
  e = p_off[r + 1];
  if (b < 0 || b > nnz || e < b || e > nnz) {
    bad |= PO_FLAG_POSTINGS;
    b = e = 0;
    return;
  }
  if (b < e && (p_qry[b] < 0 || (int64_t)p_qry[e - 1] >= nq)) bad |= PO_FLAG_POSTINGS;
}

__global__ __launch_bounds__(PX_THREADS) void exact_postings_kernel(
    const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t nq, int64_t D,
    const int64_t *__restrict__ p_off, const int32_t *__restrict__ p_qry, const int32_t *__restrict__ queries, int K,
    int32_t *__restrict__ dst_out, int32_t *__restrict__ inter_out, int32_t *__restrict__ union_out,
    int32_t *__restrict__ counts_out, uint32_t *__restrict__ flags) {
  __shared__ PxShared sh;
  const int tid = threadIdx.x;
  const int64_t x = blockIdx.x;
  for (int i = tid; i < PP_TABLE_SLOTS; i += PX_THREADS) {
    sh.key[i] = -1;
    sh.cnt[i] = 0;
  }
  if (tid == 0) {
    const int64_t s = queries ? (int64_t)queries[x] : x;
    const int64_t nnz = off[nq];
    uint32_t bad = 0;
    sh.s = -1;
    sh.a = 0;
    sh.lo_s = 0;
    if (s < 0 || s >= nq) {
      bad = PO_FLAG_QUERY;
    } else {
      sh.s = s;
      sh.lo_s = off[s];
      sh.a = off[s + 1] - off[s];
    }
    if (p_off[0] != 0 || p_off[D] != nnz) bad |= PO_FLAG_POSTINGS;
    sh.nnz = nnz;
    sh.bad = bad;
    sh.total = 0;
    sh.thr = ek_threshold(EK_NONE_INTER, EK_NONE_UNION);
    sh.q_n = 0;
    sh.positives = 0;
  }
  __syncthreads();
  const int64_t s = sh.s, a = sh.a, lo_s = sh.lo_s, nnz = sh.nnz;
  const bool in_lds = a <= PX_LISTS;   // uniform
  uint32_t bad = 0, positives = 0;
  // the kept list of wave 0: lane e holds entry e (lanes at and past K stay EK_NONE), kn entries, wthr its threshold word
  int32_t ki = EK_NONE_INTER, ku = EK_NONE_UNION, kd = EK_NONE_ID;
  int kn = 0;
  unsigned long long wthr = ek_threshold(EK_NONE_INTER, EK_NONE_UNION);

  // the lists' extents: all entries of the request, and (few lists) the cursors
  {
    unsigned long long part = 0;
    for (int64_t i = tid; i < a; i += PX_THREADS) {
      int64_t b, e;
      px_list(rows, lo_s, i, D, p_off, p_qry, nnz, nq, b, e, bad);
      if (in_lds) {
        sh.cur[i] = b;
        sh.wend[i] = b;
        sh.lend[i] = e;
      }
      part += (unsigned long long)(e - b);
    }
    if (part) atomicAdd(&sh.total, part);
  }
  __syncthreads();
  const unsigned long long all = sh.total;
  __syncthreads();
  const int64_t width = pp_width(all, nq, PP_PASS_ENTRIES);
  // lanes per list in the fill: the widest power of two that gives every list of a small request a group of its own
  int L = 1;
  if (in_lds)
    while (L < PX_THREADS && (int64_t)L * 2 * a <= PX_THREADS) L *= 2;
  const int sub = tid & (L - 1), grp = tid / L, ngrp = PX_THREADS / L;
  const int32_t a32 = (int32_t)a;   // a <= D <= 2^20 for distinct rows

  for (int64_t lo = 0; all && lo < nq;) {   // uniform: all, lo and hi are the same in every thread
    int64_t hi = pp_window_end(lo, nq, width);
    unsigned long long count;
    for (;;) {   // plan: the exact entry count of [lo, hi), halved until it is a pass
      if (tid == 0) sh.total = 0;
      __syncthreads();
      unsigned long long part = 0;
      for (int64_t i = tid; i < a; i += PX_THREADS) {
        int64_t b, e;
        if (in_lds) {
          b = sh.cur[i];
          e = pp_lower_bound(p_qry, b, sh.lend[i], hi);
          sh.wend[i] = e;
        } else {
          uint32_t ignore = 0;
          px_list(rows, lo_s, i, D, p_off, p_qry, nnz, nq, b, e, ignore);
          b = pp_lower_bound(p_qry, b, e, lo);
          e = pp_lower_bound(p_qry, b, e, hi);
        }
        part += (unsigned long long)(e - b);
      }
      if (part) atomicAdd(&sh.total, part);
      __syncthreads();
      count = sh.total;
      __syncthreads();
      if (pp_is_pass(count, lo, hi, PP_PASS_ENTRIES)) break;
      hi = pp_halve(lo, hi);
    }
    if (count) {
      // fill: a group of L lanes per list
      for (int64_t i = grp; i < a; i += ngrp) {
        int64_t b, e;
        if (in_lds) {
          b = sh.cur[i];
          e = sh.wend[i];
        } else {
          uint32_t ignore = 0;
          px_list(rows, lo_s, i, D, p_off, p_qry, nnz, nq, b, e, ignore);
          b = pp_lower_bound(p_qry, b, e, lo);
          e = pp_lower_bound(p_qry, b, e, hi);
        }
        for (int64_t p = b + sub; p < e; p += L) {
          const int32_t j = p_qry[p];
          if ((uint32_t)j >= (uint64_t)nq) {
            bad |= PO_FLAG_POSTINGS;   // never a key: it would index offsets
            continue;
          }
          if (j == s) continue;
          uint32_t h = pp_slot((uint32_t)j);
          for (int step = 0; step < PP_TABLE_SLOTS; ++step) {   // at most half the slots are taken: a free one is met
            const int32_t was = atomicCAS(&sh.key[h], -1, j);
            if (was == -1 || was == j) {
              atomicAdd(&sh.cnt[h], 1u);
              break;
            }
            h = (h + 1) & (PP_TABLE_SLOTS - 1);
          }
        }
      }
      __syncthreads();
      // walk: the bound first, survivors to the queue; what does not fit stays in the table for the next round
      for (;;) {   // uniform: ends when a round queued everything it found
        const unsigned long long thr = sh.thr;
        for (int h = tid; h < PP_TABLE_SLOTS; h += PX_THREADS) {
          const int32_t j = sh.key[h];
          if (j < 0) continue;
          const int32_t inter = (int32_t)sh.cnt[h];
          if (ek_may_enter(inter, a32, thr)) {   // union >= |A(s)|: J <= inter / |A(s)|
            const uint32_t at = atomicAdd(&sh.q_n, 1u);
            if (at >= (uint32_t)PX_QUEUE) continue;   // stays
            sh.q_id[at] = j;
            sh.q_in[at] = inter;
          }
          ++positives;
          sh.key[h] = -1;
          sh.cnt[h] = 0;
        }
        __syncthreads();
        const uint32_t asked = sh.q_n, n = asked < (uint32_t)PX_QUEUE ? asked : (uint32_t)PX_QUEUE;
        // drain, all threads: the exact union from two offsets, compared again
        for (uint32_t e = tid; e < n; e += PX_THREADS) {
          const int64_t j = sh.q_id[e];
          const int64_t uni = a + (off[j + 1] - off[j]) - sh.q_in[e];
          sh.q_un[e] = uni > 0 && uni <= 2147483647ll && ek_may_enter(sh.q_in[e], (int32_t)uni, thr) ? (int32_t)uni : 0;
        }
        __syncthreads();
        // drain, one wave: a lane per entry, the entries that still may enter inserted one at a time.  The kept list is in
        // the wave's registers, lane e its entry e: an insert is one comparison per lane, a ballot and a shift by one lane
        if (tid < WAVE) {
          const unsigned long long lanes_k = K == WAVE ? ~0ull : (1ull << K) - 1ull;
          for (uint32_t e0 = 0; e0 < n; e0 += WAVE) {   // uniform over the wave
            const uint32_t e = e0 + (uint32_t)tid;
            const int32_t uni = e < n ? sh.q_un[e] : 0;
            const int32_t inter = e < n ? sh.q_in[e] : 0, id = e < n ? sh.q_id[e] : 0;
            const bool want = uni > 0 && ek_may_enter(inter, uni, wthr);
            for (unsigned long long turn = __ballot(want); turn; turn &= turn - 1) {   // uniform
              const int from = __ffsll(turn) - 1;
              const int32_t ci = __shfl(inter, from), cu = __shfl(uni, from), cd = __shfl(id, from);
              // the lanes whose entry comes after the candidate: a suffix (the list is in order, EK_NONE comes last)
              const unsigned long long after = __ballot(ek_before(ci, cu, cd, ki, ku, kd)) & lanes_k;
              const int32_t pi = __shfl_up(ki, 1), pu = __shfl_up(ku, 1), pd = __shfl_up(kd, 1);
              if (!after) continue;
              const int pos = __ffsll(after) - 1;
              if (tid == pos) {
                ki = ci;
                ku = cu;
                kd = cd;
              } else if (tid > pos && tid < K) {
                ki = pi;
                ku = pu;
                kd = pd;
              }
              if (kn < K) ++kn;
              const int32_t ti = __shfl(ki, K - 1), tu = __shfl(ku, K - 1);
              if (kn == K) wthr = ek_threshold(ti, tu);
            }
          }
          if (tid == 0) {
            sh.q_n = 0;
            sh.thr = wthr;
          }
        }
        __syncthreads();
        if (asked <= (uint32_t)PX_QUEUE) break;
      }
    }
    if (in_lds)
      for (int64_t i = tid; i < a; i += PX_THREADS) sh.cur[i] = sh.wend[i];
    lo = hi;
  }
  // entries past the last window: ids at or above nq in a list that is not ascending
  if (in_lds)
    for (int64_t i = tid; i < a; i += PX_THREADS)
      if (sh.cur[i] != sh.lend[i]) bad |= PO_FLAG_POSTINGS;
  if (positives) atomicAdd(&sh.positives, positives);
  if (bad) atomicOr(&sh.bad, bad);
  __syncthreads();
  if (tid < K) {   // K <= 64: lanes of wave 0, the owners of the kept list
    const bool in = tid < kn;
    dst_out[x * K + tid] = in ? kd : -1;
    inter_out[x * K + tid] = in ? ki : 0;
    union_out[x * K + tid] = in ? ku : 0;
  }
  if (tid == 0) {
    counts_out[x * 2] = kn;
    counts_out[x * 2 + 1] = (int32_t)sh.positives;
    if (sh.bad) atomicOr(flags, sh.bad);
  }
}

}  // namespace

QRLSH_EXPORT size_t qrlsh_answer_postings_scratch_bytes(int64_t nnz, int64_t D) {
  if (!po_build_sizes_ok(nnz, D) || nnz == 0) return 0;
  return QR_LAYOUT_BYTES(postings_layout, nnz);
}

QRLSH_EXPORT int qrlsh_answer_postings(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t nnz, int64_t D,
                                       int64_t *p_off_out, int32_t *p_qry_out, uint32_t *flags_out, void *scratch,
                                       size_t scratch_bytes, void *stream) {
  QR_CHECK_ARG(nq >= 0 && nq <= 2147483647ll && nnz >= 0 && D >= 0 && D <= PO_MAX_D,
               "qrlsh_answer_postings: bad sizes nq=%lld nnz=%lld D=%lld", (long long)nq, (long long)nnz, (long long)D);
  QR_CHECK_ARG(flags_out && offsets && p_off_out, "qrlsh_answer_postings: null pointer");
  QR_CHECK_ARG(nnz == 0 || (rows && p_qry_out && nq > 0), "qrlsh_answer_postings: %lld entries need rows, p_qry_out and a query",
               (long long)nnz);
  if (nnz >= (1ll << 32)) {
    qrlsh_set_error("qrlsh_answer_postings: nnz=%lld above the 2^32 - 1 entries the sort serves", (long long)nnz);
    return QRLSH_EUNSUPPORTED;
  }
  QR_CHECK_WORKSPACE("qrlsh_answer_postings", scratch, scratch_bytes, qrlsh_answer_postings_scratch_bytes(nnz, D));
  QR_CHECK_ALIGNED("qrlsh_answer_postings", "scratch", qr_addr(scratch), 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_LAUNCH("postings_offsets_check", postings_offsets_check_kernel, dim3((unsigned)ceil_div64(nq + 1, PO_THREADS)),
            dim3(PO_THREADS), 0, st, offsets, nq, nnz, flags_out);
  const uint64_t *sorted = nullptr;
  if (nnz > 0) {
    QrCarve carve(scratch);
    const PostingsWs ws = postings_layout(carve, nnz);
    QR_LAUNCH("postings_expand", postings_expand_kernel, dim3((unsigned)ceil_div64(nnz, PO_TILE)), dim3(PO_THREADS), 0, st,
              offsets, rows, nq, nnz, D, ws.words_a, flags_out);
    const int where = qrlsh_sort_u64(ws.words_a, ws.words_b, nullptr, nullptr, nnz, 1, 32, 32 + qr_id_bits(D), 0, 0,
                                     ws.sort_ws, ws.sort_bytes, stream);
    if (where < 0) return where;
    sorted = where ? ws.words_b : ws.words_a;
  }
  const int64_t cover = nnz > D + 1 ? nnz : D + 1;
  QR_LAUNCH("postings_unpack", postings_unpack_kernel, dim3((unsigned)ceil_div64(cover, PO_THREADS)), dim3(PO_THREADS), 0,
            st, sorted, nnz, D, p_off_out, p_qry_out);
  QR_LAUNCH_CHECK("qrlsh_answer_postings");
  return QRLSH_OK;
}

QRLSH_EXPORT int32_t qrlsh_exact_postings_pass_entries(void) { return PP_PASS_ENTRIES; }
QRLSH_EXPORT int32_t qrlsh_exact_postings_list_cursors(void) { return PX_LISTS; }
QRLSH_EXPORT int32_t qrlsh_exact_postings_queue(void) { return PX_QUEUE; }
QRLSH_EXPORT int32_t qrlsh_exact_postings_threads(void) { return PX_THREADS; }

QRLSH_EXPORT size_t qrlsh_exact_postings_scratch_bytes(int64_t nq, int64_t m, int32_t K) {
  (void)nq, (void)m, (void)K;
  return 0;   // the request kernel keeps everything in LDS
}

QRLSH_EXPORT int qrlsh_exact_neighbours_postings(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t D,
                                                 const int64_t *p_off, const int32_t *p_qry, const int32_t *queries,
                                                 int64_t m, int32_t K, int32_t *dst_out, int32_t *inter_out,
                                                 int32_t *union_out, int32_t *counts_out, uint32_t *flags_out, void *scratch,
                                                 size_t scratch_bytes, void *stream) {
  (void)scratch, (void)scratch_bytes;
  QR_CHECK_ARG(K >= 1 && K <= PO_MAXK, "qrlsh_exact_neighbours_postings: K=%d outside 1..%d", K, PO_MAXK);
  QR_CHECK_ARG(nq >= 0 && nq <= 2147483647ll && m >= 0 && D >= 0 && D <= PO_MAX_D,
               "qrlsh_exact_neighbours_postings: bad sizes m=%lld nq=%lld D=%lld", (long long)m, (long long)nq, (long long)D);
  QR_CHECK_ARG(flags_out, "qrlsh_exact_neighbours_postings: flags_out is required");
  QR_CHECK_ARG(queries || m <= nq, "qrlsh_exact_neighbours_postings: m=%lld requests of %lld queries need `queries`",
               (long long)m, (long long)nq);
  if (m > PO_MAX_M) {
    qrlsh_set_error("qrlsh_exact_neighbours_postings: m=%lld above the %lld requests served", (long long)m,
                    (long long)PO_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  if (m == 0 || nq == 0) return QRLSH_OK;
  QR_CHECK_ARG(offsets && p_off && dst_out && inter_out && union_out && counts_out,
               "qrlsh_exact_neighbours_postings: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_LAUNCH("exact_postings", exact_postings_kernel, dim3((unsigned)m), dim3(PX_THREADS), 0, st, offsets, rows, nq, D, p_off,
            p_qry, queries, (int)K, dst_out, inter_out, union_out, counts_out, flags_out);
  QR_LAUNCH_CHECK("qrlsh_exact_neighbours_postings");
  return QRLSH_OK;
}
