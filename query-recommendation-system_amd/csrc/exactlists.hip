// exactlists.hip -- the exact top K by Jaccard over the CSR answer sets, for chosen queries (qrlsh_exact_neighbours; the
// contract is in include/qrlsh.h).  What fidelity.hip measures the served lists against, produced: request x with chosen
// query s gets the j != s that share a row with s, by J(s, j) descending, ties by j ascending, cut at K.  Integer
// arithmetic only (exactkeep.h: the order, the kept list, the threshold word).
//
//   exact_sweep    fidelity_sweep's shape (fidelitywalk.h): a workgroup per (group of G requests, slice of the ids j), the
//                  G answer sets as one interleaved bitmap in LDS, groups of FD_W lanes walking the CSR one query ahead.
//                  The 256 words of a request hold its best K so far, in order, as inter[64] / union[64] / id[64], the
//                  threshold word (the K-th entry's inter << 32 | union, one 64-bit LDS word) and the count.  A (request,
//                  j) whose bit came up has its intersection counted and is compared ONCE, with the threshold; only one
//                  that may enter takes the request's lock and inserts.  The K entries of every (request, slice) leave as
//                  a partial list with plain vector stores, positives with integer atomics.
//   exact_finish   one wave per request: a K-round selection over the heads of its S partial lists under the same total
//                  order (a lane owns up to four slices), the padding and the counts.
//
// The lock ("Exact lists"): one LDS word per request, taken by lane 0 of a lane group in a try-lock
// loop whose critical section -- at most K moves of exactkeep.h's insert, no wait of any kind -- and release sit inside
// the branch of the successful compare-and-swap.  The lanes of one wave that want a lock at the same time go through
// that loop ONE AT A TIME (a ballot, a scalar loop over its bits): a spinning lane is then the only active lane of its
// wave, its lock's holder is a lane of another wave of the same workgroup, every wave of a workgroup is resident, and a
// holder holds one lock, waits on nothing and releases after at most K moves.  A stale threshold is a lower one: it lets
// a candidate through to the lock and the exact comparison there, it never drops one.
#include "exactkeep.h"
#include "fidelitywalk.h"

namespace {

constexpr int EL_THREADS = 256;                  // the finish: four waves, one request each
constexpr int EL_IN = 0, EL_UN = FD_MAXK, EL_ID = 2 * FD_MAXK;   // a request's words: the kept list ...
constexpr int EL_THR = 3 * FD_MAXK;              // ... its threshold (two words, 8-byte aligned) ...
constexpr int EL_N = 3 * FD_MAXK + 2;            // ... and its count
static_assert(EL_N < FD_REQ_WORDS && (FD_FIXED_WORDS + EL_THR) % 2 == 0 && FD_REQ_WORDS % 2 == 0, "a request's words");
static_assert(FD_MAXS <= 4 * WAVE, "a lane of the finish owns up to four slices");

// where the partial list of (request x, slice y) starts in the scratch: [3][K] words = inter, union, id
__device__ static inline int64_t el_partial(int64_t x, int64_t S, int64_t y, int K) { return (x * S + y) * 3 * K; }

__global__ __launch_bounds__(FD_SWEEP_THREADS) void exact_sweep_kernel(
    const int64_t *__restrict__ off, const int32_t *__restrict__ rows, int64_t nq, int64_t D,
    const int32_t *__restrict__ queries, int64_t m, int K, int G, int64_t per, int32_t *__restrict__ partial,
    int32_t *__restrict__ counts_out, uint32_t *__restrict__ flags) {
  __shared__ uint32_t lds[FD_LDS_WORDS];
  int32_t *const sid = reinterpret_cast<int32_t *>(lds);   // [FD_MAXG] the chosen query, -1 = not served
  uint32_t *const size_a = lds + FD_MAXG;                  // [FD_MAXG]
  uint32_t *const positives = lds + 2 * FD_MAXG;           // [FD_MAXG]
  uint32_t *const lock = lds + 3 * FD_MAXG;                // [FD_MAXG] 0 = free
  uint32_t *const ent = lds + FD_FIXED_WORDS;              // [G][FD_REQ_WORDS]
  uint32_t *const bits = ent + G * FD_REQ_WORDS;           // ceil(D G / 32) words
  const int tid = threadIdx.x;
  const int64_t x0 = (int64_t)blockIdx.x * G, S = gridDim.y;
  const int ng = (int)(m - x0 < G ? m - x0 : G);
  const int64_t j0 = (int64_t)blockIdx.y * per, j1 = j0 + per < nq ? j0 + per : nq;
  if (j0 >= j1) {   // uniform: a slice without ids still owes its (empty) partial lists
    for (int i = tid; i < ng * K; i += FD_SWEEP_THREADS) {
      int32_t *const out = partial + el_partial(x0 + i / K, S, blockIdx.y, K);
      const int e = i % K;
      out[e] = EK_NONE_INTER;
      out[K + e] = EK_NONE_UNION;
      out[2 * K + e] = EK_NONE_ID;
    }
    return;
  }
  const int bitw = (int)((D * G + 31) / 32);
  for (int i = tid; i < bitw; i += FD_SWEEP_THREADS) bits[i] = 0;
  if (tid < FD_MAXG) {
    int64_t s = -1, len;
    uint32_t bad = 0;
    if (tid < ng) s = fd_request(queries, x0 + tid, nq, nullptr, len, bad);
    if (bad && blockIdx.y == 0) atomicOr(flags, bad);
    sid[tid] = (int32_t)s;
    size_a[tid] = s < 0 ? 0u : (uint32_t)(off[s + 1] - off[s]);
    positives[tid] = 0;
    lock[tid] = 0;
    if (tid < G) {
      uint32_t *const row = ent + tid * FD_REQ_WORDS;
      row[EL_N] = 0;
      __hip_atomic_store(reinterpret_cast<uint64_t *>(row + EL_THR), ek_threshold(EK_NONE_INTER, EK_NONE_UNION),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  fd_stage(off, rows, D, G, sid, ng, bits, flags);
  __syncthreads();

  // the walk of fidelity_sweep_kernel: the bounds and the first two trips of rows of the group's next query are requested
  // before the current one is worked on
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
      if (sub != 0) continue;   // one lane of the group takes the candidate on
      const int32_t inter = cnt, uni = (int32_t)((int64_t)size_a[g] + len - cnt);
      atomicAdd(&positives[g], 1u);
      uint32_t *const row = ent + g * FD_REQ_WORDS;
      uint64_t *const thr = reinterpret_cast<uint64_t *>(row + EL_THR);
      // the one comparison per positive; a stale word is a lower one
      const bool want = ek_may_enter(inter, uni, __hip_atomic_load(thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      // One lane of the WAVE at a time: the lanes that want a lock here take turns by a ballot, a scalar loop.  Two lanes
      // of one wave never contend, so the compiler is free to move the critical section behind the spin (it does) without
      // a holder ever sitting masked off beside a spinning lane of its own wave.
      for (unsigned long long turn = __ballot(want); turn; turn &= turn - 1) {
        if (lane_id() != __ffsll(turn) - 1) continue;
        for (bool done = false; !done;) {
          uint32_t expect = 0;
          if (__hip_atomic_compare_exchange_strong(&lock[g], &expect, 1u, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP)) {
            const int n = ek_insert(row + EL_IN, row + EL_UN, row + EL_ID, (int)row[EL_N], K, inter, uni, (int32_t)j);
            row[EL_N] = (uint32_t)n;
            if (n == K)
              __hip_atomic_store(thr, ek_threshold((int32_t)row[EL_IN + K - 1], (int32_t)row[EL_UN + K - 1]),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(&lock[g], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            done = true;
          }
        }
      }
    }
    lo = nlo;
    hi = nhi;
    r0 = nr0;
    r1 = nr1;
  }
  __syncthreads();
  for (int i = tid; i < ng * K; i += FD_SWEEP_THREADS) {
    const int g = i / K, e = i % K;
    const uint32_t *const row = ent + g * FD_REQ_WORDS;
    const bool in = (uint32_t)e < row[EL_N];
    int32_t *const out = partial + el_partial(x0 + g, S, blockIdx.y, K);
    out[e] = in ? (int32_t)row[EL_IN + e] : EK_NONE_INTER;
    out[K + e] = in ? (int32_t)row[EL_UN + e] : EK_NONE_UNION;
    out[2 * K + e] = in ? (int32_t)row[EL_ID + e] : EK_NONE_ID;
  }
  if (tid < ng && positives[tid]) atomicAdd(&counts_out[(x0 + tid) * 2 + 1], (int32_t)positives[tid]);
}

// one wave per request: lane l owns slices l, l + 64, l + 128, l + 192; round e takes the first of all heads
__global__ __launch_bounds__(EL_THREADS) void exact_finish_kernel(const int32_t *__restrict__ partial, int64_t m, int K,
                                                                   int64_t S, int32_t *__restrict__ dst_out,
                                                                   int32_t *__restrict__ inter_out,
                                                                   int32_t *__restrict__ union_out,
                                                                   int32_t *__restrict__ counts_io) {
  const int lane = lane_id();
  const int64_t x = (int64_t)blockIdx.x * (EL_THREADS / WAVE) + threadIdx.x / WAVE;
  if (x >= m) return;   // the whole wave
  int32_t hi_[4], hu[4], hd[4];
  int at[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t y = lane + c * WAVE;
    at[c] = 0;
    hi_[c] = EK_NONE_INTER;
    hu[c] = EK_NONE_UNION;
    hd[c] = EK_NONE_ID;
    if (y < S) {
      const int32_t *const p = partial + el_partial(x, S, y, K);
      hi_[c] = p[0];
      hu[c] = p[K];
      hd[c] = p[2 * K];
    }
  }
  int32_t oi = 0, ou = 0, od = -1;   // lane e keeps round e's entry
  int listed = 0;
  for (int e = 0; e < K; ++e) {
    int32_t bi = hi_[0], bu = hu[0], bd = hd[0];
    int own = lane * 4;   // lane * 4 + c: whose head it is
#pragma unroll
    for (int c = 1; c < 4; ++c)
      if (ek_before(hi_[c], hu[c], hd[c], bi, bu, bd)) {
        bi = hi_[c];
        bu = hu[c];
        bd = hd[c];
        own = lane * 4 + c;
      }
#pragma unroll
    for (int dl = WAVE / 2; dl; dl >>= 1) {
      const int32_t ti = __shfl_xor(bi, dl, WAVE), tu = __shfl_xor(bu, dl, WAVE), td = __shfl_xor(bd, dl, WAVE);
      const int town = __shfl_xor(own, dl, WAVE);
      if (ek_before(ti, tu, td, bi, bu, bd)) {   // ids are distinct across heads: every lane ends with the same entry
        bi = ti;
        bu = tu;
        bd = td;
        own = town;
      }
    }
    if (bi == EK_NONE_INTER) break;   // uniform: nothing is left in any slice
    ++listed;
    if (lane == e) {
      oi = bi;
      ou = bu;
      od = bd;
    }
    if (own / 4 == lane) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c == (own & 3)) {
          ++at[c];
          hi_[c] = EK_NONE_INTER;
          hu[c] = EK_NONE_UNION;
          hd[c] = EK_NONE_ID;
          if (at[c] < K) {
            const int32_t *const p = partial + el_partial(x, S, lane + c * WAVE, K) + at[c];
            hi_[c] = p[0];
            hu[c] = p[K];
            hd[c] = p[2 * K];
          }
        }
    }
  }
  if (lane < K) {
    dst_out[x * K + lane] = od;
    inter_out[x * K + lane] = oi;
    union_out[x * K + lane] = ou;
  }
  if (lane == 0) counts_io[x * 2] = listed;
}

struct ExactWs {
  int32_t *partial;   // [m][S][3][K]
};
static ExactWs exact_layout(QrCarve &c, int64_t m, int64_t S, int K) {
  ExactWs w;
  w.partial = c.take<int32_t>((size_t)m * (size_t)S * (size_t)K * 3, 4);   // the header's formula, to the word
  return w;
}

bool el_sizes_ok(int64_t nq, int64_t m, int64_t D, int32_t slices) {
  return nq >= 0 && nq <= 2147483647ll && m >= 0 && D >= 0 && D <= FD_MAX_D && slices >= 0 && slices <= FD_MAXS;
}

}  // namespace

QRLSH_EXPORT int32_t qrlsh_exact_neighbours_slices(int64_t nq, int64_t m, int64_t D, int32_t slices) {
  if (!el_sizes_ok(nq, m, D, slices) || m > FD_MAX_M) return 0;
  return (int32_t)fd_slices(ceil_div64(m, fd_group(D)), nq, slices);
}

QRLSH_EXPORT int qrlsh_exact_neighbours(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t D,
                                        const int32_t *queries, int64_t m, int32_t K, int32_t slices, int32_t *dst_out,
                                        int32_t *inter_out, int32_t *union_out, int32_t *counts_out, uint32_t *flags_out,
                                        void *scratch, size_t scratch_bytes, void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= FD_MAXK, "qrlsh_exact_neighbours: K=%d outside 1..%d", K, FD_MAXK);
  QR_CHECK_ARG(el_sizes_ok(nq, m, D, slices), "qrlsh_exact_neighbours: bad sizes m=%lld nq=%lld D=%lld slices=%d",
               (long long)m, (long long)nq, (long long)D, slices);
  QR_CHECK_ARG(flags_out, "qrlsh_exact_neighbours: flags_out is required");
  QR_CHECK_ARG(queries || m <= nq, "qrlsh_exact_neighbours: m=%lld requests of %lld queries need `queries`", (long long)m,
               (long long)nq);
  if (m > FD_MAX_M) {
    qrlsh_set_error("qrlsh_exact_neighbours: m=%lld above the %lld requests served", (long long)m, (long long)FD_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  if (m == 0 || nq == 0) return QRLSH_OK;
  QR_CHECK_ARG(offsets && dst_out && inter_out && union_out && counts_out, "qrlsh_exact_neighbours: null pointer");
  const int G = fd_group(D);
  const int64_t groups = ceil_div64(m, G), S = fd_slices(groups, nq, slices);
  const int64_t per = ceil_div64(nq, S);
  QR_CHECK_WORKSPACE("qrlsh_exact_neighbours", scratch, scratch_bytes, QR_LAYOUT_BYTES(exact_layout, m, S, (int)K));
  QR_CHECK_ALIGNED("qrlsh_exact_neighbours", "scratch", qr_addr(scratch), 4);
  QrCarve carve(scratch);
  const ExactWs ws = exact_layout(carve, m, S, (int)K);
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_exact_neighbours", counts_out, 0, (size_t)m * 2 * sizeof(int32_t), st);
  QR_LAUNCH("exact_sweep", exact_sweep_kernel, dim3((unsigned)groups, (unsigned)S), dim3(FD_SWEEP_THREADS), 0, st, offsets,
            rows, nq, D, queries, m, (int)K, G, per, ws.partial, counts_out, flags_out);
  QR_LAUNCH("exact_finish", exact_finish_kernel, dim3((unsigned)ceil_div64(m, EL_THREADS / WAVE)), dim3(EL_THREADS), 0, st,
            (const int32_t *)ws.partial, m, (int)K, S, dst_out, inter_out, union_out, counts_out);
  QR_LAUNCH_CHECK("qrlsh_exact_neighbours");
  return QRLSH_OK;
}
