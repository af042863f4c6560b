// recommend.hip -- top-k unrated queries for every requested user, read off the completed utility matrix
// (the batch form of recommender.py:357-375; qrlsh_recommend_topk in include/qrlsh.h).
//
// A cell (u, j) is eligible when ratings[u][j] == 0 and pred[u][j] != 0.  Per row the k eligible cells with the
// largest pred, ordered by value descending, then column ascending.  Values are compared as biased keys
// key = (uint32)v ^ 0x80000000 (unsigned order = signed order), sort keys are (~key << 32 | column).
//
// Forms (same results):
//   rows form  (nq <= RC_DIRECT_MAXQ, slices = auto): one workgroup per row gathers the row's eligible cells into
//              LDS, sorts them and writes the first k -- one sweep;
//   slice form: (row, slice) workgroups, a slice = a contiguous run of 16-byte vectors of the row.
//     hist      -- per (row, slice) LDS histogram of the eligible keys over RC_BINS exact bins [base, base + RC_BINS)
//                  plus a "below" and an "above" bin (window pass: base = lo);
//     threshold -- per row, sums the slices' histograms and walks down from the top to the bin where k is reached.
//                  A bin of one value: the threshold t, and every slice's quota of its cells equal to t (the ties
//                  with the smallest columns: slices take them in slice order).  The below / above bin (values
//                  outside the window): radix rounds over the key, digits 12 / 12 / 8 from the top, each round
//                  restricted to the prefix found so far (three more hist + threshold launches that return at once
//                  for rows already resolved; the decision is on the device, no read-back);
//     emit      -- cells > t (fewer than k) and the slices' ties up to their quotas into the row's k candidates
//                  (the one slice that takes only part of its ties takes them in column order, block-wide scan);
//     finish    -- per row, bitonic sort of the <= k candidates in LDS, padded output.
//
// COMPACT (qrlsh_recommend_users): the rows come from a compact [m][stride] buffer of eligible-mode predictions
// (0 where rated: predict_users_kernel) instead of the two matrices -- row x of the buffer is request x, a cell is
// eligible when it is not 0, and no ratings are read; `users` only tells a bad id (avail -1) from a served one.
#include "common.h"

namespace {
constexpr int RC_THREADS = 256;
constexpr int RC_BINS = 4096;              // exact bins of one histogram round (12 bits)
constexpr int RC_BELOW = RC_BINS;          // keys below the round's range
constexpr int RC_ABOVE = RC_BINS + 1;      // keys above it
constexpr int RC_HSTRIDE = RC_BINS + 4;    // words per histogram (a 16-byte multiple)
constexpr int RC_MAXS = 256;               // slices per row (one per thread of the threshold kernel)
constexpr int RC_DIRECT_MAXQ = 2048;       // rows form up to this many columns
constexpr int RC_SORT_CAP = 2048;          // LDS sort capacity (>= RC_DIRECT_MAXQ, >= QRLSH_RECOMMEND_MAX_K)
constexpr int64_t RC_MAX_GROUPS = 1ll << 24;  // m x slices workgroups served (32-bit grid and thread counts)
constexpr int RC_AUTO_GROUPS = 2048;       // auto slicing aims at 8 workgroups per CU
constexpr int64_t RC_MIN_SLICE_COLS = 8192;

constexpr uint32_t RC_PENDING = 0, RC_ALL = 1, RC_THRESH = 2, RC_BAD = 3;

struct RowState {      // one per requested row, written by the threshold kernel
  uint32_t mode;       // RC_PENDING (another radix round), RC_ALL (avail <= k), RC_THRESH, RC_BAD (user id)
  uint32_t base, shift, nbins;  // the next round's range (RC_PENDING)
  uint32_t t;          // threshold key (RC_THRESH)
  uint32_t ucount;     // candidates placed in any order: [0, ucount); the partial slice's ties follow
  uint32_t avail;      // eligible cells of the row
  uint32_t cnt;        // emit's position counter
  uint32_t pad[8];
};
static_assert(sizeof(RowState) == 64, "RowState is 64 bytes");

__device__ __forceinline__ uint64_t rc_sort_key(uint32_t key, uint32_t col) {
  return ((uint64_t)(~key) << 32) | col;
}
__device__ __forceinline__ int32_t rc_key_value(uint64_t sk) { return (int32_t)(~(uint32_t)(sk >> 32) ^ 0x80000000u); }

// The columns of slice s of S of one row, in column order, four at a time: f(col0, r[4], p[4], n) with n valid
// items at columns col0 .. col0 + n - 1.  Every thread of the block makes the same number of calls (n may be 0),
// and the calls go in column order (head, vector steps, tail; threads in order inside a call), so f may hold
// block-wide scans.  Rows start anywhere: the body from the first 16-byte-aligned column on is read as int4 (the two
// matrices have the same alignment phase: both base pointers are 16-byte aligned), the <= 3 columns before it by
// slice 0, the <= 3 after it by slice S - 1.  RATED = false: there is no ratings row (rr is not read, r stays 0).
template <bool RATED, typename F>
__device__ __forceinline__ void rc_sweep(const int32_t *__restrict__ rr, const int32_t *__restrict__ pr, int64_t nq,
                                         int s, int S, F &&f) {
  const int tid = threadIdx.x;
  int64_t a0 = (int64_t)(((16u - ((uint32_t)(uintptr_t)pr & 15u)) & 15u) >> 2);
  if (a0 > nq) a0 = nq;
  const int64_t nv = (nq - a0) >> 2;
  const int64_t vb = nv * s / S, ve = nv * (s + 1) / S;
  int r[4] = {0, 0, 0, 0}, p[4] = {0, 0, 0, 0};
  if (s == 0 && a0 > 0) {
    const int n = tid < a0 ? 1 : 0;
    if (n) {
      if (RATED) r[0] = rr[tid];
      p[0] = pr[tid];
    }
    f((int64_t)tid, r, p, n);
  }
  const int4 *rv = RATED ? reinterpret_cast<const int4 *>(rr + a0) : nullptr;
  const int4 *pv = reinterpret_cast<const int4 *>(pr + a0);
  for (int64_t v = vb; v < ve; v += 2 * RC_THREADS) {
    const int64_t va = v + tid, vc = v + RC_THREADS + tid;
    int4 ra = make_int4(0, 0, 0, 0), pa = ra, rc = ra, pc = ra;
    if (va < ve) {
      if (RATED) ra = rv[va];
      pa = pv[va];
    }
    if (vc < ve) {
      if (RATED) rc = rv[vc];
      pc = pv[vc];
    }
    int r0[4] = {ra.x, ra.y, ra.z, ra.w}, p0[4] = {pa.x, pa.y, pa.z, pa.w};
    f(a0 + 4 * va, r0, p0, va < ve ? 4 : 0);
    int r1[4] = {rc.x, rc.y, rc.z, rc.w}, p1[4] = {pc.x, pc.y, pc.z, pc.w};
    f(a0 + 4 * vc, r1, p1, vc < ve ? 4 : 0);
  }
  const int64_t t0 = a0 + 4 * nv;
  if (s == S - 1 && t0 < nq) {
    const int n = t0 + tid < nq ? 1 : 0;
    r[0] = p[0] = 0;
    if (n) {
      if (RATED) r[0] = rr[t0 + tid];
      p[0] = pr[t0 + tid];
    }
    f(t0 + tid, r, p, n);
  }
}

// ascending bitonic sort of P (a power of two <= RC_SORT_CAP) keys in LDS by the whole block
__device__ void rc_block_sort(uint64_t *keys, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < (P >> 1); i += RC_THREADS) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == asc) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
}

// n keys sorted in keys[0 .. P): row `row` of the outputs gets the first min(k, n), padding idx -1 / val 0
__device__ void rc_write_row(const uint64_t *keys, int n, int k, int64_t row, int32_t *__restrict__ idx_out,
                             int32_t *__restrict__ val_out) {
  for (int j = threadIdx.x; j < k; j += RC_THREADS) {
    const bool in = j < n;
    const uint64_t sk = in ? keys[j] : 0;
    idx_out[row * k + j] = in ? (int32_t)(uint32_t)sk : -1;
    val_out[row * k + j] = in ? rc_key_value(sk) : 0;
  }
}

__device__ __forceinline__ int rc_pow2(int n) {
  int P = 1;
  while (P < n) P <<= 1;
  return P;
}

// ---- rows form ---------------------------------------------------------------------------------------------------
template <bool COMPACT>
__global__ __launch_bounds__(RC_THREADS) void recommend_rows_kernel(const int32_t *__restrict__ ratings,
                                                                   const int32_t *__restrict__ pred, int64_t nu,
                                                                   int64_t nq, int64_t stride,
                                                                   const int32_t *__restrict__ users, int k,
                                                                   int32_t *__restrict__ idx_out,
                                                                   int32_t *__restrict__ val_out,
                                                                   int32_t *__restrict__ avail_out) {
  __shared__ uint64_t keys[RC_SORT_CAP];
  __shared__ uint32_t n_s;
  const int64_t row = blockIdx.x;
  const int64_t u = users ? (int64_t)users[row] : row;
  const bool bad = u < 0 || u >= nu;
  if (threadIdx.x == 0) n_s = 0;
  __syncthreads();
  if (!bad) {
    const int32_t *rr = COMPACT ? nullptr : ratings + u * nq, *pr = pred + (COMPACT ? row : u) * stride;
    for (int64_t c = threadIdx.x; c < nq; c += RC_THREADS) {
      const int32_t r = COMPACT ? 0 : rr[c], p = pr[c];
      if (r == 0 && p != 0) keys[atomicAdd(&n_s, 1u)] = rc_sort_key((uint32_t)p ^ 0x80000000u, (uint32_t)c);
    }
  }
  __syncthreads();
  const int n = (int)n_s, P = rc_pow2(n);
  for (int i = n + threadIdx.x; i < P; i += RC_THREADS) keys[i] = ~0ull;
  __syncthreads();
  rc_block_sort(keys, P);
  rc_write_row(keys, n, k, row, idx_out, val_out);
  if (threadIdx.x == 0) avail_out[row] = bad ? -1 : n;
}

// ---- slice form --------------------------------------------------------------------------------------------------
// pass 0: the window [lo_key, lo_key + RC_BINS); passes 1-3: the radix round st[row] names (rows not pending return)
template <bool COMPACT>
__global__ __launch_bounds__(RC_THREADS) void recommend_hist_kernel(const int32_t *__restrict__ ratings,
                                                                   const int32_t *__restrict__ pred, int64_t nu,
                                                                   int64_t nq, int64_t stride,
                                                                   const int32_t *__restrict__ users, int S,
                                                                   int pass, uint32_t lo_key,
                                                                   const RowState *__restrict__ st,
                                                                   uint32_t *__restrict__ hist,
                                                                   uint32_t *__restrict__ rowhist) {
  __shared__ uint32_t h[RC_HSTRIDE];
  const int64_t row = blockIdx.x / S;
  const int s = (int)(blockIdx.x - row * S);
  uint32_t base = lo_key, shift = 0, nbins = RC_BINS;
  if (pass > 0) {
    if (st[row].mode != RC_PENDING) return;
    base = st[row].base;
    shift = st[row].shift;
    nbins = st[row].nbins;
  }
  for (int i = threadIdx.x; i < RC_HSTRIDE; i += RC_THREADS) h[i] = 0;
  __syncthreads();
  const int64_t u = users ? (int64_t)users[row] : row;
  if (u >= 0 && u < nu) {
    rc_sweep<!COMPACT>(COMPACT ? nullptr : ratings + u * nq, pred + (COMPACT ? row : u) * stride, nq, s, S,
                       [&](int64_t, const int *r, const int *p, int n) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n && r[j] == 0 && p[j] != 0) {
          const uint32_t key = (uint32_t)p[j] ^ 0x80000000u;
          uint32_t b = RC_BELOW;
          if (key >= base) {
            const uint32_t d = (key - base) >> shift;
            b = d < nbins ? d : (uint32_t)RC_ABOVE;
          }
          atomicAdd(&h[b], 1u);
        }
    });
  }
  __syncthreads();
  uint32_t *out = hist + (size_t)blockIdx.x * RC_HSTRIDE;
  uint32_t *acc = rowhist + (size_t)row * RC_HSTRIDE;
  for (int i = threadIdx.x; i < RC_HSTRIDE; i += RC_THREADS) {
    const uint32_t c = h[i];
    out[i] = c;
    if (S > 1 && c) atomicAdd(&acc[i], c);
  }
}

// one workgroup per row: find the bin where the count from the top reaches k; resolve the row or set the next round
__global__ __launch_bounds__(RC_THREADS) void recommend_threshold_kernel(int64_t nu, const int32_t *__restrict__ users,
                                                                        int k, int S, int pass, uint32_t lo_key,
                                                                        RowState *__restrict__ st,
                                                                        const uint32_t *__restrict__ hist,
                                                                        uint32_t *__restrict__ rowhist,
                                                                        int32_t *__restrict__ tq) {
  __shared__ uint64_t sm[4];
  __shared__ uint32_t found[2];
  __shared__ uint32_t partial_s;
  const int64_t row = blockIdx.x;
  const int t = threadIdx.x;
  RowState *q = st + row;
  uint32_t base = lo_key, shift = 0;
  if (pass > 0) {
    if (q->mode != RC_PENDING) return;
    base = q->base;
    shift = q->shift;
  } else {
    const int64_t u = users ? (int64_t)users[row] : row;
    if (u < 0 || u >= nu) {
      if (t == 0) {
        q->mode = RC_BAD;
        q->avail = 0;
      }
      return;
    }
  }
  uint32_t *rh = S > 1 ? rowhist + (size_t)row * RC_HSTRIDE : const_cast<uint32_t *>(hist) + (size_t)row * RC_HSTRIDE;
  // thread t holds bins [RC_BINS - 16 (t + 1), RC_BINS - 16 t), c[0] the highest
  uint32_t c[16], sum = 0;
  const int top = RC_BINS - 16 * t - 1;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    c[j] = rh[top - j];
    sum += c[j];
  }
  const uint32_t below = rh[RC_BELOW], above = rh[RC_ABOVE];
  if (t == 0) {
    found[0] = 0xFFFFFFFFu;
    partial_s = 0;
  }
  uint64_t inbins;
  const uint64_t before = block_excl_scan_u64_256(sum, sm, &inbins);   // ends with a barrier
  const uint64_t avail = inbins + below + above;
  if (pass == 0 && avail <= (uint64_t)k) {
    if (t == 0) {
      q->mode = RC_ALL;
      q->avail = (uint32_t)avail;
      q->ucount = (uint32_t)avail;
      q->cnt = 0;
    }
    return;
  }
  uint64_t run = above + before;
  if (run < (uint64_t)k && run + sum >= (uint64_t)k) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (run + c[j] >= (uint64_t)k) {
        found[0] = (uint32_t)(top - j);
        found[1] = (uint32_t)run;
        break;
      }
      run += c[j];
    }
  }
  __syncthreads();
  const uint32_t bin = found[0];
  if (bin == 0xFFFFFFFFu || shift > 0) {
    // another radix round: from the top digit when the window missed, else one digit further under the prefix
    if (t == 0) {
      if (pass == 0) q->avail = (uint32_t)avail;
      if (bin == 0xFFFFFFFFu) {
        q->base = 0;
        q->shift = 20;
        q->nbins = RC_BINS;
      } else {
        q->base = base + (bin << shift);
        q->shift = shift == 20 ? 8 : 0;
        q->nbins = shift == 20 ? RC_BINS : 256;
      }
      q->mode = RC_PENDING;
    }
    if (S > 1)
      for (int i = t; i < RC_HSTRIDE; i += RC_THREADS) rh[i] = 0;
    return;
  }
  // resolved: t = base + bin; gt cells above it, quota = k - gt ties, taken by the slices in slice order
  const uint32_t gt = found[1], quota = (uint32_t)k - gt;
  const uint32_t cs = t < S ? hist[((size_t)row * S + t) * RC_HSTRIDE + bin] : 0;
  uint64_t total;
  const uint64_t tb = block_excl_scan_u64_256(cs, sm, &total);
  if (t < S) {
    const uint32_t take = tb >= quota ? 0u : min(cs, quota - (uint32_t)tb);
    tq[(size_t)row * S + t] = take == cs ? (cs ? -1 : 0) : (int32_t)take;
    if (take != cs && take > 0) partial_s = take;   // at most one slice takes part of its ties
  }
  __syncthreads();
  if (t == 0) {
    if (pass == 0) q->avail = (uint32_t)avail;
    q->t = base + bin;
    q->ucount = (uint32_t)k - partial_s;
    q->cnt = 0;
    q->mode = RC_THRESH;
  }
}

// wave-aggregated append of the keys sk[j] with bit j of `mask` set (any order), at positions from *cnt
__device__ __forceinline__ void rc_append(uint32_t *cnt, uint64_t *out, const uint64_t *sk, uint32_t mask) {
  const int n = __popc(mask);
  if (!__any(n > 0)) return;
  const uint64_t inc = wave_incl_scan((uint64_t)n);
  const uint64_t tot = __shfl(inc, WAVE - 1, WAVE);
  uint32_t base = 0;
  if (lane_id() == WAVE - 1) base = atomicAdd(cnt, (uint32_t)tot);
  base = __shfl(base, WAVE - 1, WAVE);
  uint32_t pos = base + (uint32_t)(inc - n);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (mask >> j & 1u) out[pos++] = sk[j];
}

template <bool COMPACT>
__global__ __launch_bounds__(RC_THREADS) void recommend_emit_kernel(const int32_t *__restrict__ ratings,
                                                                   const int32_t *__restrict__ pred, int64_t nq,
                                                                   int64_t stride, const int32_t *__restrict__ users,
                                                                   int k, int S,
                                                                   RowState *__restrict__ st,
                                                                   const int32_t *__restrict__ tq,
                                                                   uint64_t *__restrict__ cand) {
  __shared__ uint64_t sm[4];
  const int64_t row = blockIdx.x / S;
  const int s = (int)(blockIdx.x - row * S);
  const uint32_t mode = st[row].mode;
  if (mode != RC_ALL && mode != RC_THRESH) return;
  const int64_t u = users ? (int64_t)users[row] : row;   // in range: the threshold kernel checked it
  const bool all = mode == RC_ALL;
  const uint32_t thr = all ? 0u : st[row].t;
  const int32_t quota = all ? -1 : tq[(size_t)row * S + s];   // -1 every tie, 0 none, > 0 the first `quota`
  const uint32_t ucount = st[row].ucount;
  uint32_t *cnt = &st[row].cnt;
  uint64_t *out = cand + (size_t)row * k;
  uint64_t taken = 0;   // ordered ties seen so far (block-uniform)
  rc_sweep<!COMPACT>(COMPACT ? nullptr : ratings + u * nq, pred + (COMPACT ? row : u) * stride, nq, s, S,
                     [&](int64_t col0, const int *r, const int *p, int n) {
    uint64_t sk[4];
    uint32_t many = 0, mtie = 0;   // bit j: cell j goes in any order / is a tie of a partially taken slice
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t key = (uint32_t)p[j] ^ 0x80000000u;
      sk[j] = rc_sort_key(key, (uint32_t)(col0 + j));
      if (j < n && r[j] == 0 && p[j] != 0) {
        if (all || key > thr || (key == thr && quota < 0)) many |= 1u << j;
        else if (key == thr && quota > 0) mtie |= 1u << j;
      }
    }
    rc_append(cnt, out, sk, many);
    if (quota > 0 && taken < (uint64_t)quota) {
      uint64_t tot;
      uint64_t pos = taken + block_excl_scan_u64_256((uint64_t)__popc(mtie), sm, &tot);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (mtie >> j & 1u) {
          if (pos < (uint64_t)quota) out[ucount + pos] = sk[j];
          ++pos;
        }
      taken += tot;
    }
  });
}

__global__ __launch_bounds__(RC_THREADS) void recommend_finish_kernel(int k, const RowState *__restrict__ st,
                                                                     const uint64_t *__restrict__ cand,
                                                                     int32_t *__restrict__ idx_out,
                                                                     int32_t *__restrict__ val_out,
                                                                     int32_t *__restrict__ avail_out) {
  __shared__ uint64_t keys[QRLSH_RECOMMEND_MAX_K];
  const int64_t row = blockIdx.x;
  const uint32_t mode = st[row].mode;
  const int n = mode == RC_ALL ? (int)st[row].avail : mode == RC_THRESH ? k : 0;
  const int P = rc_pow2(n);
  for (int i = threadIdx.x; i < P; i += RC_THREADS) keys[i] = i < n ? cand[(size_t)row * k + i] : ~0ull;
  __syncthreads();
  rc_block_sort(keys, P);
  rc_write_row(keys, n, k, row, idx_out, val_out);
  if (threadIdx.x == 0) avail_out[row] = mode == RC_BAD ? -1 : (int32_t)st[row].avail;
}

// slices of the slice form; 0 = rows form
int64_t rc_slices(int64_t m, int64_t nq, int32_t slices) {
  if (slices > 0) return slices;
  if (nq <= RC_DIRECT_MAXQ) return 0;
  int64_t S = RC_AUTO_GROUPS / (m > 0 ? m : 1);   // 2000 rows: one slice each; 8 rows: 256
  const int64_t most = ceil_div64(nq, RC_MIN_SLICE_COLS);
  if (S > most) S = most;
  if (S > RC_MAXS) S = RC_MAXS;
  return S < 1 ? 1 : S;
}

constexpr size_t RC_ALIGN = 256;   // every region of this file's workspaces is rounded up to it

// workspace: [RowState m][candidates m x k u64][histograms m x S][row sums m (S > 1)][tie quotas m x S int32]
struct RcWs {
  RowState *rs;
  uint64_t *cand;
  uint32_t *hist, *rowhist;
  int32_t *tq;
};
RcWs rc_layout(QrCarve &c, int64_t m, int32_t k, int64_t S) {
  RcWs w;
  w.rs = c.take<RowState>((size_t)m, RC_ALIGN);
  w.cand = c.take<uint64_t>((size_t)m * k, RC_ALIGN);
  w.hist = c.take<uint32_t>((size_t)m * S * RC_HSTRIDE, RC_ALIGN);
  w.rowhist = c.take<uint32_t>(S > 1 ? (size_t)m * RC_HSTRIDE : 0, RC_ALIGN);
  w.tq = c.take<int32_t>((size_t)m * S, RC_ALIGN);
  return w;
}

// The selection over m rows, once the arguments are checked: the rows form (S == 0 or nq == 0; no workspace) or the
// slice form over the workspace `w` (rc_layout(m, k, S)).  COMPACT = false: rows users[.] of ratings / pred, stride = nq;
// true: rows 0 .. m - 1 of the compact buffer `pred`.
template <bool COMPACT>
int rc_select(const char *who, const int32_t *ratings, const int32_t *pred, int64_t stride, int64_t nu, int64_t nq,
              const int32_t *users, int64_t m, int32_t k, int32_t lo, int64_t S, int32_t *idx_out, int32_t *val_out,
              int32_t *avail_out, const RcWs &w, hipStream_t st) {
  if (S == 0 || nq == 0) {
    // rows form (also every row of an empty matrix: avail 0, padded, bad ids flagged)
    QR_LAUNCH("recommend_rows", recommend_rows_kernel<COMPACT>, dim3((unsigned)m), dim3(RC_THREADS), 0, st, ratings, pred,
              nu, nq, stride, users, (int)k, idx_out, val_out, avail_out);
    QR_LAUNCH_CHECK(who);
    return QRLSH_OK;
  }
  RowState *rs = w.rs;
  uint64_t *cand = w.cand;
  uint32_t *hist = w.hist, *rowhist = w.rowhist;
  int32_t *tq = w.tq;
  if (S > 1) QR_MEMSET(who, rowhist, 0, (size_t)m * RC_HSTRIDE * sizeof(uint32_t), st);
  const unsigned groups = (unsigned)(m * S);
  const uint32_t lo_key = (uint32_t)lo ^ 0x80000000u;
  for (int pass = 0; pass < 4; ++pass) {
    // pass 0: the window; 1-3: radix rounds, returning at once for every row the window resolved
    QR_LAUNCH(pass ? "recommend_refine_hist" : "recommend_hist", recommend_hist_kernel<COMPACT>, dim3(groups),
              dim3(RC_THREADS), 0, st, ratings, pred, nu, nq, stride, users, (int)S, pass, lo_key, (const RowState *)rs,
              hist, rowhist);
    QR_LAUNCH(pass ? "recommend_refine_threshold" : "recommend_threshold", recommend_threshold_kernel, dim3((unsigned)m),
              dim3(RC_THREADS), 0, st, nu, users, (int)k, (int)S, pass, lo_key, rs, (const uint32_t *)hist, rowhist, tq);
  }
  QR_LAUNCH("recommend_emit", recommend_emit_kernel<COMPACT>, dim3(groups), dim3(RC_THREADS), 0, st, ratings, pred, nq,
            stride, users, (int)k, (int)S, rs, (const int32_t *)tq, cand);
  QR_LAUNCH("recommend_finish", recommend_finish_kernel, dim3((unsigned)m), dim3(RC_THREADS), 0, st, (int)k,
            (const RowState *)rs, (const uint64_t *)cand, idx_out, val_out, avail_out);
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}

// qrlsh_recommend_users' compact rows: a stride of whole 16-byte vectors, so that every row starts on one
int64_t rc_compact_stride(int64_t nq) { return (nq + 3) & ~(int64_t)3; }

// the selection's workspace where there is one: the slice form over a matrix with columns
RcWs rc_select_layout(QrCarve &c, int64_t m, int64_t nq, int32_t k, int64_t S) {
  return S > 0 && m > 0 && nq > 0 ? rc_layout(c, m, k, S) : RcWs{};
}
// workspace: [compact eligible-mode rows: m x round_up(nq, 4) int32][the selection's workspace (slice form)]
struct RuWs {
  int32_t *rows;
  RcWs select;
};
RuWs ru_layout(QrCarve &c, int64_t m, int64_t nq, int32_t k, int64_t S) {
  RuWs w;
  w.rows = c.take<int32_t>((size_t)m * (size_t)rc_compact_stride(nq), RC_ALIGN);
  w.select = rc_select_layout(c, m, nq, k, S);
  return w;
}
}  // namespace

QRLSH_EXPORT size_t qrlsh_recommend_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices) {
  if (m <= 0 || nq <= 0 || k < 1 || k > QRLSH_RECOMMEND_MAX_K || slices < 0 || slices > RC_MAXS) return 0;
  const int64_t S = rc_slices(m, nq, slices);
  if (S == 0 || m > RC_MAX_GROUPS || m * S > RC_MAX_GROUPS) return 0;
  return QR_LAYOUT_BYTES(rc_select_layout, m, nq, k, S);
}

QRLSH_EXPORT int qrlsh_recommend_topk(const int32_t *ratings, const int32_t *pred, int64_t nu, int64_t nq,
                                      const int32_t *users, int64_t m, int32_t k, int32_t lo, int32_t slices,
                                      int32_t *idx_out, int32_t *val_out, int32_t *avail_out, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(k >= 1 && k <= QRLSH_RECOMMEND_MAX_K, "qrlsh_recommend_topk: k=%d outside 1..%d", k,
               QRLSH_RECOMMEND_MAX_K);
  QR_CHECK_ARG(m >= 0 && nu >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_recommend_topk: bad sizes m=%lld nu=%lld nq=%lld",
               (long long)m, (long long)nu, (long long)nq);
  QR_CHECK_ARG(slices >= 0 && slices <= RC_MAXS, "qrlsh_recommend_topk: slices=%d outside 0..%d", slices, RC_MAXS);
  QR_CHECK_ARG(users || m == nu, "qrlsh_recommend_topk: without a user list m (%lld) must equal nu (%lld)",
               (long long)m, (long long)nu);
  QR_CHECK_ARG(m == 0 || (idx_out && val_out && avail_out), "qrlsh_recommend_topk: null output pointer");
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(nq == 0 || nu == 0 || (ratings && pred), "qrlsh_recommend_topk: null matrix pointer");
  QR_CHECK_ALIGNED("qrlsh_recommend_topk", "ratings and pred", qr_addr(ratings) | qr_addr(pred), 16);
  const int64_t S = rc_slices(m, nq, slices);
  if (m > RC_MAX_GROUPS || m * (S > 0 ? S : 1) > RC_MAX_GROUPS) {
    qrlsh_set_error("qrlsh_recommend_topk: m=%lld x slices=%lld above the %lld workgroups served", (long long)m,
                    (long long)S, (long long)RC_MAX_GROUPS);
    return QRLSH_EUNSUPPORTED;
  }
  QR_CHECK_WORKSPACE("qrlsh_recommend_topk", workspace, workspace_bytes,
                     qrlsh_recommend_workspace_bytes(m, nq, k, slices));
  QrCarve c(workspace);
  return rc_select<false>("qrlsh_recommend_topk", ratings, pred, nq, nu, nq, users, m, k, lo, S, idx_out, val_out,
                          avail_out, rc_select_layout(c, m, nq, k, S), static_cast<hipStream_t>(stream));
}

// ---- the selection over compact rows for other files (common.h): qrlsh_evaluate_ranking's sweep in rankeval.hip writes
// the rows, rc_select<true> ranks them -- the path qrlsh_recommend_users takes after qr_predict_users
int64_t qr_select_compact_stride(int64_t nq) { return rc_compact_stride(nq); }

int qr_select_compact_plan(const char *who, int64_t m, int64_t nq, int32_t k, int32_t slices, size_t *rows_bytes,
                           size_t *select_bytes) {
  QR_CHECK_ARG(k >= 1 && k <= QRLSH_RECOMMEND_MAX_K, "%s: k=%d outside 1..%d", who, k, QRLSH_RECOMMEND_MAX_K);
  QR_CHECK_ARG(m >= 0 && nq >= 0 && nq <= 2147483647ll, "%s: bad sizes m=%lld nq=%lld", who, (long long)m, (long long)nq);
  QR_CHECK_ARG(slices >= 0 && slices <= RC_MAXS, "%s: slices=%d outside 0..%d", who, slices, RC_MAXS);
  const int64_t S = rc_slices(m, nq, slices);
  if (m > RC_MAX_GROUPS || m * (S > 0 ? S : 1) > RC_MAX_GROUPS) {
    qrlsh_set_error("%s: m=%lld x slices=%lld above the %lld workgroups served", who, (long long)m, (long long)S,
                    (long long)RC_MAX_GROUPS);
    return QRLSH_EUNSUPPORTED;
  }
  QrCarve all(nullptr), select(nullptr);
  ru_layout(all, m, nq, k, S);
  rc_select_layout(select, m, nq, k, S);
  *rows_bytes = all.bytes() - select.bytes();
  *select_bytes = select.bytes();
  return QRLSH_OK;
}

int qr_select_compact(const char *who, const int32_t *rows, int64_t nu, int64_t nq, const int32_t *users, int64_t m,
                      int32_t k, int32_t lo, int32_t slices, int32_t *idx_out, int32_t *val_out, int32_t *avail_out,
                      void *select_ws, hipStream_t st) {
  const int64_t S = rc_slices(m, nq, slices);
  QrCarve c(select_ws);
  return rc_select<true>(who, nullptr, rows, rc_compact_stride(nq), nu, nq, users, m, k, lo, S, idx_out, val_out,
                         avail_out, rc_select_layout(c, m, nq, k, S), st);
}

QRLSH_EXPORT size_t qrlsh_recommend_users_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices) {
  if (m <= 0 || nq <= 0 || k < 1 || k > QRLSH_RECOMMEND_MAX_K || slices < 0 || slices > RC_MAXS) return 0;
  const int64_t S = rc_slices(m, nq, slices);
  if (m > RC_MAX_GROUPS || m * (S > 0 ? S : 1) > RC_MAX_GROUPS) return 0;
  return QR_LAYOUT_BYTES(ru_layout, m, nq, k, S);
}

QRLSH_EXPORT int qrlsh_recommend_users(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                                       const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx,
                                       const double *u_val, int32_t ku, double query_weight, double user_weight,
                                       double default_mean, int32_t sum_order, const int32_t *users, int64_t m, int32_t k,
                                       int32_t lo, int32_t slices, int32_t *idx_out, int32_t *val_out, int32_t *avail_out,
                                       uint32_t *flags_out, void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(k >= 1 && k <= QRLSH_RECOMMEND_MAX_K, "qrlsh_recommend_users: k=%d outside 1..%d", k,
               QRLSH_RECOMMEND_MAX_K);
  QR_CHECK_ARG(m >= 0 && nu >= 0 && nq >= 0 && nq <= 2147483647ll, "qrlsh_recommend_users: bad sizes m=%lld nu=%lld nq=%lld",
               (long long)m, (long long)nu, (long long)nq);
  QR_CHECK_ARG(slices >= 0 && slices <= RC_MAXS, "qrlsh_recommend_users: slices=%d outside 0..%d", slices, RC_MAXS);
  QR_CHECK_ARG(m == 0 || (idx_out && val_out && avail_out), "qrlsh_recommend_users: null output pointer");
  const int64_t S = rc_slices(m, nq, slices);
  if (m > RC_MAX_GROUPS || m * (S > 0 ? S : 1) > RC_MAX_GROUPS) {
    qrlsh_set_error("qrlsh_recommend_users: m=%lld x slices=%lld above the %lld workgroups served", (long long)m,
                    (long long)S, (long long)RC_MAX_GROUPS);
    return QRLSH_EUNSUPPORTED;
  }
  const size_t need = qrlsh_recommend_users_workspace_bytes(m, nq, k, slices);
  if (m > 0 && need > 0) {
    QR_CHECK_ALIGNED("qrlsh_recommend_users", "the workspace", qr_addr(workspace), 16);
    QR_CHECK_WORKSPACE("qrlsh_recommend_users", workspace, workspace_bytes, need);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  const RuWs w = ru_layout(c, m, nq, k, S);
  const int64_t stride = rc_compact_stride(nq);
  int32_t *rows = w.rows;
  // the remaining checks (sizes, sum_order, pointers) are the sweep's, made before any device work as well; m = 0
  // returns from there
  const int rc = qr_predict_users("qrlsh_recommend_users", ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, ku,
                                  query_weight, user_weight, default_mean, sum_order, users, m, true, rows, stride,
                                  flags_out, st);
  if (rc != QRLSH_OK || m == 0) return rc;
  return rc_select<true>("qrlsh_recommend_users", nullptr, rows, stride, nu, nq, users, m, k, lo, S, idx_out, val_out,
                         avail_out, w.select, st);
}
