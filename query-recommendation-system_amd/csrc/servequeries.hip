// servequeries.hip -- serving chosen queries from the live lists: the completed columns of indexed queries
// (qrlsh_predict_queries), their top-k users (qrlsh_recommend_queries) and their utility words, without the [nu][nq]
// prediction matrix.  The column-shaped counterpart of predict_users_kernel (predict.hip); the arithmetic is
// evalsides.h's one copy (weighted_average, Pairwise8, ev_blend), so the file is compiled with -ffp-contract=off.
//
// "Whom do I show query j?"  For a fixed column j the two gathers of a cell (u, j) change sides against the row sweep:
//   user side   weighted_average(ratings[:, j], user_sims[u]) reads column j only, at u's <= 64 neighbour users.  The
//               column is first gathered out of the row-major matrix into a compact buffer (serve_queries_gather_kernel:
//               nu strided reads, once per call) and then staged by every workgroup in LDS as bytes;
//   query side  weighted_average(ratings[u], query_sims[j]) reads u's own row at j's <= 64 neighbour columns: a
//               scattered global gather, one memory transaction per (user, neighbour of j).  j's list is the same for
//               every user of the column: read once into LDS.
// The user side must see the RAW column, never cells this call has already predicted: that is why the compact column is
// a buffer of its own (cols) and not the output.
//
// One PU_THREADS-thread workgroup per (user slice, request), the requests varying fastest (predict_users_kernel's
// geometry).  Two forms, decided on the device, same results: the compact column staged in LDS as bytes (nu <= PR_MAXQ
// and every value in 0 .. 255: ev_stage_row, unchanged -- its "row" is the compact column), or read from memory.
// ELIGIBLE = false: completed columns (the rating where rated); true: 0 where rated, so that out != 0 is the
// selection's eligibility test, and qr_select_compact (recommend.hip) ranks the columns as it ranks compact rows: row
// length nu, "row ids" = the query ids, checked against nq.
//
// Nothing outside the buffers is read whatever the inputs hold: a list longer than PRED_MAXK is not walked, a neighbour
// index outside [0, nq) is not gathered (both: the unrated cells of the column get 0), the column of a query id outside
// [0, nq) is not read (the output row gets 0, no utility).  qr_lists_check raises the flags for all three.  u_idx entries
// are TRUSTED to lie in [0, nu), exactly as qrlsh_predict_users trusts them.
#include "common.h"
#include "evalsides.h"

namespace {
constexpr int SG_THREADS = 256;
constexpr int64_t SQ_MAX_M = 1ll << 24;   // requests served per call (the grids stay in 32 bits)

// cols[x][u] = ratings[u][queries[x]]: strided reads, coalesced writes; `gs` workgroups per request stride over the users.
// A request outside [0, nq) reads nothing and writes zeros.
__global__ __launch_bounds__(SG_THREADS) void serve_queries_gather_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                          int64_t nq,
                                                                          const int32_t *__restrict__ queries,
                                                                          int64_t gs, int32_t *__restrict__ cols) {
  const int64_t x = blockIdx.x / gs, b = blockIdx.x - x * gs;
  const int64_t j = queries ? (int64_t)queries[x] : x;
  const bool bad = j < 0 || j >= nq;
  int32_t *col = cols + x * nu;
  for (int64_t u = b * SG_THREADS + threadIdx.x; u < nu; u += gs * SG_THREADS) col[u] = bad ? 0 : ratings[u * nq + j];
}

// the sum of v over the wave, in every lane
__device__ __forceinline__ unsigned long long sq_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

template <bool ELIGIBLE>
__global__ __launch_bounds__(PU_THREADS) void serve_queries_kernel(
    const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, const int64_t *__restrict__ q_off,
    const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli, const int32_t *__restrict__ u_idx,
    const double *__restrict__ u_val, int ku, double qw, double uw, double dmean, int sequential,
    const int32_t *__restrict__ queries, int64_t m, int64_t slices, const int32_t *__restrict__ cols,
    int32_t *__restrict__ out, int64_t ostride, unsigned long long *__restrict__ util) {
  __shared__ uint8_t lcol[PR_MAXQ];
  __shared__ int wide;
  __shared__ int32_t lidx[PRED_MAXK];
  __shared__ double lval[PRED_MAXK];
  __shared__ int skip_s;
  __shared__ unsigned long long words_s[8];
  const int64_t s = blockIdx.x / m, x = blockIdx.x - s * m;
  const int t = threadIdx.x;
  const int64_t per = (nu + slices - 1) / slices;
  const int64_t u0 = s * per, u1 = min(nu, u0 + per);
  int32_t *ocol = out ? out + x * ostride : nullptr;
  const int64_t j = queries ? (int64_t)queries[x] : x;
  if (j < 0 || j >= nq) {  // uniform; flagged (bit 2) by the check kernel
    if (ocol)
      for (int64_t u = u0 + t; u < u1; u += PU_THREADS) ocol[u] = 0;
    return;
  }
  // j's list, once: too long (bit 0) is not walked, an index outside the matrix (bit 1) is not gathered
  const int64_t lo = q_off[j], n64 = q_off[j + 1] - lo;
  const bool fits = n64 >= 0 && n64 <= PRED_MAXK;
  if (t == 0) skip_s = fits ? 0 : 1;
  if (t < 8) words_s[t] = 0;
  __syncthreads();
  if (fits && t < n64) {
    const int32_t ix = q_idx[lo + t];
    if ((uint32_t)ix >= (uint32_t)nq) skip_s = 1;
    lidx[t] = ix;
    lval[t] = (double)q_milli[lo + t] / 1000.0;
  }
  __syncthreads();
  const bool skip = skip_s != 0;  // uniform
  const int n = fits ? (int)n64 : 0;
  const int32_t *col = cols + x * nu;
  bool in_lds = false;
  if (nu <= PR_MAXQ) in_lds = ev_stage_row<PU_THREADS>(col, nu, lcol, &wide);  // uniform
  const int lane = lane_id();
  // The utility words.  The rated users are counted in a sweep of their own over the column, and the count of the
  // predictions and the three branch counts go to LDS wave by wave (ballots), so that the hot loop carries one sum:
  // with eight accumulators per thread the kernel did not fit its 128 registers.
  if (util) {  // uniform
    uint32_t c0 = 0;
    unsigned long long w1 = 0;
    for (int64_t u = u0 + t; u < u1; u += PU_THREADS) {
      const int32_t own = in_lds ? (int32_t)lcol[u] : col[u];
      if (own != 0) {
        c0 += 1;
        w1 += (unsigned long long)(long long)own;
      }
    }
    const unsigned long long r0 = sq_wave_sum(c0), r1 = sq_wave_sum(w1);
    if (lane == 0 && r0) {
      atomicAdd(&words_s[0], r0);
      atomicAdd(&words_s[1], r1);
    }
  }
  unsigned long long w3 = 0;
  // nu < 2^31: a user id, and the id PU_THREADS past the last, fit 32 bits
  for (uint32_t u = (uint32_t)u0 + (uint32_t)t; u < (uint32_t)u1; u += PU_THREADS) {
    const int32_t own = in_lds ? (int32_t)lcol[u] : col[u];
    if (own != 0) {
      if (ocol) ocol[u] = ELIGIBLE ? 0 : own;
      continue;
    }
    int32_t p = 0;
    if (!skip) {
      const int32_t *row = ratings + (int64_t)u * nq;
      const double qp = weighted_average(
          n, sequential != 0, [&](int k) { return row[lidx[k]]; }, [&](int k) { return lval[k]; });
      const int32_t *ui = u_idx + (int64_t)u * ku;
      const double *uv = u_val + (int64_t)u * ku;
      const int mu = ev_list_len(ui, ku);
      const double up = weighted_average(
          mu, sequential != 0, [&](int k) { return in_lds ? (int32_t)lcol[ui[k]] : col[ui[k]]; },
          [&](int k) { return uv[k]; });
      int branch;
      p = (int32_t)rint(ev_blend(qp, up, qw, uw, dmean, branch));
      if (util) {
        // the lanes here are the wave's unrated users of this round; the first of them adds for all
        const unsigned long long here = __ballot(1), b2 = __ballot(p != 0), b5 = __ballot(branch == 0 && qp != 0.0),
                                 b6 = __ballot(branch == 1), b7 = __ballot(branch == 2);
        if (lane == __ffsll((long long)here) - 1) {
          if (b2) atomicAdd(&words_s[2], (unsigned long long)__popcll(b2));
          if (b5) atomicAdd(&words_s[5], (unsigned long long)__popcll(b5));
          if (b6) atomicAdd(&words_s[6], (unsigned long long)__popcll(b6));
          if (b7) atomicAdd(&words_s[7], (unsigned long long)__popcll(b7));
        }
      }
    }
    if (ocol) ocol[u] = p;
    w3 += (unsigned long long)(long long)p;
  }
  if (util == nullptr) return;  // uniform
  // exact int64 words: per wave by shuffles, per workgroup in LDS, then one 64-bit vector atomic per non-zero word
  const unsigned long long r3 = sq_wave_sum(w3);
  if (lane == 0 && r3) atomicAdd(&words_s[3], r3);
  __syncthreads();
  if (t < 8) {
    // the missed users are the rest of the slice
    const unsigned long long span = u1 > u0 ? (unsigned long long)(u1 - u0) : 0ull;
    const unsigned long long v = t == 4 ? span - words_s[0] - words_s[2] : words_s[t];
    if (v) atomicAdd(&util[x * 8 + t], v);
  }
}

// every check of the arguments both entry points share (no device work)
int sq_check(const char *who, const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
             const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku, int32_t sum_order,
             const int32_t *queries, int64_t m, const int32_t *cols_tmp, const uint32_t *flags_out) {
  QR_CHECK_ARG(nu >= 0 && nu <= 2147483647ll && nq >= 0 && nq <= 2147483647ll && m >= 0 && ku >= 0 && ku <= PRED_MAXK,
               "%s: bad sizes nu=%lld nq=%lld m=%lld ku=%d (<= %d)", who, (long long)nu, (long long)nq, (long long)m, ku,
               PRED_MAXK);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL, "%s: bad sum_order %d", who,
               sum_order);
  QR_CHECK_ARG(queries || m == nq, "%s: without a query list m (%lld) must equal nq (%lld)", who, (long long)m,
               (long long)nq);
  QR_CHECK_ARG(flags_out, "%s: flags_out is required", who);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(nu == 0 || cols_tmp, "%s: cols_tmp is required", who);
  QR_CHECK_ARG(nq == 0 || nu == 0 || (ratings && q_off && q_idx && q_milli && (ku == 0 || (u_idx && u_val))),
               "%s: null pointer", who);
  if (m > SQ_MAX_M) {
    qrlsh_set_error("%s: m=%lld above the %lld requests served per call", who, (long long)m, (long long)SQ_MAX_M);
    return QRLSH_EUNSUPPORTED;
  }
  return QRLSH_OK;
}

// The flags, the gather and the sweep, once every argument is checked (m > 0).  `out` columns are `ostride` words apart;
// out == NULL: only the utility words are made.
int sq_sweep(const char *who, const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
             const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku, double query_weight,
             double user_weight, double default_mean, int32_t sum_order, const int32_t *queries, int64_t m, bool eligible,
             int32_t *out, int64_t ostride, int32_t *cols_tmp, int64_t *util_out, uint32_t *flags_out, hipStream_t st) {
  QR_MEMSET(who, flags_out, 0, sizeof(uint32_t), st);
  qr_lists_check("serve_queries_check", q_off, q_idx, nq, queries, m, nq, flags_out, st);
  if (nu > 0) {
    int64_t gs = ceil_div64(nu, SG_THREADS);
    const int64_t room = SQ_MAX_M / m;   // >= 1
    if (gs > room) gs = room;
    QR_LAUNCH("serve_queries_gather", serve_queries_gather_kernel, dim3((unsigned)(m * gs)), dim3(SG_THREADS), 0, st,
              ratings, nu, nq, queries, gs, cols_tmp);
    int64_t slices = ceil_div64(PU_AUTO_GROUPS, m);
    const int64_t most = ceil_div64(nu, PU_THREADS);
    if (slices > most) slices = most;   // m x slices <= 2^24 + 2^12 workgroups
    const dim3 grid((unsigned)(m * slices));
    const int seq = (int)(sum_order == QRLSH_SUM_SEQUENTIAL);
    unsigned long long *util = reinterpret_cast<unsigned long long *>(util_out);
    if (eligible)
      QR_LAUNCH("serve_queries", serve_queries_kernel<true>, grid, dim3(PU_THREADS), 0, st, ratings, nu, nq, q_off, q_idx,
                q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean, seq, queries, m, slices,
                (const int32_t *)cols_tmp, out, ostride, util);
    else
      QR_LAUNCH("serve_queries", serve_queries_kernel<false>, grid, dim3(PU_THREADS), 0, st, ratings, nu, nq, q_off,
                q_idx, q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean, seq, queries, m, slices,
                (const int32_t *)cols_tmp, out, ostride, util);
  }
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}
}  // namespace

QRLSH_EXPORT int qrlsh_predict_queries(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                                       const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx,
                                       const double *u_val, int32_t ku, double query_weight, double user_weight,
                                       double default_mean, int32_t sum_order, const int32_t *queries, int64_t m,
                                       int32_t *out, int32_t *cols_tmp, int64_t *util_out, uint32_t *flags_out,
                                       void *stream) {
  const char *who = "qrlsh_predict_queries";
  const int rc = sq_check(who, ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, ku, sum_order, queries, m, cols_tmp,
                          flags_out);
  if (rc != QRLSH_OK || m == 0) return rc;
  return sq_sweep(who, ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, ku, query_weight, user_weight, default_mean,
                  sum_order, queries, m, false, out, nu, cols_tmp, util_out, flags_out, static_cast<hipStream_t>(stream));
}

QRLSH_EXPORT int qrlsh_recommend_queries(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                                         const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx,
                                         const double *u_val, int32_t ku, double query_weight, double user_weight,
                                         double default_mean, int32_t sum_order, const int32_t *queries, int64_t m,
                                         int32_t k, int32_t lo, int32_t slices, int32_t *idx_out, int32_t *val_out,
                                         int32_t *avail_out, int64_t *util_out, uint32_t *flags_out, int32_t *cols_tmp,
                                         void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "qrlsh_recommend_queries";
  // the selection's own checks (k, m, the row length nu, slices, m x slices workgroups) and its two regions: the layout
  // of qrlsh_recommend_users_workspace_bytes(m, nu, k, slices), compact rows of length nu first
  size_t rows_bytes = 0, select_bytes = 0;
  QR_CHECK_ARG(nu >= 0, "%s: bad sizes nu=%lld", who, (long long)nu);
  int rc = qr_select_compact_plan(who, m, nu, k, slices, &rows_bytes, &select_bytes);
  if (rc != QRLSH_OK) return rc;
  rc = sq_check(who, ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, ku, sum_order, queries, m, cols_tmp, flags_out);
  if (rc != QRLSH_OK || m == 0) return rc;
  QR_CHECK_ARG(idx_out && val_out && avail_out, "%s: null output pointer", who);
  if (nu > 0) {
    QR_CHECK_ALIGNED(who, "the workspace", qr_addr(workspace), 16);
    QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, rows_bytes + select_bytes);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  int32_t *rows = static_cast<int32_t *>(c.take_bytes(rows_bytes, 1));
  void *select_ws = c.take_bytes(select_bytes, 1);
  rc = sq_sweep(who, ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, ku, query_weight, user_weight, default_mean,
                sum_order, queries, m, true, rows, qr_select_compact_stride(nu), cols_tmp, util_out, flags_out, st);
  if (rc != QRLSH_OK) return rc;
  // the roles swapped: rows of length nu, the "row ids" are the query ids, checked against nq
  return qr_select_compact(who, rows, nq, nu, queries, m, k, lo, slices, idx_out, val_out, avail_out, select_ws, st);
}
