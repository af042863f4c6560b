// rankeval.hip -- qrlsh_evaluate_ranking: is what the user would like in the list the user is shown?  The sweep
// (rank_sweep_kernel), the score (rank_score_kernel) and the workspace.  The cell prediction and the row staging are
// evalsides.h's one copy, shared with predict.hip, evaluate.hip and rankgrid.hip (the same call for a whole grid of
// settings); the queue of the held-out cells is ev_cell_queue's protocol written out in the sweep (see there).
// Compiled with -ffp-contract=off as those files are.
//
// Hold-out only.  `train` = the matrix with the test cells zeroed, `truth` = the full one.  A TEST cell of user u:
// train[u][j] == 0 && truth[u][j] != 0; it is RELEVANT when truth[u][j] >= relevant.  The user's list is
// qrlsh_recommend_users' over `train`: a test cell is 0 there, so the serving arithmetic (ev_predict<false>) is its
// hold-out prediction.  Three steps: rank_sweep_kernel writes the compact eligible-mode rows and counts the test cells,
// rc_select<true> (recommend.hip, through qr_select_compact) ranks them, rank_score_kernel holds the lists to the truth.
// Everything counted is an integer: exact, and independent of the launch order.
//
#include "common.h"
#include "evalsides.h"

// The sweep: predict_users_kernel's geometry (predict.hip) and two row forms.  HELDOUT = false: every unrated cell of
// `train` is predicted -- predict_users_kernel<true>'s rows, word for word.  true: only the test cells are candidates;
// they are queued in LDS as evaluate_kernel queues its cells (1024 predicted whenever 1024 wait; written out below), so the
// lanes stay full when 1 % of the row is held out, and every other word of the slice is written 0.  In the same pass
// the workgroup counts its slice's test cells and relevant test cells -- also those the model cannot reach (prediction 0)
// -- into part[request][slice][2] (word 0 test cells, word 1 relevant ones).
constexpr int RK_THREADS = PU_THREADS;

static int64_t rk_sweep_slices(int64_t m, int64_t nq, int32_t slices) {
  int64_t S = slices > 0 ? slices : ceil_div64(PU_AUTO_GROUPS, m > 0 ? m : 1);
  const int64_t most = ceil_div64(nq, RK_THREADS);
  if (S > most) S = most;
  return S;   // 0 when nq == 0
}

template <bool HELDOUT>
__global__ __launch_bounds__(RK_THREADS) void rank_sweep_kernel(
    const int32_t *__restrict__ train, const int32_t *__restrict__ truth, int64_t nu, int64_t nq,
    const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli,
    const int32_t *__restrict__ u_idx, const double *__restrict__ u_val, int ku, double qw, double uw, double dmean,
    int sequential, const int32_t *__restrict__ users, int64_t m, int64_t slices, int32_t relevant,
    int32_t *__restrict__ out, int64_t ostride, long long *__restrict__ part) {
  __shared__ uint8_t lrow[PR_MAXQ];
  __shared__ int32_t queue_j[HELDOUT ? EV_QUEUE_SLOTS<RK_THREADS> : 1];
  __shared__ uint32_t wsum[RK_THREADS / WAVE];
  __shared__ uint32_t cred[RK_THREADS / WAVE][2];
  __shared__ int wide;
  const int64_t s = blockIdx.x / m, x = blockIdx.x - s * m;
  const int t = threadIdx.x;
  const int64_t per = (nq + slices - 1) / slices;
  const int64_t j0 = s * per, j1 = min(nq, j0 + per);
  int32_t *orow = out + x * ostride;
  long long *pout = part + (x * slices + s) * 2;
  const int64_t i = users ? (int64_t)users[x] : x;
  if (i < 0 || i >= nu) {  // uniform; flagged (bit 2) by the check kernel
    for (int64_t j = j0 + t; j < j1; j += RK_THREADS) orow[j] = 0;
    if (t < 2) pout[t] = 0;
    return;
  }
  const int32_t *row = train + i * nq;
  const int32_t *trow = truth + i * nq;
  bool in_lds = false;
  if (nq <= PR_MAXQ) in_lds = ev_stage_row<RK_THREADS>(row, nq, lrow, &wide);  // uniform
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  // The list-length loop (ev_list_len) and, below, the queue (ev_cell_queue) are written out: through both helpers the
  // held-out sweep measured 1 to 1.2 % slower than before with 16 requests, through the queue helper alone up to 1.7 %
  // with 2000.  As written, with the shared ev_predict<false>, both instantiations compile to the instructions they
  // had before the split (profiles/predict_split_parent_vs_branch.json: diagnostic_rank_sweep_heldout).
  int mu = 0;
  while (mu < ku && ui[mu] >= 0) ++mu;  // uniform: the user's own neighbour list
  auto predict = [&](int64_t j) {
    int branch;
    return ev_predict<false>(
        train, nu, nq, i, j, q_off, q_idx, q_milli, ui, uv, mu, qw, uw, dmean, sequential != 0,
        [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; }, branch);
  };
  uint32_t ntest = 0, nrel = 0;
  if (!HELDOUT) {
    for (int64_t j = j0 + t; j < j1; j += RK_THREADS) {
      const int32_t own = in_lds ? (int32_t)lrow[j] : row[j];
      const int32_t tv = trow[j];
      const bool test = own == 0 && tv != 0;
      ntest += test ? 1u : 0u;
      nrel += test && tv >= relevant ? 1u : 0u;
      orow[j] = own != 0 ? 0 : predict(j);
    }
  } else {
    // ev_cell_queue's ring and barriers (evalsides.h), columns only
    constexpr int RK_QUEUE = EV_QUEUE_SLOTS<RK_THREADS>;
    uint32_t head = 0, tail = 0;  // uniform
    for (int64_t base = j0; base < j1; base += RK_THREADS) {
      const int64_t j = base + t;
      bool take = false;
      if (j < j1) {
        const int32_t own = in_lds ? (int32_t)lrow[j] : row[j];
        const int32_t tv = trow[j];
        take = own == 0 && tv != 0;
        ntest += take ? 1u : 0u;
        nrel += take && tv >= relevant ? 1u : 0u;
        if (!take) orow[j] = 0;
      }
      uint32_t total;
      const uint32_t pos = block_excl_scan<RK_THREADS>(take ? 1u : 0u, wsum, total);
      if (take) queue_j[(tail + pos) & (RK_QUEUE - 1)] = (int32_t)j;
      tail += total;
      if (tail - head >= (uint32_t)RK_THREADS) {  // uniform
        __syncthreads();
        const int64_t jq = queue_j[(head + t) & (RK_QUEUE - 1)];
        orow[jq] = predict(jq);
        head += RK_THREADS;
      }
      // the next scan's first barrier stands between these reads of the queue and the writes that follow it
    }
    __syncthreads();
    if ((uint32_t)t < tail - head) {
      const int64_t jq = queue_j[(head + t) & (RK_QUEUE - 1)];
      orow[jq] = predict(jq);
    }
  }
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) {
    ntest += __shfl_xor(ntest, d, WAVE);
    nrel += __shfl_xor(nrel, d, WAVE);
  }
  if ((t & (WAVE - 1)) == 0) {
    cred[t >> 6][0] = ntest;
    cred[t >> 6][1] = nrel;
  }
  __syncthreads();
  if (t < 2) {
    long long sum = 0;
#pragma unroll
    for (int k = 0; k < RK_THREADS / WAVE; ++k) sum += cred[k][t];
    pout[t] = sum;
  }
}

// The score: one wave per request.  Lanes stride over the list positions and gather truth[user][idx[p]]; the wave
// reduces the 8 words of the request's line (include/qrlsh.h) and sums the request's slice counts.  The workgroup's
// RS_WAVES lines are added in LDS and reach totals_out by 64-bit integer atomics: exact in any order.  A request with a
// user id outside [0, nu) gets a zero line with avail -1 and adds nothing to the totals.  Flag bit 3: a negative gain.
constexpr int RS_WAVES = 4;
constexpr int RS_TOTALS = 12;   // words of totals_out that are sums
__global__ __launch_bounds__(RS_WAVES *WAVE) void rank_score_kernel(
    const int32_t *__restrict__ truth, int64_t nu, int64_t nq, const int32_t *__restrict__ users, int64_t m, int k,
    int32_t relevant, const int32_t *__restrict__ idx, const int32_t *__restrict__ avail,
    const long long *__restrict__ gain, const long long *__restrict__ gain_prefix, const long long *__restrict__ part,
    int64_t slices, long long *__restrict__ per_user_out, unsigned long long *__restrict__ totals,
    uint32_t *__restrict__ flags) {
  __shared__ long long tile[RS_WAVES][RS_TOTALS];
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const int64_t x = (int64_t)blockIdx.x * RS_WAVES + w;
  if (blockIdx.x == 0 && w == 0) {
    bool negative = false;
    for (int p = lane; p < k; p += WAVE) negative |= gain[p] < 0;
    if (negative) atomicOr(flags, 8u);
  }
  long long listed = 0, hits = 0, known = 0, first = 0, dcg = 0, rel = 0, test = 0, av = 0, ideal = 0;
  bool served = false;
  if (x < m) {  // wave-uniform
    const int64_t u = users ? (int64_t)users[x] : x;
    served = u >= 0 && u < nu;
    av = served ? (long long)avail[x] : -1;
    if (served) {
      listed = av < k ? av : k;
      int32_t h = 0, kn = 0, fr = 0x7fffffff;
      const int32_t *trow = truth + u * nq;
      const int32_t *lrow = idx + x * k;
      for (int p = lane; p < (int)listed; p += WAVE) {
        const int32_t tv = trow[lrow[p]];   // a listed cell is unrated in train: rated in truth = a test cell
        kn += tv != 0 ? 1 : 0;
        if (tv >= relevant) {
          ++h;
          dcg += gain[p];
          fr = min(fr, p + 1);
        }
      }
      for (int64_t s = lane; s < slices; s += WAVE) {
        test += part[(x * slices + s) * 2];
        rel += part[(x * slices + s) * 2 + 1];
      }
#pragma unroll
      for (int d = WAVE / 2; d >= 1; d >>= 1) {
        h += __shfl_xor(h, d, WAVE);
        kn += __shfl_xor(kn, d, WAVE);
        fr = min(fr, __shfl_xor(fr, d, WAVE));
        dcg += __shfl_xor(dcg, d, WAVE);
        test += __shfl_xor(test, d, WAVE);
        rel += __shfl_xor(rel, d, WAVE);
      }
      hits = h;
      known = kn;
      first = h ? fr : 0;
      ideal = gain_prefix[rel < k ? rel : k];
    }
    const long long line = lane == 0 ? listed : lane == 1 ? hits : lane == 2 ? known : lane == 3 ? first
                           : lane == 4 ? dcg : lane == 5 ? rel : lane == 6 ? test : av;
    if (lane < 8) per_user_out[x * 8 + lane] = line;
  }
  if (lane < RS_TOTALS) {
    const long long add = lane == 0 ? listed : lane == 1 ? hits : lane == 2 ? known : lane == 3 ? first
                          : lane == 4 ? dcg : lane == 5 ? rel : lane == 6 ? test : lane == 7 ? (served ? av : 0)
                          : lane == 8 ? (served ? 1 : 0) : lane == 9 ? (rel > 0 ? 1 : 0)
                          : lane == 10 ? (hits > 0 ? 1 : 0) : ideal;
    tile[w][lane] = add;
  }
  __syncthreads();
  if (t < RS_TOTALS) {
    long long sum = 0;
#pragma unroll
    for (int q = 0; q < RS_WAVES; ++q) sum += tile[q][t];
    if (sum != 0) atomicAdd(totals + t, (unsigned long long)sum);
  }
}

// workspace: [compact rows: m x round_up(nq, 4) int32][the selection's workspace (slice form)][part: m x sweep slices x 2
// int64]
struct RkWs {
  int32_t *rows;
  void *select;
  long long *part;
};
// rows_bytes, select_bytes: qr_select_compact_plan's (multiples of 256)
static RkWs rk_layout(QrCarve &c, int64_t m, int64_t nq, int32_t slices, size_t rows_bytes, size_t select_bytes) {
  RkWs w;
  w.rows = static_cast<int32_t *>(c.take_bytes(rows_bytes, 1));
  w.select = c.take_bytes(select_bytes, 1);
  w.part = c.take<long long>((size_t)m * (size_t)rk_sweep_slices(m, nq, slices) * 2, 256);
  return w;
}
QRLSH_EXPORT size_t qrlsh_evaluate_ranking_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices) {
  if (m <= 0 || nq <= 0) return 0;
  size_t rows = 0, select = 0;
  if (qr_select_compact_plan("qrlsh_evaluate_ranking_workspace_bytes", m, nq, k, slices, &rows, &select) != QRLSH_OK)
    return 0;
  return QR_LAYOUT_BYTES(rk_layout, m, nq, slices, rows, select);
}

QRLSH_EXPORT int qrlsh_evaluate_ranking(const int32_t *train, const int32_t *truth, int64_t nu, int64_t nq,
                                        const int64_t *q_off, const int32_t *q_idx, const int32_t *q_milli,
                                        const int32_t *u_idx, const double *u_val, int32_t ku, double query_weight,
                                        double user_weight, double default_mean, int32_t sum_order,
                                        const int32_t *users, int64_t m, int32_t k, int32_t relevant, int32_t candidates,
                                        int32_t lo, int32_t slices, const int64_t *gain, const int64_t *gain_prefix,
                                        int32_t *idx_out, int32_t *val_out, int32_t *avail_out, int64_t *per_user_out,
                                        int64_t *totals_out, uint32_t *flags_out, void *workspace, size_t workspace_bytes,
                                        void *stream) {
  const char *who = "qrlsh_evaluate_ranking";
  size_t rows_bytes = 0, select_bytes = 0;
  const int rc = qr_select_compact_plan(who, m, nq, k, slices, &rows_bytes, &select_bytes);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(nu >= 0 && ku >= 0 && ku <= PRED_MAXK, "%s: bad sizes nu=%lld ku=%d (<= %d)", who, (long long)nu, ku,
               PRED_MAXK);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL, "%s: bad sum_order %d", who,
               sum_order);
  QR_CHECK_ARG(relevant >= 1, "%s: relevant=%d below 1", who, relevant);
  QR_CHECK_ARG(candidates == QRLSH_RANK_ALL || candidates == QRLSH_RANK_HELDOUT, "%s: bad candidates %d", who, candidates);
  QR_CHECK_ARG(users || m == nu, "%s: without a user list m (%lld) must equal nu (%lld)", who, (long long)m,
               (long long)nu);
  QR_CHECK_ARG(flags_out && totals_out, "%s: flags_out and totals_out are required", who);
  QR_CHECK_ARG(m == 0 || (idx_out && val_out && avail_out && per_user_out), "%s: null output pointer", who);
  QR_CHECK_ARG(m == 0 || (gain && gain_prefix), "%s: gain and gain_prefix are required", who);
  QR_CHECK_ARG(m == 0 || nq == 0 || (q_off && (nu == 0 || (train && truth && (ku == 0 || (u_idx && u_val))))),
               "%s: null pointer", who);
  if (m > (1ll << 24)) {
    qrlsh_set_error("%s: m=%lld above the %lld rows served per call", who, (long long)m, (long long)(1ll << 24));
    return QRLSH_EUNSUPPORTED;
  }
  const int64_t S = rk_sweep_slices(m, nq, slices);
  const size_t need = qrlsh_evaluate_ranking_workspace_bytes(m, nq, k, slices);
  if (m > 0 && need > 0) {
    QR_CHECK_ALIGNED(who, "the workspace", qr_addr(workspace), 16);
    QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, need);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET(who, flags_out, 0, sizeof(uint32_t), st);
  QR_MEMSET(who, totals_out, 0, 16 * sizeof(int64_t), st);
  if (m == 0) return QRLSH_OK;
  QrCarve c(workspace);
  const RkWs w = rk_layout(c, m, nq, slices, rows_bytes, select_bytes);
  int32_t *rows = w.rows;
  long long *part = w.part;
  qr_lists_check("rank_check", q_off, q_idx, nq, users, m, nu, flags_out, st);
  if (nq > 0) {
    const dim3 grid((unsigned)(m * S));
    const int64_t stride = qr_select_compact_stride(nq);
    const int seq = (int)(sum_order == QRLSH_SUM_SEQUENTIAL);
    if (candidates == QRLSH_RANK_HELDOUT)
      QR_LAUNCH("rank_sweep_heldout", rank_sweep_kernel<true>, grid, dim3(RK_THREADS), 0, st, train, truth, nu, nq, q_off,
                q_idx, q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean, seq, users, m, S, relevant,
                rows, stride, part);
    else
      QR_LAUNCH("rank_sweep", rank_sweep_kernel<false>, grid, dim3(RK_THREADS), 0, st, train, truth, nu, nq, q_off, q_idx,
                q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean, seq, users, m, S, relevant, rows,
                stride, part);
  }
  const int rs = qr_select_compact(who, rows, nu, nq, users, m, k, lo, slices, idx_out, val_out, avail_out,
                                   w.select, st);
  if (rs != QRLSH_OK) return rs;
  QR_LAUNCH("rank_score", rank_score_kernel, dim3((unsigned)ceil_div64(m, RS_WAVES)), dim3(RS_WAVES * WAVE), 0, st, truth,
            nu, nq, users, m, (int)k, relevant, (const int32_t *)idx_out, (const int32_t *)avail_out,
            reinterpret_cast<const long long *>(gain), reinterpret_cast<const long long *>(gain_prefix),
            (const long long *)part, S, reinterpret_cast<long long *>(per_user_out),
            reinterpret_cast<unsigned long long *>(totals_out), flags_out);
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}
