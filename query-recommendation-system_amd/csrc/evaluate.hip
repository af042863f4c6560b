// evaluate.hip -- the prediction error on rated cells: qrlsh_ratings_holdout, qrlsh_evaluate, qrlsh_evaluate_grid and
// qrlsh_evaluate_cells, with their finish and totals kernels.  The prediction itself (the sides, the blend, the cell
// prediction), the row staging and the queue of a sweep's cells are evalsides.h's one copy, shared with predict.hip,
// rankeval.hip and rankgrid.hip (evaluate_grid_kernel alone stages its row with a loop of its own: see there); the
// lists' flags come from qr_lists_check (predict.hip).  Compiled with -ffp-contract=off as those files are.
//
// The blend of cell (i, j) reads the user's ratings of j's neighbour queries and the neighbour users' ratings of j, never
// ratings[i][j] itself.  So a RATED cell can be predicted as if it were unrated -- predict_users_kernel's computation over
// the complement of the cells it fills -- and compared with its rating.  Predictions and ratings are integers: every
// statistic is an exact integer sum and the result cannot depend on the launch order.
#include "common.h"
#include "evalsides.h"

// Sample rule (one rule, everywhere): cell (i, j) is KEPT iff the top 32 bits of mix64(seed ^ (i << 32 | j)) lie below
// `keep` (a 64-bit word in [0, 2^32]: 2^32 keeps every cell, 0 none).  It does not depend on nq.
__device__ static inline bool ev_kept(uint64_t seed, uint64_t keep, int64_t i, int64_t j) {
  return (qr_mix64(seed ^ ((uint64_t)i << 32 | (uint64_t)(uint32_t)j)) >> 32) < keep;
}

// The 14 integers of one line of per_user_out, in registers (no indexed array: selects).  Words 0-3, 4-7, 8-11 = n,
// sum err, sum |err|, sum err^2 of the cells predicted from the query side only, the user side only and both; word 12 =
// cells whose prediction is 0 (missed: in no sum); word 13 = cells.
constexpr int EV_WORDS = 14;
struct EvalStats {
  long long qn, qe, qa, qs, un, ue, ua, us, bn, be, ba, bs, missed, cells;
  __device__ void clear() { qn = qe = qa = qs = un = ue = ua = us = bn = be = ba = bs = missed = cells = 0; }
  // branch: 0 query side only, 1 user side only, 2 both (of a non-zero prediction)
  __device__ void add(int32_t pred, int branch, int32_t truth) {
    const long long e = (long long)pred - (long long)truth, a = e < 0 ? -e : e, s = e * e;
    const bool hit = pred != 0, q = hit && branch == 0, u = hit && branch == 1, b = hit && branch == 2;
    qn += q ? 1 : 0; qe += q ? e : 0; qa += q ? a : 0; qs += q ? s : 0;
    un += u ? 1 : 0; ue += u ? e : 0; ua += u ? a : 0; us += u ? s : 0;
    bn += b ? 1 : 0; be += b ? e : 0; ba += b ? a : 0; bs += b ? s : 0;
    missed += hit ? 0 : 1;
    cells += 1;
  }
  template <typename F> __device__ void each(F f) {
    f(qn, 0); f(qe, 1); f(qa, 2); f(qs, 3); f(un, 4); f(ue, 5); f(ua, 6); f(us, 7);
    f(bn, 8); f(be, 9); f(ba, 10); f(bs, 11); f(missed, 12); f(cells, 13);
  }
};

// sum over the workgroup (THREADS threads, all of them call it); red: LDS [THREADS / WAVE][EV_WORDS].  Afterwards thread
// w < EV_WORDS returns word w of the workgroup's sum (other threads: 0).
template <int THREADS> __device__ static inline long long ev_block_sum(EvalStats &s, long long (*red)[EV_WORDS]) {
  s.each([](long long &v, int) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
  });
  const int t = threadIdx.x, w = t >> 6;
  if ((t & (WAVE - 1)) == 0) s.each([&](long long &v, int word) { red[w][word] = v; });
  __syncthreads();
  long long sum = 0;
  if (t < EV_WORDS) {
#pragma unroll
    for (int k = 0; k < THREADS / WAVE; ++k) sum += red[k][t];
  }
  return sum;
}

// The sweep: one workgroup per (column slice, user), the users of a slice together, the user's row of `ratings` staged in
// LDS as bytes where it fits (predict_users_kernel's two forms).  The workgroup reads its slice of `truth` coalesced,
// 1024 columns at a time, and queues the evaluated cells (truth != 0 and kept) in LDS (ev_cell_queue); whenever 1024 are
// queued every thread predicts one (ev_predict<true>: the cell as if its own rating were 0), so the lanes stay full
// however thin the sample is.  Each thread keeps its 14 sums in registers; the workgroup's sums go to
// part[user][slice][16] (summed by evaluate_finish_kernel: no atomics, no order).
constexpr int EV_THREADS = 1024;
constexpr int EV_AUTO_GROUPS = 4096;

static int64_t ev_slices(int64_t nu, int64_t nq) {
  int64_t slices = ceil_div64(EV_AUTO_GROUPS, nu > 0 ? nu : 1);
  const int64_t most = ceil_div64(nq, EV_THREADS);
  if (slices > most) slices = most;
  return slices < 1 ? 1 : slices;
}

__global__ __launch_bounds__(EV_THREADS) void evaluate_kernel(
    const int32_t *__restrict__ ratings, const int32_t *__restrict__ truth, int64_t nu, int64_t nq,
    const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli,
    const int32_t *__restrict__ u_idx, const double *__restrict__ u_val, int ku, double qw, double uw, double dmean,
    int sequential, uint64_t seed, uint64_t keep, int64_t slices, long long *__restrict__ part,
    int32_t *__restrict__ pred_out) {
  __shared__ uint8_t lrow[PR_MAXQ];
  __shared__ int32_t queue_j[EV_QUEUE_SLOTS<EV_THREADS>];
  __shared__ int32_t queue_v[EV_QUEUE_SLOTS<EV_THREADS>];
  __shared__ long long red[EV_THREADS / WAVE][EV_WORDS];
  __shared__ uint32_t wsum[EV_THREADS / WAVE];
  __shared__ int wide;
  const int64_t s = blockIdx.x / nu, i = blockIdx.x - s * nu;
  const int t = threadIdx.x;
  const int64_t per = (nq + slices - 1) / slices;
  const int64_t j0 = s * per, j1 = min(nq, j0 + per);
  const int32_t *row = ratings + i * nq;
  const int32_t *trow = truth + i * nq;
  bool in_lds = false;
  if (nq <= PR_MAXQ) in_lds = ev_stage_row<EV_THREADS>(row, nq, lrow, &wide);  // uniform
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  const int mu = ev_list_len(ui, ku);  // uniform: the user's own neighbour list
  EvalStats st;
  st.clear();
  ev_cell_queue<EV_THREADS>(
      j0, j1, queue_j, queue_v, wsum,
      [&](int64_t j, bool in_range, int32_t &tv) {
        if (in_range) tv = trow[j];
        const bool take = tv != 0 && ev_kept(seed, keep, i, j);
        if (pred_out && in_range && !take) pred_out[i * nq + j] = -1;
        return take;
      },
      [&](uint32_t, int32_t j, int32_t tv, bool active) {
        if (!active) return;
        int branch;
        const int32_t pred = ev_predict<true>(
            ratings, nu, nq, i, j, q_off, q_idx, q_milli, ui, uv, mu, qw, uw, dmean, sequential != 0,
            [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; }, branch);
        st.add(pred, branch, tv);
        if (pred_out) pred_out[i * nq + j] = pred;
      });
  const long long sum = ev_block_sum<EV_THREADS>(st, red);
  if (t < 16) part[(i * slices + s) * 16 + t] = t < EV_WORDS ? sum : 0;
}

// per_user_out[u][w] = the sum over the slices of part[u][.][w]; one workgroup per 64 users (thread = (user, word)), whose
// column sums go to gpart[workgroup][16]
constexpr int EVF_USERS = 64;
__global__ __launch_bounds__(EVF_USERS * 16) void evaluate_finish_kernel(const long long *__restrict__ part, int64_t nu,
                                                                         int64_t slices,
                                                                         long long *__restrict__ per_user_out,
                                                                         long long *__restrict__ gpart) {
  __shared__ long long tile[EVF_USERS][16];
  const int t = threadIdx.x, ul = t >> 4, w = t & 15;
  const int64_t u = (int64_t)blockIdx.x * EVF_USERS + ul;
  long long sum = 0;
  if (u < nu) {
    for (int64_t s = 0; s < slices; ++s) sum += part[(u * slices + s) * 16 + w];
    per_user_out[u * 16 + w] = sum;
  }
  tile[ul][w] = sum;
  __syncthreads();
  if (t < 16) {
    long long col = 0;
#pragma unroll 8
    for (int k = 0; k < EVF_USERS; ++k) col += tile[k][t];
    gpart[(int64_t)blockIdx.x * 16 + t] = col;
  }
}

// totals_out[w] = the sum of gpart[.][w] (one workgroup)
__global__ __launch_bounds__(1024) void evaluate_totals_kernel(const long long *__restrict__ gpart, int64_t groups,
                                                               long long *__restrict__ totals_out) {
  __shared__ long long tile[64][16];
  const int t = threadIdx.x, r = t >> 4, w = t & 15;
  long long sum = 0;
  for (int64_t g = r; g < groups; g += 64) sum += gpart[g * 16 + w];
  tile[r][w] = sum;
  __syncthreads();
  if (t < 16) {
    long long col = 0;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) col += tile[k][t];
    totals_out[t] = col;
  }
}

// workspace: [part: nu x slices x 16 int64][gpart: ceil(nu / 64) x 16 int64]
struct EvWs {
  long long *part, *gpart;
};
// `words` sums per (user, slice) and per group of `group_users` users
static EvWs ev_layout(QrCarve &c, int64_t nu, int64_t nq, size_t words, int group_users) {
  EvWs w;
  w.part = c.take<long long>((size_t)nu * (size_t)ev_slices(nu, nq) * words, 8);
  w.gpart = c.take<long long>((size_t)ceil_div64(nu, group_users) * words, 8);
  return w;
}
QRLSH_EXPORT size_t qrlsh_evaluate_workspace_bytes(int64_t nu, int64_t nq) {
  if (nu <= 0 || nq <= 0) return 0;
  return QR_LAYOUT_BYTES(ev_layout, nu, nq, 16, EVF_USERS);
}

static int ev_check_lists(const char *who, int64_t nu, int64_t nq, int32_t ku, int32_t sum_order, uint64_t keep) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && nu <= 2147483647ll && nq <= 2147483647ll && ku >= 0 && ku <= PRED_MAXK,
               "%s: bad sizes nu=%lld nq=%lld ku=%d (<= %d)", who, (long long)nu, (long long)nq, ku, PRED_MAXK);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL, "%s: bad sum_order %d", who,
               sum_order);
  QR_CHECK_ARG(keep <= (1ull << 32), "%s: keep=%llu above 2^32", who, (unsigned long long)keep);
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_evaluate(const int32_t *ratings, const int32_t *truth, int64_t nu, int64_t nq, const int64_t *q_off,
                                const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx, const double *u_val,
                                int32_t ku, double query_weight, double user_weight, double default_mean,
                                int32_t sum_order, uint64_t seed, uint64_t keep, int64_t *per_user_out, int64_t *totals_out,
                                int32_t *pred_out, uint32_t *flags_out, void *workspace, size_t workspace_bytes,
                                void *stream) {
  const int rc = ev_check_lists("qrlsh_evaluate", nu, nq, ku, sum_order, keep);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(flags_out && totals_out, "qrlsh_evaluate: flags_out and totals_out are required");
  const bool empty = nu == 0 || nq == 0;
  QR_CHECK_ARG(empty || (ratings && truth && q_off && per_user_out && (ku == 0 || (u_idx && u_val))),
               "qrlsh_evaluate: null pointer");
  const size_t need = qrlsh_evaluate_workspace_bytes(nu, nq);
  QR_CHECK_ARG(empty || (workspace && workspace_bytes >= need && (uintptr_t)workspace % 8 == 0),
               "qrlsh_evaluate: needs %zu workspace bytes (8-byte aligned), got %zu", need, workspace_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_evaluate", flags_out, 0, sizeof(uint32_t), st);
  if (empty) QR_MEMSET("qrlsh_evaluate", totals_out, 0, 16 * sizeof(int64_t), st);
  if (empty && nu > 0) QR_MEMSET("qrlsh_evaluate", per_user_out, 0, (size_t)nu * 16 * sizeof(int64_t), st);
  if (empty) return QRLSH_OK;
  const int64_t slices = ev_slices(nu, nq), groups = ceil_div64(nu, EVF_USERS);
  if (nu * slices > 2147483647ll) {
    qrlsh_set_error("qrlsh_evaluate: nu=%lld x %lld slices above 2^31 - 1 workgroups", (long long)nu, (long long)slices);
    return QRLSH_EUNSUPPORTED;
  }
  QrCarve c(workspace);
  const EvWs w = ev_layout(c, nu, nq, 16, EVF_USERS);
  long long *part = w.part, *gpart = w.gpart;
  qr_lists_check("evaluate_check", q_off, q_idx, nq, nullptr, 0, nu, flags_out, st);   // the lists' two flags
  QR_LAUNCH("evaluate", evaluate_kernel, dim3((unsigned)(nu * slices)), dim3(EV_THREADS), 0, st, ratings, truth, nu, nq,
            q_off, q_idx, q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean,
            (int)(sum_order == QRLSH_SUM_SEQUENTIAL), seed, keep, slices, part, pred_out);
  QR_LAUNCH("evaluate_finish", evaluate_finish_kernel, dim3((unsigned)groups), dim3(EVF_USERS * 16), 0, st,
            (const long long *)part, nu, slices, reinterpret_cast<long long *>(per_user_out), gpart);
  QR_LAUNCH("evaluate_totals", evaluate_totals_kernel, dim3(1), dim3(1024), 0, st, (const long long *)gpart, groups,
            reinterpret_cast<long long *>(totals_out));
  QR_LAUNCH_CHECK("qrlsh_evaluate");
  return QRLSH_OK;
}

// ---- the grid: qrlsh_evaluate's cells under S = ncq x ncu x nw settings in one sweep (qrlsh_evaluate_grid) ----
// qp and up of a cell do not depend on the weights, and a stored list is ordered (score descending, id ascending), so its
// first c entries are the list a run with K = c would have stored.  evaluate_kernel's sweep therefore serves a whole
// grid: per cell one query side per query cut and one user side per user cut (the pairwise order depends on the length,
// so each cut has its own accumulation -- at most 4 + 4, never one per setting), then a uniform loop over the settings
// that blends, rounds, wave-reduces the error sums and adds them to an LDS table [S][8] of int64.  The table of a
// workgroup goes to part[user][slice][S][8]; evaluate_grid_finish_kernel / evaluate_grid_totals_kernel add the slices and
// the users (no global atomics, no order).
// Table words while the sweep runs: 0-3 = n, sum err, sum |err|, sum err^2 over the non-zero predictions, 6 / 7 = n of
// the query-only / user-only branch; words 4 (missed = cells - n) and 5 (cells, the same for every setting) are filled
// in when the table is written out.
constexpr int EG_WORDS = 8;
constexpr int EGF_USERS = 16;   // users per workgroup of the finish kernel

__device__ static inline long long eg_wave_sum(long long v) {
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

__global__ __launch_bounds__(64) void evaluate_grid_cuts_kernel(const int32_t *__restrict__ q_cuts, int ncq,
                                                                const int32_t *__restrict__ u_cuts, int ncu,
                                                                uint32_t *__restrict__ flags) {
  eg_check_cuts(threadIdx.x, q_cuts, ncq, u_cuts, ncu, flags);
}

__global__ __launch_bounds__(EV_THREADS) void evaluate_grid_kernel(
    const int32_t *__restrict__ ratings, const int32_t *__restrict__ truth, int64_t nu, int64_t nq,
    const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli,
    const int32_t *__restrict__ u_idx, const double *__restrict__ u_val, int ku, const int32_t *__restrict__ q_cuts,
    int ncq, const int32_t *__restrict__ u_cuts, int ncu, const double *__restrict__ weights, int nw, int sequential,
    uint64_t seed, uint64_t keep, int64_t slices, long long *__restrict__ part, uint32_t *__restrict__ flags) {
  __shared__ uint8_t lrow[PR_MAXQ];
  __shared__ int32_t queue_j[EV_QUEUE_SLOTS<EV_THREADS>];
  __shared__ int32_t queue_v[EV_QUEUE_SLOTS<EV_THREADS>];
  __shared__ unsigned long long table[QRLSH_GRID_MAX_SETTINGS * EG_WORDS];
  __shared__ unsigned long long cells_all;
  __shared__ uint32_t wsum[EV_THREADS / WAVE];
  __shared__ int wide;
  const int64_t s = blockIdx.x / nu, i = blockIdx.x - s * nu;
  const int t = threadIdx.x;
  const int words = ncq * ncu * nw * EG_WORDS;   // <= 1024
  const int64_t per = (nq + slices - 1) / slices;
  const int64_t j0 = s * per, j1 = min(nq, j0 + per);
  const int32_t *row = ratings + i * nq;
  const int32_t *trow = truth + i * nq;
  if (blockIdx.x == 0) eg_check_cuts(t, q_cuts, ncq, u_cuts, ncu, flags);
  if (t < words) table[t] = 0;
  if (t == 0) {
    cells_all = 0;
    wide = 0;
  }
  __syncthreads();
  // ev_stage_row's loop, written out: `wide` is cleared with the table, one barrier fewer -- and through the helper this
  // kernel measured 1.5 % slower on thin samples with 128 settings (profiles/predict_split_parent_vs_branch.json)
  bool in_lds = false;
  if (nq <= PR_MAXQ) {  // uniform
    bool bad = false;
    for (int64_t j = t; j < nq; j += EV_THREADS) {
      const int32_t v = row[j];
      bad |= (v < 0) | (v > 255);
      lrow[j] = (uint8_t)v;
    }
    if (bad) wide = 1;
    __syncthreads();
    in_lds = wide == 0;
  }
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  const int mu = ev_list_len(ui, ku);  // uniform: the user's own neighbour list
  // the cuts (uniform; a negative one is flagged and reads as 0) and the user list's length under each
  int qc[QRLSH_GRID_MAX_CUTS], um[QRLSH_GRID_MAX_CUTS];
#pragma unroll
  for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
    qc[c] = c < ncq ? max(q_cuts[c], 0) : 0;
    um[c] = c < ncu ? min(mu, max(u_cuts[c], 0)) : 0;
  }
  const bool seq = sequential != 0;
  unsigned long long cells = 0;  // of this wave (uniform)
  // one cell per active lane: its sides under every cut, then every setting; all lanes of a wave arrive together
  auto one = [&](uint32_t, int64_t j, int32_t tv, bool active) {   // tv = 0 on the lanes without a cell
    const unsigned long long act = __ballot(active);
    if (act == 0) return;  // wave-uniform
    cells += (unsigned long long)__popcll(act);
    double qp[QRLSH_GRID_MAX_CUTS] = {0.0, 0.0, 0.0, 0.0}, up[QRLSH_GRID_MAX_CUTS] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
      const int64_t lo = q_off[j], n64 = q_off[j + 1] - lo;
      if (n64 >= 0 && n64 <= PRED_MAXK) {  // else flagged (bit 0), never walked: every setting misses the cell
        bool outside = false;
        int last = -1;
#pragma unroll
        for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
          if (c < ncq) {
            const int n = min((int)n64, qc[c]);
            if (c > 0 && n == last) qp[c] = qp[c - 1];  // the list is no longer than either cut: the same prefix
            else
              qp[c] = ev_query_side<true>(
                  nq, j, lo, n, q_idx, q_milli, seq, [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; },
                  outside);
            last = n;
          }
        }
#pragma unroll
        for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
          if (c < ncu) {
            if (c > 0 && um[c] == um[c - 1]) up[c] = up[c - 1];  // uniform
            else up[c] = ev_user_side<true>(ratings, nu, nq, i, j, ui, uv, um[c], seq);
          }
        }
        if (outside) {  // flagged (bit 1): every setting misses the cell
#pragma unroll
          for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) qp[c] = up[c] = 0.0;
        }
      }
    }
    const int lane = t & (WAVE - 1);
    int sidx = 0;
    for (int cq = 0; cq < ncq; ++cq) {
      const double qpc = eg_pick(qp, cq);
      for (int cu = 0; cu < ncu; ++cu) {
        const double upc = eg_pick(up, cu);
        for (int w = 0; w < nw; ++w, ++sidx) {
          int branch;
          const double r = ev_blend(qpc, upc, weights[3 * w], weights[3 * w + 1], weights[3 * w + 2], branch);
          const int32_t pred = (int32_t)rint(r);   // 0 on the lanes without a cell: both sides are 0 there
          const bool hit = pred != 0;
          const unsigned long long hits = __ballot(hit);
          if (hits == 0) continue;  // wave-uniform: nothing to add
          const long long e = hit ? (long long)pred - (long long)tv : 0;
          const long long se = eg_wave_sum(e), sa = eg_wave_sum(e < 0 ? -e : e), ss = eg_wave_sum(e * e);
          const long long qn = __popcll(__ballot(hit && branch == 0)), un = __popcll(__ballot(hit && branch == 1));
          // lanes 0 .. 5 add one word each: a single LDS atomic instruction per setting and wave
          const long long v = lane == 0 ? (long long)__popcll(hits)
                                        : (lane == 1 ? se : (lane == 2 ? sa : (lane == 3 ? ss : (lane == 4 ? qn : un))));
          if (lane < 6 && v != 0)
            atomicAdd(&table[sidx * EG_WORDS + (lane < 4 ? lane : lane + 2)], (unsigned long long)v);
        }
      }
    }
  };
  ev_cell_queue<EV_THREADS>(
      j0, j1, queue_j, queue_v, wsum,
      [&](int64_t j, bool in_range, int32_t &tv) {
        if (in_range) tv = trow[j];
        return tv != 0 && ev_kept(seed, keep, i, j);
      },
      one);
  if ((t & (WAVE - 1)) == 0 && cells != 0) atomicAdd(&cells_all, cells);
  __syncthreads();
  if (t < words) {
    const int word = t & (EG_WORDS - 1);
    unsigned long long v = table[t];
    if (word == 4) v = cells_all - table[t - 4];
    if (word == 5) v = cells_all;
    part[(i * slices + s) * words + t] = (long long)v;
  }
}

// per_user_out[u][.] (when wanted) = the sum over the slices of part[u][.][.]; one workgroup per EGF_USERS users, one
// thread per word of the table, whose sums over its users go to gpart[workgroup][words]
__global__ __launch_bounds__(1024) void evaluate_grid_finish_kernel(const long long *__restrict__ part, int64_t nu,
                                                                    int64_t slices, int words,
                                                                    long long *__restrict__ per_user_out,
                                                                    long long *__restrict__ gpart) {
  const int t = threadIdx.x;
  if (t >= words) return;
  const int64_t u0 = (int64_t)blockIdx.x * EGF_USERS, u1 = min(nu, u0 + EGF_USERS);
  long long col = 0;
  for (int64_t u = u0; u < u1; ++u) {
    long long sum = 0;
    for (int64_t s = 0; s < slices; ++s) sum += part[(u * slices + s) * words + t];
    if (per_user_out) per_user_out[u * words + t] = sum;
    col += sum;
  }
  gpart[(int64_t)blockIdx.x * words + t] = col;
}

// totals_out[.] = the sum of gpart[.][.] (one workgroup)
__global__ __launch_bounds__(1024) void evaluate_grid_totals_kernel(const long long *__restrict__ gpart, int64_t groups,
                                                                    int words, long long *__restrict__ totals_out) {
  const int t = threadIdx.x;
  if (t >= words) return;
  long long sum = 0;
  for (int64_t g = 0; g < groups; ++g) sum += gpart[g * words + t];
  totals_out[t] = sum;
}

// workspace: [part: nu x slices x S x 8 int64][gpart: ceil(nu / 16) x S x 8 int64]
QRLSH_EXPORT size_t qrlsh_evaluate_grid_workspace_bytes(int64_t nu, int64_t nq, int32_t settings) {
  if (nu <= 0 || nq <= 0 || settings <= 0 || settings > QRLSH_GRID_MAX_SETTINGS) return 0;
  return QR_LAYOUT_BYTES(ev_layout, nu, nq, (size_t)settings * EG_WORDS, EGF_USERS);
}

QRLSH_EXPORT int qrlsh_evaluate_grid(const int32_t *ratings, const int32_t *truth, int64_t nu, int64_t nq,
                                     const int64_t *q_off, const int32_t *q_idx, const int32_t *q_milli,
                                     const int32_t *u_idx, const double *u_val, int32_t ku, const int32_t *q_cuts,
                                     int32_t ncq, const int32_t *u_cuts, int32_t ncu, const double *weights, int32_t nw,
                                     int32_t sum_order, uint64_t seed, uint64_t keep, int64_t *per_user_out,
                                     int64_t *totals_out, uint32_t *flags_out, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  const char *who = "qrlsh_evaluate_grid";
  const int rc = ev_check_lists(who, nu, nq, ku, sum_order, keep);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(ncq >= 1 && ncq <= QRLSH_GRID_MAX_CUTS && ncu >= 1 && ncu <= QRLSH_GRID_MAX_CUTS && nw >= 1 &&
                   (int64_t)ncq * ncu * nw <= QRLSH_GRID_MAX_SETTINGS,
               "%s: bad grid ncq=%d ncu=%d (1 .. %d each) nw=%d (settings 1 .. %d)", who, ncq, ncu, QRLSH_GRID_MAX_CUTS, nw,
               QRLSH_GRID_MAX_SETTINGS);
  QR_CHECK_ARG(flags_out && totals_out && q_cuts && u_cuts && weights,
               "%s: flags_out, totals_out, q_cuts, u_cuts and weights are required", who);
  const bool empty = nu == 0 || nq == 0;
  QR_CHECK_ARG(empty || (ratings && truth && q_off && (ku == 0 || (u_idx && u_val))), "%s: null pointer", who);
  const int settings = ncq * ncu * nw, words = settings * EG_WORDS;
  const size_t need = qrlsh_evaluate_grid_workspace_bytes(nu, nq, settings);
  if (!empty) {
    QR_CHECK_ALIGNED(who, "the workspace", qr_addr(workspace), 8);
    QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, need);
  }
  const int64_t slices = ev_slices(nu, nq), groups = ceil_div64(nu, EGF_USERS);
  if (!empty && nu * slices > 2147483647ll) {
    qrlsh_set_error("%s: nu=%lld x %lld slices above 2^31 - 1 workgroups", who, (long long)nu, (long long)slices);
    return QRLSH_EUNSUPPORTED;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET(who, flags_out, 0, sizeof(uint32_t), st);
  if (empty) QR_MEMSET(who, totals_out, 0, (size_t)words * sizeof(int64_t), st);
  if (empty && nu > 0 && per_user_out) QR_MEMSET(who, per_user_out, 0, (size_t)nu * words * sizeof(int64_t), st);
  if (empty) {
    QR_LAUNCH("evaluate_grid_cuts", evaluate_grid_cuts_kernel, dim3(1), dim3(64), 0, st, q_cuts, (int)ncq, u_cuts,
              (int)ncu, flags_out);
    QR_LAUNCH_CHECK(who);
    return QRLSH_OK;
  }
  QrCarve c(workspace);
  const EvWs w = ev_layout(c, nu, nq, (size_t)words, EGF_USERS);
  long long *part = w.part, *gpart = w.gpart;
  const unsigned fin_threads = (unsigned)((words + WAVE - 1) / WAVE * WAVE);
  qr_lists_check("evaluate_check", q_off, q_idx, nq, nullptr, 0, nu, flags_out, st);   // the lists' two flags
  QR_LAUNCH("evaluate_grid", evaluate_grid_kernel, dim3((unsigned)(nu * slices)), dim3(EV_THREADS), 0, st, ratings, truth,
            nu, nq, q_off, q_idx, q_milli, u_idx, u_val, (int)ku, q_cuts, (int)ncq, u_cuts, (int)ncu, weights, (int)nw,
            (int)(sum_order == QRLSH_SUM_SEQUENTIAL), seed, keep, slices, part, flags_out);
  QR_LAUNCH("evaluate_grid_finish", evaluate_grid_finish_kernel, dim3((unsigned)groups), dim3(fin_threads), 0, st,
            (const long long *)part, nu, slices, words, reinterpret_cast<long long *>(per_user_out), gpart);
  QR_LAUNCH("evaluate_grid_totals", evaluate_grid_totals_kernel, dim3(1), dim3(fin_threads), 0, st,
            (const long long *)gpart, groups, words, reinterpret_cast<long long *>(totals_out));
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}

// An explicit test set: one thread per triplet (user, query, truth), the row read from memory; every triplet counts
// (repeats once each).  The workgroup's sums reach totals_out by 64-bit integer atomics: exact in any order.
constexpr int EVC_THREADS = 256;
__global__ __launch_bounds__(EVC_THREADS) void evaluate_cells_kernel(
    const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, const int64_t *__restrict__ q_off,
    const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli, const int32_t *__restrict__ u_idx,
    const double *__restrict__ u_val, int ku, double qw, double uw, double dmean, int sequential,
    const int32_t *__restrict__ cell_user, const int32_t *__restrict__ cell_query, const int32_t *__restrict__ cell_truth,
    int64_t m, int32_t *__restrict__ pred_out, unsigned long long *__restrict__ totals, uint32_t *__restrict__ flags) {
  __shared__ long long red[EVC_THREADS / WAVE][EV_WORDS];
  const int64_t c = (int64_t)blockIdx.x * EVC_THREADS + threadIdx.x;
  EvalStats st;
  st.clear();
  if (c < m) {
    const int64_t i = cell_user[c], j = cell_query[c];
    if (i < 0 || i >= nu || j < 0 || j >= nq) {  // flagged (bit 2); nothing of the cell is read
      atomicOr(flags, 4u);
      if (pred_out) pred_out[c] = -1;
    } else {
      const int32_t *row = ratings + i * nq;
      const int32_t *ui = u_idx + i * ku;
      const int mu = ev_list_len(ui, ku);
      int branch;
      const int32_t pred = ev_predict<true>(
          ratings, nu, nq, i, j, q_off, q_idx, q_milli, ui, u_val + i * ku, mu, qw, uw, dmean, sequential != 0,
          [&](int32_t q) { return row[q]; }, branch);
      st.add(pred, branch, cell_truth[c]);
      if (pred_out) pred_out[c] = pred;
    }
  }
  const long long sum = ev_block_sum<EVC_THREADS>(st, red);
  if (threadIdx.x < EV_WORDS && sum != 0) atomicAdd(totals + threadIdx.x, (unsigned long long)sum);
}

QRLSH_EXPORT int qrlsh_evaluate_cells(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                                      const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx,
                                      const double *u_val, int32_t ku, double query_weight, double user_weight,
                                      double default_mean, int32_t sum_order, const int32_t *cell_user,
                                      const int32_t *cell_query, const int32_t *cell_truth, int64_t m, int32_t *pred_out,
                                      int64_t *totals_out, uint32_t *flags_out, void *stream) {
  const int rc = ev_check_lists("qrlsh_evaluate_cells", nu, nq, ku, sum_order, 0);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(m >= 0 && ceil_div64(m, EVC_THREADS) <= 2147483647ll, "qrlsh_evaluate_cells: bad m=%lld", (long long)m);
  QR_CHECK_ARG(flags_out && totals_out, "qrlsh_evaluate_cells: flags_out and totals_out are required");
  QR_CHECK_ARG(m == 0 || (cell_user && cell_query && cell_truth), "qrlsh_evaluate_cells: null pointer");
  QR_CHECK_ARG(m == 0 || nu == 0 || nq == 0 || (ratings && q_off && (ku == 0 || (u_idx && u_val))),
               "qrlsh_evaluate_cells: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_evaluate_cells", flags_out, 0, sizeof(uint32_t), st);
  QR_MEMSET("qrlsh_evaluate_cells", totals_out, 0, 16 * sizeof(int64_t), st);
  if (m == 0) return QRLSH_OK;
  qr_lists_check("evaluate_check", q_off, q_idx, nq, nullptr, 0, nu, flags_out, st);   // the lists' two flags; ids: below
  QR_LAUNCH("evaluate_cells", evaluate_cells_kernel, dim3((unsigned)ceil_div64(m, EVC_THREADS)), dim3(EVC_THREADS), 0, st,
            ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean,
            (int)(sum_order == QRLSH_SUM_SEQUENTIAL), cell_user, cell_query, cell_truth, m, pred_out,
            reinterpret_cast<unsigned long long *>(totals_out), flags_out);
  QR_LAUNCH_CHECK("qrlsh_evaluate_cells");
  return QRLSH_OK;
}

// The hold-out copy: out = in with the kept non-zero cells set to 0, *count_out = how many.  A streaming kernel: 16-byte
// loads and stores over the flat matrix where both pointers are 16-byte aligned (a thread finds its first row by one
// division and steps from there), single words otherwise and for the last nu x nq % 4 cells.
constexpr int HO_THREADS = 256;
constexpr int HO_MAX_GROUPS = 4096;   // 16 workgroups per CU; a thread strides over the rest
__global__ __launch_bounds__(HO_THREADS) void ratings_holdout_kernel(const int32_t *__restrict__ in, int64_t nq,
                                                                     int64_t total, int64_t n4, int64_t step_i,
                                                                     int64_t step_j, uint64_t seed, uint64_t keep,
                                                                     int32_t *__restrict__ out,
                                                                     unsigned long long *__restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * HO_THREADS;
  const int64_t g = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  uint32_t zeroed = 0;
  const int4 *in4 = reinterpret_cast<const int4 *>(in);
  int4 *out4 = reinterpret_cast<int4 *>(out);
  // (i, j) of the thread's next vector: one division at the start, then steps of one stride = step_i rows + step_j
  // columns (the host's division)
  int64_t ci = 0, cj = 0;
  if (g < n4) {
    ci = (g * 4) / nq;
    cj = g * 4 - ci * nq;
  }
  auto four = [&](int4 v) {
    int64_t i = ci, j = cj;
    ci += step_i;
    cj += step_j;
    if (cj >= nq) {
      cj -= nq;
      ++ci;
    }
    int32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (e[k] != 0 && ev_kept(seed, keep, i, j)) {
        e[k] = 0;
        ++zeroed;
      }
      if (++j == nq) {
        j = 0;
        ++i;
      }
    }
    return make_int4(e[0], e[1], e[2], e[3]);
  };
  // two vectors per trip, both loads issued before either is used
  for (int64_t c4 = g; c4 < n4; c4 += 2 * stride) {
    const int64_t d4 = c4 + stride;
    const bool two = d4 < n4;
    const int4 v0 = in4[c4];
    const int4 v1 = two ? in4[d4] : make_int4(0, 0, 0, 0);
    out4[c4] = four(v0);
    if (two) out4[d4] = four(v1);
  }
  for (int64_t c = n4 * 4 + g; c < total; c += stride) {
    const int64_t i = c / nq, j = c - i * nq;
    int32_t v = in[c];
    if (v != 0 && ev_kept(seed, keep, i, j)) {
      v = 0;
      ++zeroed;
    }
    out[c] = v;
  }
  // one atomic per workgroup: thousands of adds to one word cost more than the copy
  __shared__ uint32_t wz[HO_THREADS / WAVE];
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) zeroed += __shfl_xor(zeroed, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) wz[threadIdx.x >> 6] = zeroed;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < HO_THREADS / WAVE; ++k) sum += wz[k];
    if (sum) atomicAdd(count, sum);
  }
}

QRLSH_EXPORT int qrlsh_ratings_holdout(const int32_t *in, int64_t nu, int64_t nq, uint64_t seed, uint64_t keep, int32_t *out,
                                       int64_t *count_out, void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && nu <= 2147483647ll && nq <= 2147483647ll, "qrlsh_ratings_holdout: bad sizes nu=%lld nq=%lld",
               (long long)nu, (long long)nq);
  QR_CHECK_ARG(keep <= (1ull << 32), "qrlsh_ratings_holdout: keep=%llu above 2^32", (unsigned long long)keep);
  QR_CHECK_ARG(count_out, "qrlsh_ratings_holdout: count_out is required");
  const int64_t total = nu * nq;
  QR_CHECK_ARG(total == 0 || (in && out && in != out), "qrlsh_ratings_holdout: null pointer, or in == out");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_ratings_holdout", count_out, 0, sizeof(int64_t), st);
  if (total == 0) return QRLSH_OK;
  const bool aligned = ((uintptr_t)in | (uintptr_t)out) % 16 == 0;
  const int64_t n4 = aligned ? total / 4 : 0;
  int64_t groups = ceil_div64(aligned ? ceil_div64(total, 4) : total, HO_THREADS);
  if (groups > HO_MAX_GROUPS) groups = HO_MAX_GROUPS;   // grid-stride beyond
  const int64_t step = groups * HO_THREADS * 4;   // cells between a thread's vectors
  QR_LAUNCH("ratings_holdout", ratings_holdout_kernel, dim3((unsigned)groups), dim3(HO_THREADS), 0, st, in, nq, total, n4,
            step / nq, step % nq, seed, keep, out, reinterpret_cast<unsigned long long *>(count_out));
  QR_LAUNCH_CHECK("qrlsh_ratings_holdout");
  return QRLSH_OK;
}
