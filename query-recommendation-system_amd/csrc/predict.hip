// predict.hip -- N1: the hybrid prediction loop (consumer of the hot path's output), in the three forms that are
// SERVED: the whole matrix (qrlsh_predict: cell, row and tile forms), the columns of new queries
// (qrlsh_predict_columns) and the rows of chosen users (qrlsh_predict_users, qr_predict_users), with the check of the
// lists that every consumer launches (qr_lists_check).  The evaluation of the predictions is in evaluate.hip, the
// ranking evaluation in rankeval.hip and rankgrid.hip; the arithmetic all of them share is in evalsides.h.
//
// Reference: Recommender.compute_scores, recommender.py:301-331, and weighted_average,
// recommender.py:36-47.  Every zero cell (user i, query j) of the utility matrix gets
//     qp = weighted_average(ratings[i],    query_sims[j])      (content-based, :313-317)
//     up = weighted_average(ratings[:, j], user_sims[i])       (collaborative,  :320)
// blended by the rules of :324-331 and rounded with Python's round() (half to even).
// One thread per cell; every cell is independent.  float64 throughout, compiled with
// -ffp-contract=off, the blend evaluated in the reference's operand order, rint() = round-half-to-even.
//
// Order of the two sums inside weighted_average (np.sum(ur * vals) and np.sum(vals[ur != 0])):
//   QRLSH_SUM_PAIRWISE   numpy's pairwise_sum (8 running sums, combined as a tree, tail added one by one):
//                        what np.sum does when weighted_average runs as plain Python.  The golden fixtures
//                        (tests/golden/cfg1*_scores.npz) were captured that way -- numba is not installable
//                        here, tools/make_golden.py replaces @jit by the identity -- so THIS order is the one
//                        parity is pinned for.
//   QRLSH_SUM_SEQUENTIAL one accumulator, index order: what numba's nopython np.sum compiles to, i.e. what
//                        the reference computes where numba is installed.  Unpinned (no fixture can be made
//                        here); differs from the pairwise order by an ulp of the sums for lists of 8 or more,
//                        which can flip a cell whose blend lies exactly on .5.
// No per-thread arrays: the products are accumulated while the ratings are gathered (the position of a
// product in the sum is its neighbour index), the non-zero flags of the ratings are kept as one 64-bit mask,
// and the weight sum walks the mask's set bits (the position of a weight in the compacted list is its rank
// in the mask) -- so a neighbour list of up to 64 entries needs 8 accumulators, not four 64-entry arrays.
#include "common.h"
#include "evalsides.h"   // PRED_MAXK, weighted_average, the blend, the cell prediction, the row staging

// TL: the query neighbour lists come transposed and padded, idx_t / val_t [kq][nq] (entry k of query j at
// k * nq + j; predict_lists_transpose_kernel): consecutive lanes = consecutive queries then read consecutive words,
// where the CSR form costs a separate cache line per lane for every list entry (q_idx / q_val = idx_t / val_t).
template <bool TL>
__global__ __launch_bounds__(256) void predict_kernel(const int32_t *__restrict__ ratings, int64_t nu, int64_t nq,
                                                      const int64_t *__restrict__ q_off,
                                                      const int32_t *__restrict__ q_idx,
                                                      const double *__restrict__ q_val,
                                                      const int32_t *__restrict__ u_idx,
                                                      const double *__restrict__ u_val, int ku, double qw, double uw,
                                                      double dmean, int sequential, int nlimit,
                                                      int32_t *__restrict__ out,
                                                      const uint32_t *__restrict__ only_if = nullptr) {
  if (only_if && *only_if == 0) return;  // the tile form has done the work
  // consecutive lanes = consecutive queries of ONE user: the user-side gathers ratings[u][j] are coalesced
  // across the wave and the user's neighbour list is wave-uniform; the query-side gathers stay inside the
  // user's own row (4 nq bytes, cache-resident while the row's workgroups run)
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= nu * nq) return;
  const int64_t i = cell / nq, j = cell - i * nq;
  const int32_t own = ratings[cell];
  if (own != 0) {
    out[cell] = own;
    return;
  }
  // query side: neighbours of query j, this user's ratings of them
  const int64_t lo = q_off[j];
  const int64_t n64 = q_off[j + 1] - lo;
  // a list longer than the limit (PRED_MAXK entries, or the kq rows of the transposed workspace) is never walked:
  // predict_check_kernel has raised *too_long_out for it, the cell gets 0 and the caller discards the result
  if (n64 < 0 || n64 > nlimit) {
    out[cell] = 0;
    return;
  }
  const int n = (int)n64;
  const int32_t *row = ratings + i * nq;
  const double qp = TL ? weighted_average(
                             n, sequential != 0, [&](int k) { return row[q_idx[(int64_t)k * nq + j]]; },
                             [&](int k) { return q_val[(int64_t)k * nq + j]; })
                       : weighted_average(
                             n, sequential != 0, [&](int k) { return row[q_idx[lo + k]]; },
                             [&](int k) { return q_val[lo + k]; });
  // user side: neighbours of user i (-1 padded), their ratings of query j
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  const int m = ev_list_len(ui, ku);
  const double up = weighted_average(
      m, sequential != 0, [&](int k) { return ratings[(int64_t)ui[k] * nq + j]; }, [&](int k) { return uv[k]; });
  out[cell] = ev_blend_round(qp, up, qw, uw, dmean);
}

// Row form of the sweep (transposed lists only): one 1024-thread workgroup per (user, slice of the user's cells).
// Every query-side gather of a cell reads the SAME user's row -- ratings[i][q_idx[..]], a random word of a
// 4 nq-byte row per neighbour, each its own trip to L2 in the kernel above.  Ratings are small non-negative
// integers (0 .. 100 in the reference's data), so the workgroup first stages its user's whole row in LDS as BYTES
// (nq <= 128 K queries; a value outside 0 .. 255 anywhere in the row makes the workgroup read the row from memory
// instead -- same results) and the neighbour gathers become LDS byte reads.  The user-side gathers
// (ratings[u_k][j], consecutive lanes = consecutive j) stay coalesced global reads.
constexpr int PR_THREADS = 1024;
__global__ __launch_bounds__(PR_THREADS) void predict_row_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                 int64_t nq, const int64_t *__restrict__ q_off,
                                                                 const int32_t *__restrict__ idx_t,
                                                                 const double *__restrict__ val_t,
                                                                 const int32_t *__restrict__ u_idx,
                                                                 const double *__restrict__ u_val, int ku, double qw,
                                                                 double uw, double dmean, int sequential, int nlimit,
                                                                 int32_t *__restrict__ out,
                                                                 const uint32_t *__restrict__ only_if = nullptr) {
  __shared__ uint8_t lrow[PR_MAXQ];
  __shared__ int wide;
  if (only_if && *only_if == 0) return;  // the tile form has done the work
  const int64_t i = blockIdx.y;
  const int t = threadIdx.x;
  const int32_t *row = ratings + i * nq;
  const bool in_lds = ev_stage_row<PR_THREADS>(row, nq, lrow, &wide);  // uniform
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  const int m = ev_list_len(ui, ku);  // uniform: the user's own neighbour list
  // this workgroup's slice of the row
  const int64_t per = (nq + gridDim.x - 1) / gridDim.x;
  const int64_t j0 = (int64_t)blockIdx.x * per, j1 = min(nq, j0 + per);
  for (int64_t j = j0 + t; j < j1; j += PR_THREADS) {
    const int64_t cell = i * nq + j;
    const int32_t own = in_lds ? (int32_t)lrow[j] : row[j];
    if (own != 0) {
      out[cell] = own;
      continue;
    }
    const int64_t n64 = q_off[j + 1] - q_off[j];
    if (n64 < 0 || n64 > nlimit) {  // flagged by predict_check_kernel; never walked
      out[cell] = 0;
      continue;
    }
    const double qp = weighted_average(
        (int)n64, sequential != 0,
        [&](int k) {
          const int32_t q = idx_t[(int64_t)k * nq + j];
          return in_lds ? (int32_t)lrow[q] : row[q];
        },
        [&](int k) { return val_t[(int64_t)k * nq + j]; });
    const double up = weighted_average(
        m, sequential != 0, [&](int k) { return ratings[(int64_t)ui[k] * nq + j]; }, [&](int k) { return uv[k]; });
    out[cell] = ev_blend_round(qp, up, qw, uw, dmean);
  }
}

// ---- tile form ------------------------------------------------------------------------------------------
// Both sweeps above walk a cell's two neighbour lists with per-lane loads: every user's pass over the row re-reads
// ALL query lists (kq x nq x 12 bytes, 2000 times on the bench shape: 67 GB out of L2) -- the lists, not the ratings,
// are what those kernels move.  Here the matrix is first transposed to BYTES, rt[q][u] (ratings are small
// non-negative integers; a value outside 0 .. 255 raises a flag and the row form runs instead), and a workgroup
// owns a tile of 64 users x 16 queries: wave w = query j0 + w, lane = user u0 + lane.  Then
//   * a wave's query list (index, similarity) is the same for all its lanes: read once from LDS, broadcast;
//   * the query-side gathers ratings[u][idx] = rt[idx][u0 + lane] are 64 consecutive bytes per neighbour;
//   * the user-side gathers ratings[u_k][j] = rt[j][u_k] stay inside ONE 'nu'-byte row of rt per wave;
//   * every list is read once per tile (64 users' lists, 16 queries' lists: LDS), not once per cell;
//   * the output tile is turned in LDS and written as 64-byte row segments.
// The arithmetic per cell is the same weighted_average, in the same order.
constexpr int PT_USERS = 64;
constexpr int PT_QUERIES = 16;
constexpr int PT_THREADS = PT_USERS * PT_QUERIES;
constexpr int PT_MAXKU = 32;   // user lists beyond this take the row form

// ratings int32 [nu][nq] -> rt uint8 [nq][nus] (64 x 64 tiles through LDS: coalesced both ways); *wide |= 1 when a
// value does not fit a byte
__global__ __launch_bounds__(256) void predict_transpose_u8_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                   int64_t nq, int64_t nus, uint8_t *__restrict__ rt,
                                                                   uint32_t *__restrict__ wide) {
  __shared__ uint8_t tile[64][65];
  const int64_t q0 = (int64_t)blockIdx.x * 64, u0 = (int64_t)blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  bool bad = false;
  for (int r = ty; r < 64; r += 4) {
    const int64_t u = u0 + r, q = q0 + tx;
    int32_t v = 0;
    if (u < nu && q < nq) v = ratings[u * nq + q];
    bad |= (v < 0) | (v > 255);
    tile[r][tx] = (uint8_t)v;
  }
  if (bad) atomicOr(wide, 1u);
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int64_t q = q0 + r, u = u0 + tx;
    if (q < nq && u < nus) rt[q * nus + u] = tile[tx][r];
  }
}

__global__ __launch_bounds__(PT_THREADS, 8) void predict_tile_kernel(const uint8_t *__restrict__ rt, int64_t nus,
                                                                  const int32_t *__restrict__ ratings, int64_t nu,
                                                                  int64_t nq, const int64_t *__restrict__ q_off,
                                                                  const int32_t *__restrict__ q_idx,
                                                                  const double *__restrict__ q_val,
                                                                  const int32_t *__restrict__ u_idx,
                                                                  const double *__restrict__ u_val, int ku, double qw,
                                                                  double uw, double dmean, int sequential, int nlimit,
                                                                  const uint32_t *__restrict__ wide,
                                                                  int32_t *__restrict__ out) {
  __shared__ double lval[PT_QUERIES][PRED_MAXK];
  __shared__ int32_t lidx[PT_QUERIES][PRED_MAXK];
  __shared__ double uval[PT_USERS][PT_MAXKU + 1];
  __shared__ int32_t uidx[PT_USERS][PT_MAXKU + 1];
  __shared__ int32_t otile[PT_USERS][PT_QUERIES + 1];
  if (*wide) return;  // uniform: some rating does not fit a byte, the row form (launched next) does the work
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * PT_QUERIES, u0 = (int64_t)blockIdx.y * PT_USERS;
  // the tile's lists: 16 query lists (CSR) and 64 user lists (padded [nu][ku]), each read once
  for (int e = t; e < PT_QUERIES * PRED_MAXK; e += PT_THREADS) {
    const int jj = e / PRED_MAXK, k = e - jj * PRED_MAXK;
    const int64_t j = j0 + jj;
    int32_t ix = 0;
    double vv = 0.0;
    if (j < nq) {
      const int64_t lo = q_off[j], n = q_off[j + 1] - lo;
      if (k < n && n <= nlimit) {
        ix = q_idx[lo + k];
        vv = q_val[lo + k];
      }
    }
    lidx[jj][k] = ix;
    lval[jj][k] = vv;
  }
  for (int e = t; e < PT_USERS * PT_MAXKU; e += PT_THREADS) {
    const int ul = e / PT_MAXKU, k = e - ul * PT_MAXKU;
    const int64_t u = u0 + ul;
    int32_t ix = -1;
    double vv = 0.0;
    if (u < nu && k < ku) {
      ix = u_idx[u * ku + k];
      vv = u_val[u * ku + k];
    }
    uidx[ul][k] = ix;
    uval[ul][k] = vv;
  }
  __syncthreads();
  const int64_t j = j0 + w, u = u0 + lane;
  int32_t res = 0;
  if (j < nq && u < nu) {
    const uint8_t *rj = rt + j * nus;
    const int32_t own = (int32_t)rj[u];
    res = own;
    const int64_t n64 = q_off[j + 1] - q_off[j];  // (wave-uniform)
    if (own == 0 && n64 >= 0 && n64 <= nlimit) {
      const double qp = weighted_average(
          (int)n64, sequential != 0, [&](int k) { return (int32_t)rt[(int64_t)lidx[w][k] * nus + u]; },
          [&](int k) { return lval[w][k]; });
      const int m = ev_list_len(uidx[lane], ku);
      const double up = weighted_average(
          m, sequential != 0, [&](int k) { return (int32_t)rj[uidx[lane][k]]; }, [&](int k) { return uval[lane][k]; });
      res = ev_blend_round(qp, up, qw, uw, dmean);
    }
  }
  otile[lane][w] = res;
  __syncthreads();
  {
    // 16 consecutive threads write one user's 16 cells (64 bytes)
    const int ul = t >> 4, jj = t & 15;
    const int64_t uu = u0 + ul, jw = j0 + jj;
    if (uu < nu && jw < nq) out[uu * nq + jw] = otile[ul][jj];
  }
}

// longest query neighbour list (host pre-check of the 64-entry limit without a read-back: the kernel below
// raises a device flag, the caller reads it together with the result)
__global__ __launch_bounds__(256) void predict_check_kernel(const int64_t *__restrict__ q_off, int64_t nq, int maxlen,
                                                            uint32_t *__restrict__ too_long) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nq && q_off[j + 1] - q_off[j] > maxlen) atomicOr(too_long, 1u);
}

// CSR neighbour lists -> [kq][nq], coalesced writes (one thread per output word; -1 / 0.0 past a list's end)
__global__ __launch_bounds__(256) void predict_lists_transpose_kernel(const int64_t *__restrict__ q_off,
                                                                      const int32_t *__restrict__ q_idx,
                                                                      const double *__restrict__ q_val, int64_t nq,
                                                                      int kq, int32_t *__restrict__ idx_t,
                                                                      double *__restrict__ val_t,
                                                                      const uint32_t *__restrict__ only_if = nullptr) {
  if (only_if && *only_if == 0) return;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)kq * nq) return;
  const int64_t k = t / nq, j = t - k * nq;
  const int64_t lo = q_off[j];
  const bool in = k < q_off[j + 1] - lo;
  idx_t[t] = in ? q_idx[lo + k] : -1;
  val_t[t] = in ? q_val[lo + k] : 0.0;
}

static int64_t pt_stride(int64_t nu) { return (nu + 63) / 64 * 64; }

// workspace: [transposed query lists: kq x nq doubles, kq x nq int32 (row / cell forms)][16 B: flags]
//            [byte matrix rt: nq x round_up(nu, 64) (tile form)]
struct PredictWs {
  double *val_t;
  int32_t *idx_t;
  uint32_t *wide;
  uint8_t *rt;
};
static PredictWs predict_layout(QrCarve &c, int64_t nu, int64_t nq, int32_t kq) {
  PredictWs w;
  w.val_t = c.take<double>((size_t)kq * (size_t)nq, 8);
  w.idx_t = c.take<int32_t>((size_t)kq * (size_t)nq, 4);
  w.wide = c.take<uint32_t>(4, 4);   // 4-byte aligned; 16 bytes reserved
  w.rt = c.take<uint8_t>((size_t)nq * (size_t)pt_stride(nu), 1);
  return w;
}
QRLSH_EXPORT size_t qrlsh_predict_workspace_bytes(int64_t nu, int64_t nq, int32_t kq) {
  if (nu <= 0 || nq <= 0 || kq <= 0) return 0;
  return QR_LAYOUT_BYTES(predict_layout, nu, nq, kq);
}

QRLSH_EXPORT int qrlsh_predict(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                               const int32_t *q_idx, const double *q_val, const int32_t *u_idx, const double *u_val,
                               int32_t ku, double query_weight, double user_weight, double default_mean,
                               int32_t sum_order, int32_t *out, uint32_t *too_long_out, int32_t kq, void *workspace,
                               size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && ku >= 0 && ku <= PRED_MAXK, "qrlsh_predict: bad sizes nu=%lld nq=%lld ku=%d (<= %d)",
               (long long)nu, (long long)nq, ku, PRED_MAXK);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL, "qrlsh_predict: bad sum_order %d",
               sum_order);
  QR_CHECK_ARG(too_long_out, "qrlsh_predict: too_long_out is required");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_predict", too_long_out, 0, sizeof(uint32_t), st);
  if (nu == 0 || nq == 0) return QRLSH_OK;
  QR_CHECK_ARG(ratings && q_off && out && (ku == 0 || (u_idx && u_val)), "qrlsh_predict: null pointer");
  const bool tl = kq > 0 && workspace != nullptr;
  QR_CHECK_ARG(kq >= 0 && kq <= PRED_MAXK && (!tl || workspace_bytes >= qrlsh_predict_workspace_bytes(nu, nq, kq)),
               "qrlsh_predict: kq=%d (<= %d) needs %zu workspace bytes, got %zu", kq, PRED_MAXK,
               qrlsh_predict_workspace_bytes(nu, nq, kq), workspace_bytes);
  QR_LAUNCH("predict_check", predict_check_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, st, q_off, nq,
            tl ? (int)kq : PRED_MAXK, too_long_out);
  const int seq = (int)(sum_order == QRLSH_SUM_SEQUENTIAL);
  if (!tl) {
    QR_LAUNCH("predict", predict_kernel<false>, dim3((unsigned)ceil_div64(nu * nq, 256)), dim3(256), 0, st, ratings, nu,
              nq, q_off, q_idx, q_val, u_idx, u_val, ku, query_weight, user_weight, default_mean, seq, PRED_MAXK, out);
    QR_LAUNCH_CHECK("qrlsh_predict");
    return QRLSH_OK;
  }
  QrCarve c(workspace);
  const PredictWs w = predict_layout(c, nu, nq, kq);
  double *val_t = w.val_t;
  int32_t *idx_t = w.idx_t;
  uint32_t *wide = w.wide;
  uint8_t *rt = w.rt;
  const bool tile = ku <= PT_MAXKU && ceil_div64(nq, PT_QUERIES) <= 2147483647ll && ceil_div64(nu, PT_USERS) <= 65535 &&
                    ceil_div64(nu, 64) <= 65535;
  const bool row = nq <= PR_MAXQ && nu <= 65535;
  if (tile) {
    // tile form; the row (or cell) form follows and does nothing unless a rating did not fit a byte
    const int64_t nus = pt_stride(nu);
    QR_MEMSET("qrlsh_predict", wide, 0, 16, st);
    QR_LAUNCH("predict_transpose", predict_transpose_u8_kernel,
              dim3((unsigned)ceil_div64(nq, 64), (unsigned)ceil_div64(nu, 64)), dim3(256), 0, st, ratings, nu, nq, nus, rt,
              wide);
    QR_LAUNCH("predict", predict_tile_kernel, dim3((unsigned)ceil_div64(nq, PT_QUERIES), (unsigned)ceil_div64(nu, PT_USERS)),
              dim3(PT_THREADS), 0, st, (const uint8_t *)rt, nus, ratings, nu, nq, q_off, q_idx, q_val, u_idx, u_val, ku,
              query_weight, user_weight, default_mean, seq, (int)kq, (const uint32_t *)wide, out);
  }
  // lists transposed once ([kq][nq], doubles first: 8-byte aligned), then read coalesced by every user's sweep
  const uint32_t *only_if = tile ? (const uint32_t *)wide : nullptr;
  QR_LAUNCH("predict_lists", predict_lists_transpose_kernel, dim3((unsigned)ceil_div64((int64_t)kq * nq, 256)), dim3(256), 0,
            st, q_off, q_idx, q_val, nq, (int)kq, idx_t, val_t, only_if);
  if (row) {
    // row form: slices so that a few thousand workgroups exist whatever the number of users
    int64_t slices = ceil_div64(4096, nu);
    const int64_t most = ceil_div64(nq, PR_THREADS);
    if (slices > most) slices = most;
    if (slices < 1) slices = 1;
    QR_LAUNCH("predict_rows", predict_row_kernel, dim3((unsigned)slices, (unsigned)nu), dim3(PR_THREADS), 0, st, ratings, nu,
              nq, q_off, (const int32_t *)idx_t, (const double *)val_t, u_idx, u_val, ku, query_weight, user_weight,
              default_mean, seq, (int)kq, out, only_if);
  } else {
    QR_LAUNCH("predict_cells", predict_kernel<true>, dim3((unsigned)ceil_div64(nu * nq, 256)), dim3(256), 0, st, ratings, nu,
              nq, q_off, (const int32_t *)idx_t, (const double *)val_t, u_idx, u_val, ku, query_weight, user_weight,
              default_mean, seq, (int)kq, out, only_if);
  }
  QR_LAUNCH_CHECK("qrlsh_predict");
  return QRLSH_OK;
}

// ---- column prediction: the cells of NEW queries (qrlsh_predict_columns) --------------------------------------------
// A query x that is not a column of the matrix has no ratings, so the user side of every cell (u, x) is 0
// (weighted_average over an all-zero column, recommender.py:320) and only the query side decides:
//     out[x][u] = qp == 0 ? 0 : rint(qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5)),  qp = weighted_average(ratings[u],
// x's list) -- ev_blend with up = 0.  One workgroup per (new query, block of 256 users): the list
// (<= 64 entries; similarity = milli / 1000.0, a true division) sits in LDS, lane = user.
constexpr int PC_THREADS = 256;
__global__ __launch_bounds__(PC_THREADS) void predict_columns_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                     int64_t nq, const int64_t *__restrict__ off,
                                                                     const int32_t *__restrict__ idx,
                                                                     const int32_t *__restrict__ milli, double qw,
                                                                     double uw, double dmean, int sequential,
                                                                     int32_t *__restrict__ out,
                                                                     uint32_t *__restrict__ flags) {
  __shared__ int32_t lidx[PRED_MAXK];
  __shared__ double lval[PRED_MAXK];
  __shared__ int bad;
  const int64_t x = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t u = (int64_t)blockIdx.y * PC_THREADS + t;
  const int64_t lo = off[x], n64 = off[x + 1] - lo;
  const bool fits = n64 >= 0 && n64 <= PRED_MAXK;
  if (t == 0) bad = fits ? 0 : 1;
  __syncthreads();
  if (fits && t < n64) {
    const int32_t ix = idx[lo + t];
    if (ix < 0 || ix >= nq) bad = 2;   // never gathered
    lidx[t] = ix;
    lval[t] = (double)milli[lo + t] / 1000.0;
  }
  __syncthreads();
  const int why = bad;
  if (why) {  // too long (bit 0) or an index outside the matrix (bit 1): flagged, the column gets 0
    if (t == 0 && blockIdx.y == 0) atomicOr(flags, (uint32_t)why);
    if (u < nu) out[x * nu + u] = 0;
    return;
  }
  if (u >= nu) return;
  const int32_t *row = ratings + u * nq;
  const double qp = weighted_average(
      (int)n64, sequential != 0, [&](int k) { return row[lidx[k]]; }, [&](int k) { return lval[k]; });
  out[x * nu + u] = ev_blend_round(qp, 0.0, qw, uw, dmean);
}

QRLSH_EXPORT int qrlsh_predict_columns(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *off,
                                       const int32_t *idx, const int32_t *milli, int64_t m, double query_weight,
                                       double user_weight, double default_mean, int32_t sum_order, int32_t *out,
                                       uint32_t *flags_out, void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && m >= 0 && ceil_div64(nu, PC_THREADS) <= 65535 && m <= 2147483647ll,
               "qrlsh_predict_columns: bad sizes nu=%lld nq=%lld m=%lld", (long long)nu, (long long)nq, (long long)m);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL,
               "qrlsh_predict_columns: bad sum_order %d", sum_order);
  QR_CHECK_ARG(flags_out, "qrlsh_predict_columns: flags_out is required");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_predict_columns", flags_out, 0, sizeof(uint32_t), st);
  if (nu == 0 || m == 0) return QRLSH_OK;
  QR_CHECK_ARG(off && out && (nq == 0 || (ratings && idx && milli)), "qrlsh_predict_columns: null pointer");
  QR_LAUNCH("predict_columns", predict_columns_kernel, dim3((unsigned)m, (unsigned)ceil_div64(nu, PC_THREADS)),
            dim3(PC_THREADS), 0, st, ratings, nu, nq, off, idx, milli, query_weight, user_weight, default_mean,
            (int)(sum_order == QRLSH_SUM_SEQUENTIAL), out, flags_out);
  QR_LAUNCH_CHECK("qrlsh_predict_columns");
  return QRLSH_OK;
}

// ---- the rows of chosen users (qrlsh_predict_users, qrlsh_recommend_users) -------------------------------------------
// What a server needs to answer "what do I show user u now?": predict_kernel's cells for the requested rows only,
// straight from the live lists (CSR, similarity = milli / 1000.0, a true division as in predict_columns_kernel) -- no
// [nu][nq] prediction matrix and no transposed copy of the lists.  One 1024-thread workgroup per (column slice,
// requested user), the requested users varying fastest so that the workgroups of one slice run together and share that
// slice's lists in L2.  Two forms, decided on the device, same results:
//   LDS row form (nq <= PR_MAXQ and every value of the user's row in 0 .. 255): predict_row_kernel's scheme -- the
//     workgroup stages its user's whole row in LDS as bytes and the query-side gathers become LDS byte reads;
//   global form otherwise (a wider value anywhere in the row, found while staging, or a longer row): the gathers read
//     the user's int32 row from memory.
// The user-side gathers (ratings[u_k][j], consecutive lanes = consecutive j) are coalesced global reads in both.
// ELIGIBLE = false: completed rows (the rating where rated: the rows qrlsh_predict writes); true: 0 where rated, so
// that out != 0 is exactly the recommendation's eligibility test (ratings == 0 && pred != 0).
// Nothing outside the buffers is read whatever the inputs hold: a list longer than PRED_MAXK is not walked, an index
// outside [0, nq) is not gathered (both: the cell gets 0), the row of a user id outside [0, nu) is not read (the output
// row gets 0).  predict_users_check_kernel raises the flags for all three, whatever the ratings are.

// The prediction of an unrated cell is ev_predict<false> of evalsides.h: the cell of a served row holds no rating
// that the sides would have to leave out.
template <bool ELIGIBLE>
__global__ __launch_bounds__(PU_THREADS) void predict_users_kernel(
    const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, const int64_t *__restrict__ q_off,
    const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli, const int32_t *__restrict__ u_idx,
    const double *__restrict__ u_val, int ku, double qw, double uw, double dmean, int sequential,
    const int32_t *__restrict__ users, int64_t m, int64_t slices, int32_t *__restrict__ out, int64_t ostride) {
  __shared__ uint8_t lrow[PR_MAXQ];
  __shared__ int wide;
  const int64_t s = blockIdx.x / m, x = blockIdx.x - s * m;
  const int t = threadIdx.x;
  const int64_t per = (nq + slices - 1) / slices;
  const int64_t j0 = s * per, j1 = min(nq, j0 + per);
  int32_t *orow = out + x * ostride;
  const int64_t i = users ? (int64_t)users[x] : x;
  if (i < 0 || i >= nu) {  // uniform; flagged (bit 2) by the check kernel
    for (int64_t j = j0 + t; j < j1; j += PU_THREADS) orow[j] = 0;
    return;
  }
  const int32_t *row = ratings + i * nq;
  bool in_lds = false;
  if (nq <= PR_MAXQ) in_lds = ev_stage_row<PU_THREADS>(row, nq, lrow, &wide);  // uniform
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  const int mu = ev_list_len(ui, ku);  // uniform: the user's own neighbour list
  for (int64_t j = j0 + t; j < j1; j += PU_THREADS) {
    const int32_t own = in_lds ? (int32_t)lrow[j] : row[j];
    if (own != 0) {
      orow[j] = ELIGIBLE ? 0 : own;
      continue;
    }
    int branch;
    orow[j] = ev_predict<false>(
        ratings, nu, nq, i, j, q_off, q_idx, q_milli, ui, uv, mu, qw, uw, dmean, sequential != 0,
        [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; }, branch);
  }
}

// one thread per query list and per requested user: bit 0 a list longer than PRED_MAXK, bit 1 an index outside
// [0, nq) (lists within the limit only: longer ones are not walked here either), bit 2 a user id outside [0, nu)
__global__ __launch_bounds__(256) void predict_users_check_kernel(const int64_t *__restrict__ q_off,
                                                                  const int32_t *__restrict__ q_idx, int64_t nq,
                                                                  const int32_t *__restrict__ users, int64_t m,
                                                                  int64_t nu, uint32_t *__restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t why = 0;
  if (t < nq) {
    const int64_t lo = q_off[t], n = q_off[t + 1] - lo;
    if (n < 0 || n > PRED_MAXK) {
      why |= 1u;
    } else {
      for (int64_t k = 0; k < n; ++k)
        if ((uint32_t)q_idx[lo + k] >= (uint32_t)nq) why |= 2u;
    }
  }
  if (users && t < m) {
    const int64_t u = users[t];
    if (u < 0 || u >= nu) why |= 4u;
  }
  if (why) atomicOr(flags, why);
}

void qr_lists_check(const char *label, const int64_t *q_off, const int32_t *q_idx, int64_t nq, const int32_t *users,
                    int64_t m, int64_t nu, uint32_t *flags, hipStream_t st) {
  const int64_t checks = nq > m ? nq : m;
  if (checks > 0)
    QR_LAUNCH(label, predict_users_check_kernel, dim3((unsigned)ceil_div64(checks, 256)), dim3(256), 0, st, q_off, q_idx,
              nq, users, users ? m : (int64_t)0, nu, flags);
}

// Both entry points' common part: every check of the shared arguments (all before any device work), the flags, the
// check kernel and the sweep.  `out` rows are `ostride` words apart.
int qr_predict_users(const char *who, const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                     const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                     double query_weight, double user_weight, double default_mean, int32_t sum_order,
                     const int32_t *users, int64_t m, bool eligible, int32_t *out, int64_t ostride, uint32_t *flags_out,
                     hipStream_t st) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && nq <= 2147483647ll && m >= 0 && ku >= 0 && ku <= PRED_MAXK,
               "%s: bad sizes nu=%lld nq=%lld m=%lld ku=%d (<= %d)", who, (long long)nu, (long long)nq, (long long)m, ku,
               PRED_MAXK);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL, "%s: bad sum_order %d", who,
               sum_order);
  QR_CHECK_ARG(users || m == nu, "%s: without a user list m (%lld) must equal nu (%lld)", who, (long long)m,
               (long long)nu);
  QR_CHECK_ARG(flags_out, "%s: flags_out is required", who);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(nq == 0 || (q_off && out && (nu == 0 || (ratings && (ku == 0 || (u_idx && u_val))))), "%s: null pointer",
               who);
  if (m > (1ll << 24)) {
    qrlsh_set_error("%s: m=%lld above the %lld rows served per call", who, (long long)m, (long long)(1ll << 24));
    return QRLSH_EUNSUPPORTED;
  }
  QR_MEMSET(who, flags_out, 0, sizeof(uint32_t), st);
  qr_lists_check("predict_users_check", q_off, q_idx, nq, users, m, nu, flags_out, st);
  if (nq > 0) {
    int64_t slices = ceil_div64(PU_AUTO_GROUPS, m);
    const int64_t most = ceil_div64(nq, PU_THREADS);
    if (slices > most) slices = most;   // m x slices <= 2^24 + 2^21 workgroups
    const dim3 grid((unsigned)(m * slices));
    const int seq = (int)(sum_order == QRLSH_SUM_SEQUENTIAL);
    if (eligible)
      QR_LAUNCH("predict_users", predict_users_kernel<true>, grid, dim3(PU_THREADS), 0, st, ratings, nu, nq, q_off, q_idx,
                q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean, seq, users, m, slices, out,
                ostride);
    else
      QR_LAUNCH("predict_users", predict_users_kernel<false>, grid, dim3(PU_THREADS), 0, st, ratings, nu, nq, q_off, q_idx,
                q_milli, u_idx, u_val, (int)ku, query_weight, user_weight, default_mean, seq, users, m, slices, out,
                ostride);
  }
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}

QRLSH_EXPORT size_t qrlsh_predict_users_workspace_bytes(int64_t m, int64_t nq) {
  (void)m;
  (void)nq;
  return QrCarve(nullptr).bytes();   // nothing is taken: the sweep reads the lists where they are
}

QRLSH_EXPORT int qrlsh_predict_users(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                                     const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx,
                                     const double *u_val, int32_t ku, double query_weight, double user_weight,
                                     double default_mean, int32_t sum_order, const int32_t *users, int64_t m, int32_t *out,
                                     uint32_t *flags_out, void *workspace, size_t workspace_bytes, void *stream) {
  (void)workspace;
  (void)workspace_bytes;
  return qr_predict_users("qrlsh_predict_users", ratings, nu, nq, q_off, q_idx, q_milli, u_idx, u_val, ku, query_weight,
                          user_weight, default_mean, sum_order, users, m, false, out, nq, flags_out,
                          static_cast<hipStream_t>(stream));
}
