// predict.hip -- N1: the hybrid prediction loop (consumer of the hot path's output).
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
#include "evalsides.h"   // PRED_MAXK, weighted_average, the sides and the blend: shared with rankgrid.hip

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
  int m = 0;
  while (m < ku && ui[m] >= 0) ++m;
  const double up = weighted_average(
      m, sequential != 0, [&](int k) { return ratings[(int64_t)ui[k] * nq + j]; }, [&](int k) { return uv[k]; });
  double r;
  if (up == 0.0 && qp == 0.0) r = 0.0;
  else if (up == 0.0) r = qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5);
  else if (qp == 0.0) r = up * (uw + (qw * 0.5)) + dmean * (qw * 0.5);
  else r = qp * qw + up * uw;
  out[cell] = (int32_t)rint(r);
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
  if (t == 0) wide = 0;
  __syncthreads();
  bool bad = false;
  for (int64_t j = t; j < nq; j += PR_THREADS) {
    const int32_t v = row[j];
    bad |= (v < 0) | (v > 255);
    lrow[j] = (uint8_t)v;
  }
  if (bad) wide = 1;
  __syncthreads();
  const bool in_lds = wide == 0;  // uniform
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  int m = 0;
  while (m < ku && ui[m] >= 0) ++m;  // uniform: the user's own neighbour list
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
    double r;
    if (up == 0.0 && qp == 0.0) r = 0.0;
    else if (up == 0.0) r = qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5);
    else if (qp == 0.0) r = up * (uw + (qw * 0.5)) + dmean * (qw * 0.5);
    else r = qp * qw + up * uw;
    out[cell] = (int32_t)rint(r);
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
      int m = 0;
      while (m < ku && uidx[lane][m] >= 0) ++m;
      const double up = weighted_average(
          m, sequential != 0, [&](int k) { return (int32_t)rj[uidx[lane][k]]; }, [&](int k) { return uval[lane][k]; });
      double r;
      if (up == 0.0 && qp == 0.0) r = 0.0;
      else if (up == 0.0) r = qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5);
      else if (qp == 0.0) r = up * (uw + (qw * 0.5)) + dmean * (qw * 0.5);
      else r = qp * qw + up * uw;
      res = (int32_t)rint(r);
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
QRLSH_EXPORT size_t qrlsh_predict_workspace_bytes(int64_t nu, int64_t nq, int32_t kq) {
  if (nu <= 0 || nq <= 0 || kq <= 0) return 0;
  return (size_t)kq * (size_t)nq * (sizeof(double) + sizeof(int32_t)) + 16 + (size_t)nq * (size_t)pt_stride(nu);
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
  if (hipMemsetAsync(too_long_out, 0, sizeof(uint32_t), st) != hipSuccess) {
    qrlsh_set_error("qrlsh_predict: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
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
  double *val_t = static_cast<double *>(workspace);
  int32_t *idx_t = reinterpret_cast<int32_t *>(val_t + (size_t)kq * nq);
  uint32_t *wide = reinterpret_cast<uint32_t *>(idx_t + (size_t)kq * nq);   // 4-byte aligned; 16 bytes reserved
  uint8_t *rt = reinterpret_cast<uint8_t *>(wide) + 16;
  const bool tile = ku <= PT_MAXKU && ceil_div64(nq, PT_QUERIES) <= 2147483647ll && ceil_div64(nu, PT_USERS) <= 65535 &&
                    ceil_div64(nu, 64) <= 65535;
  const bool row = nq <= PR_MAXQ && nu <= 65535;
  if (tile) {
    // tile form; the row (or cell) form follows and does nothing unless a rating did not fit a byte
    const int64_t nus = pt_stride(nu);
    if (hipMemsetAsync(wide, 0, 16, st) != hipSuccess) {
      qrlsh_set_error("qrlsh_predict: hipMemsetAsync failed");
      return QRLSH_EHIP;
    }
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
// x's list) -- predict_kernel's expression with up = 0.  One workgroup per (new query, block of 256 users): the list
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
  const double r = qp == 0.0 ? 0.0 : qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5);
  out[x * nu + u] = (int32_t)rint(r);
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
  if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), st) != hipSuccess) {
    qrlsh_set_error("qrlsh_predict_columns: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
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
constexpr int PU_THREADS = 1024;
constexpr int PU_AUTO_GROUPS = 4096;   // column slices: about this many workgroups, at least PU_THREADS columns each

// The serving prediction of the unrated cell (row, j): the two weighted averages and the blend.  rating_at(q) = the
// row's rating of query q (LDS bytes or the row in memory); ui / uv / mu = the row's own neighbour list.  One copy, for
// predict_users_kernel and rank_sweep_kernel.
template <typename RatingAt>
__device__ static inline int32_t pu_predict(const int32_t *__restrict__ ratings, int64_t nq, int64_t j,
                                            const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx,
                                            const int32_t *__restrict__ q_milli, const int32_t *__restrict__ ui,
                                            const double *__restrict__ uv, int mu, double qw, double uw, double dmean,
                                            bool sequential, RatingAt rating_at) {
  const int64_t lo = q_off[j], n64 = q_off[j + 1] - lo;
  if (n64 < 0 || n64 > PRED_MAXK) return 0;  // flagged (bit 0); never walked
  bool outside = false;
  const double qp = weighted_average(
      (int)n64, sequential,
      [&](int k) {
        const int32_t q = q_idx[lo + k];
        if ((uint32_t)q >= (uint32_t)nq) {  // flagged (bit 1); never gathered
          outside = true;
          return (int32_t)0;
        }
        return rating_at(q);
      },
      [&](int k) { return (double)q_milli[lo + k] / 1000.0; });
  const double up = weighted_average(
      mu, sequential, [&](int k) { return ratings[(int64_t)ui[k] * nq + j]; }, [&](int k) { return uv[k]; });
  double r;
  if (up == 0.0 && qp == 0.0) r = 0.0;
  else if (up == 0.0) r = qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5);
  else if (qp == 0.0) r = up * (uw + (qw * 0.5)) + dmean * (qw * 0.5);
  else r = qp * qw + up * uw;
  return outside ? 0 : (int32_t)rint(r);
}

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
  int mu = 0;
  while (mu < ku && ui[mu] >= 0) ++mu;  // uniform: the user's own neighbour list
  for (int64_t j = j0 + t; j < j1; j += PU_THREADS) {
    const int32_t own = in_lds ? (int32_t)lrow[j] : row[j];
    if (own != 0) {
      orow[j] = ELIGIBLE ? 0 : own;
      continue;
    }
    orow[j] = pu_predict(ratings, nq, j, q_off, q_idx, q_milli, ui, uv, mu, qw, uw, dmean, sequential != 0,
                         [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; });
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

int qr_lists_check(const char *label, const int64_t *q_off, const int32_t *q_idx, int64_t nq, const int32_t *users,
                   int64_t m, int64_t nu, uint32_t *flags, hipStream_t st) {
  const int64_t checks = nq > m ? nq : m;
  if (checks > 0)
    QR_LAUNCH(label, predict_users_check_kernel, dim3((unsigned)ceil_div64(checks, 256)), dim3(256), 0, st, q_off, q_idx,
              nq, users, users ? m : (int64_t)0, nu, flags);
  return QRLSH_OK;
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
  if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), st) != hipSuccess) {
    qrlsh_set_error("%s: hipMemsetAsync failed", who);
    return QRLSH_EHIP;
  }
  const int64_t checks = nq > m ? nq : m;
  QR_LAUNCH("predict_users_check", predict_users_check_kernel, dim3((unsigned)ceil_div64(checks, 256)), dim3(256), 0, st,
            q_off, q_idx, nq, users, m, nu, flags_out);
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
  return 0;   // the sweep reads the lists where they are
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

// ---- evaluation: the prediction error on rated cells (qrlsh_ratings_holdout, qrlsh_evaluate, qrlsh_evaluate_cells) ----
// The blend of cell (i, j) reads the user's ratings of j's neighbour queries and the neighbour users' ratings of j, never
// ratings[i][j] itself.  So a RATED cell can be predicted as if it were unrated -- predict_users_kernel's computation over
// the complement of the cells it fills -- and compared with its rating.  Predictions and ratings are integers: every
// statistic is an exact integer sum and the result cannot depend on the launch order.
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

// The prediction of cell (i, j) as if ratings[i][j] were 0: predict_users_kernel's two weighted averages and blend.  The
// cell's own rating is never part of either side (a list entry naming j itself, or a user list naming i, reads as 0 --
// decided by the index, not by the rating).  rating_at(q) = ratings[i][q] (LDS bytes or the row in memory).  A list
// longer than PRED_MAXK is not walked and an index outside the matrix is not gathered: the prediction is 0 (flagged by
// predict_users_check_kernel).  -> the prediction; branch as EvalStats::add takes it.
// The two sides and the blend (ev_query_side, ev_user_side, ev_blend) are separate and live in evalsides.h, so that the
// grid sweeps compute a side once per list cut and the blend once per setting, with the arithmetic of that one copy.
template <typename RatingAt>
__device__ static inline int32_t ev_predict(const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, int64_t i, int64_t j,
                                            const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx,
                                            const int32_t *__restrict__ q_milli, const int32_t *__restrict__ ui,
                                            const double *__restrict__ uv, int mu, double qw, double uw, double dmean,
                                            bool sequential, RatingAt rating_at, int &branch) {
  branch = 0;
  const int64_t lo = q_off[j], n64 = q_off[j + 1] - lo;
  if (n64 < 0 || n64 > PRED_MAXK) return 0;  // flagged (bit 0); never walked
  bool outside = false;
  const double qp = ev_query_side(nq, j, lo, (int)n64, q_idx, q_milli, sequential, rating_at, outside);
  const double up = ev_user_side(ratings, nu, nq, i, j, ui, uv, mu, sequential);
  const double r = ev_blend(qp, up, qw, uw, dmean, branch);
  return outside ? 0 : (int32_t)rint(r);
}

// The sweep: one workgroup per (column slice, user), the users of a slice together, the user's row of `ratings` staged in
// LDS as bytes where it fits (predict_users_kernel's two forms).  The workgroup reads its slice of `truth` coalesced,
// 1024 columns at a time, and queues the evaluated cells (truth != 0 and kept) in LDS; whenever 1024 are queued every
// thread predicts one, so the lanes stay full however thin the sample is.  Each thread keeps its 14 sums in registers;
// the workgroup's sums go to part[user][slice][16] (summed by evaluate_finish_kernel: no atomics, no order).
constexpr int EV_THREADS = 1024;
constexpr int EV_QUEUE = 2 * EV_THREADS;   // fewer than EV_THREADS cells wait when up to EV_THREADS more arrive
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
  __shared__ int32_t queue_j[EV_QUEUE];
  __shared__ int32_t queue_v[EV_QUEUE];
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
  int mu = 0;
  while (mu < ku && ui[mu] >= 0) ++mu;  // uniform: the user's own neighbour list
  EvalStats st;
  st.clear();
  auto one = [&](uint32_t slot) {
    const int64_t j = queue_j[slot & (EV_QUEUE - 1)];
    const int32_t tv = queue_v[slot & (EV_QUEUE - 1)];
    int branch;
    const int32_t pred = ev_predict(
        ratings, nu, nq, i, j, q_off, q_idx, q_milli, ui, uv, mu, qw, uw, dmean, sequential != 0,
        [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; }, branch);
    st.add(pred, branch, tv);
    if (pred_out) pred_out[i * nq + j] = pred;
  };
  uint32_t head = 0, tail = 0;  // uniform
  for (int64_t base = j0; base < j1; base += EV_THREADS) {
    const int64_t j = base + t;
    int32_t tv = 0;
    if (j < j1) tv = trow[j];
    const bool take = tv != 0 && ev_kept(seed, keep, i, j);
    if (pred_out && j < j1 && !take) pred_out[i * nq + j] = -1;
    uint32_t total;
    const uint32_t pos = block_excl_scan<EV_THREADS>(take ? 1u : 0u, wsum, total);
    if (take) {
      queue_j[(tail + pos) & (EV_QUEUE - 1)] = (int32_t)j;
      queue_v[(tail + pos) & (EV_QUEUE - 1)] = tv;
    }
    tail += total;
    if (tail - head >= (uint32_t)EV_THREADS) {  // uniform
      __syncthreads();
      one(head + t);
      head += EV_THREADS;
    }
    // the next scan's first barrier stands between these reads of the queue and the writes that follow it
  }
  __syncthreads();
  if ((uint32_t)t < tail - head) one(head + t);
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
QRLSH_EXPORT size_t qrlsh_evaluate_workspace_bytes(int64_t nu, int64_t nq) {
  if (nu <= 0 || nq <= 0) return 0;
  return ((size_t)nu * (size_t)ev_slices(nu, nq) + (size_t)ceil_div64(nu, EVF_USERS)) * 16 * sizeof(long long);
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
  if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), st) != hipSuccess ||
      (empty && hipMemsetAsync(totals_out, 0, 16 * sizeof(int64_t), st) != hipSuccess) ||
      (empty && nu > 0 && hipMemsetAsync(per_user_out, 0, (size_t)nu * 16 * sizeof(int64_t), st) != hipSuccess)) {
    qrlsh_set_error("qrlsh_evaluate: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
  if (empty) return QRLSH_OK;
  const int64_t slices = ev_slices(nu, nq), groups = ceil_div64(nu, EVF_USERS);
  if (nu * slices > 2147483647ll) {
    qrlsh_set_error("qrlsh_evaluate: nu=%lld x %lld slices above 2^31 - 1 workgroups", (long long)nu, (long long)slices);
    return QRLSH_EUNSUPPORTED;
  }
  long long *part = static_cast<long long *>(workspace);
  long long *gpart = part + (size_t)nu * slices * 16;
  QR_LAUNCH("evaluate_check", predict_users_check_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, st, q_off,
            q_idx, nq, (const int32_t *)nullptr, (int64_t)0, nu, flags_out);   // the lists' two flags
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
  __shared__ int32_t queue_j[EV_QUEUE];
  __shared__ int32_t queue_v[EV_QUEUE];
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
  int mu = 0;
  while (mu < ku && ui[mu] >= 0) ++mu;  // uniform: the user's own neighbour list
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
  auto one = [&](uint32_t slot, bool active) {
    const unsigned long long act = __ballot(active);
    if (act == 0) return;  // wave-uniform
    cells += (unsigned long long)__popcll(act);
    double qp[QRLSH_GRID_MAX_CUTS] = {0.0, 0.0, 0.0, 0.0}, up[QRLSH_GRID_MAX_CUTS] = {0.0, 0.0, 0.0, 0.0};
    int32_t tv = 0;
    if (active) {
      const int64_t j = queue_j[slot & (EV_QUEUE - 1)];
      tv = queue_v[slot & (EV_QUEUE - 1)];
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
              qp[c] = ev_query_side(
                  nq, j, lo, n, q_idx, q_milli, seq, [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; },
                  outside);
            last = n;
          }
        }
#pragma unroll
        for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
          if (c < ncu) {
            if (c > 0 && um[c] == um[c - 1]) up[c] = up[c - 1];  // uniform
            else up[c] = ev_user_side(ratings, nu, nq, i, j, ui, uv, um[c], seq);
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
  uint32_t head = 0, tail = 0;  // uniform
  for (int64_t base = j0; base < j1; base += EV_THREADS) {
    const int64_t j = base + t;
    int32_t tv = 0;
    if (j < j1) tv = trow[j];
    const bool take = tv != 0 && ev_kept(seed, keep, i, j);
    uint32_t total;
    const uint32_t pos = block_excl_scan<EV_THREADS>(take ? 1u : 0u, wsum, total);
    if (take) {
      queue_j[(tail + pos) & (EV_QUEUE - 1)] = (int32_t)j;
      queue_v[(tail + pos) & (EV_QUEUE - 1)] = tv;
    }
    tail += total;
    if (tail - head >= (uint32_t)EV_THREADS) {  // uniform
      __syncthreads();
      one(head + t, true);
      head += EV_THREADS;
    }
    // the next scan's first barrier stands between these reads of the queue and the writes that follow it
  }
  __syncthreads();
  one(head + t, (uint32_t)t < tail - head);
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
  return ((size_t)nu * (size_t)ev_slices(nu, nq) + (size_t)ceil_div64(nu, EGF_USERS)) * (size_t)settings * EG_WORDS *
         sizeof(long long);
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
    QR_CHECK_ARG((uintptr_t)workspace % 8 == 0, "%s: the workspace must be 8-byte aligned", who);
    if (!workspace || workspace_bytes < need) {
      qrlsh_set_error("%s: needs %zu workspace bytes, got %zu", who, need, workspace ? workspace_bytes : 0);
      return QRLSH_EWORKSPACE;
    }
  }
  const int64_t slices = ev_slices(nu, nq), groups = ceil_div64(nu, EGF_USERS);
  if (!empty && nu * slices > 2147483647ll) {
    qrlsh_set_error("%s: nu=%lld x %lld slices above 2^31 - 1 workgroups", who, (long long)nu, (long long)slices);
    return QRLSH_EUNSUPPORTED;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), st) != hipSuccess ||
      (empty && hipMemsetAsync(totals_out, 0, (size_t)words * sizeof(int64_t), st) != hipSuccess) ||
      (empty && nu > 0 && per_user_out &&
       hipMemsetAsync(per_user_out, 0, (size_t)nu * words * sizeof(int64_t), st) != hipSuccess)) {
    qrlsh_set_error("%s: hipMemsetAsync failed", who);
    return QRLSH_EHIP;
  }
  if (empty) {
    QR_LAUNCH("evaluate_grid_cuts", evaluate_grid_cuts_kernel, dim3(1), dim3(64), 0, st, q_cuts, (int)ncq, u_cuts,
              (int)ncu, flags_out);
    QR_LAUNCH_CHECK(who);
    return QRLSH_OK;
  }
  long long *part = static_cast<long long *>(workspace);
  long long *gpart = part + (size_t)nu * slices * words;
  const unsigned fin_threads = (unsigned)((words + WAVE - 1) / WAVE * WAVE);
  QR_LAUNCH("evaluate_check", predict_users_check_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, st, q_off,
            q_idx, nq, (const int32_t *)nullptr, (int64_t)0, nu, flags_out);   // the lists' two flags
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
      int mu = 0;
      while (mu < ku && ui[mu] >= 0) ++mu;
      int branch;
      const int32_t pred = ev_predict(
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
  if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), st) != hipSuccess ||
      hipMemsetAsync(totals_out, 0, 16 * sizeof(int64_t), st) != hipSuccess) {
    qrlsh_set_error("qrlsh_evaluate_cells: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
  if (m == 0) return QRLSH_OK;
  if (nq > 0)
    QR_LAUNCH("evaluate_check", predict_users_check_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, st, q_off,
              q_idx, nq, (const int32_t *)nullptr, (int64_t)0, nu, flags_out);   // the lists' two flags; ids: below
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
  if (hipMemsetAsync(count_out, 0, sizeof(int64_t), st) != hipSuccess) {
    qrlsh_set_error("qrlsh_ratings_holdout: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
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

// ---- ranking evaluation: is what the user would like in the list the user is shown? (qrlsh_evaluate_ranking) -----------
// Hold-out only.  `train` = the matrix with the test cells zeroed, `truth` = the full one.  A TEST cell of user u:
// train[u][j] == 0 && truth[u][j] != 0; it is RELEVANT when truth[u][j] >= relevant.  The user's list is
// qrlsh_recommend_users' over `train`: a test cell is 0 there, so the serving arithmetic (pu_predict) is its hold-out
// prediction.  Three steps: rank_sweep_kernel writes the compact eligible-mode rows and counts the test cells,
// rc_select<true> (recommend.hip, through qr_select_compact) ranks them, rank_score_kernel holds the lists to the truth.
// Everything counted is an integer: exact, and independent of the launch order.
//
// The sweep: predict_users_kernel's geometry and two row forms.  HELDOUT = false: every unrated cell of `train` is
// predicted -- predict_users_kernel<true>'s rows, word for word.  true: only the test cells are candidates; they are
// queued in LDS as evaluate_kernel queues its cells (block scan over 1024 columns, 1024 predicted whenever 1024 wait), so
// the lanes stay full when 1 % of the row is held out, and every other word of the slice is written 0.  In the same pass
// the workgroup counts its slice's test cells and relevant test cells -- also those the model cannot reach (prediction 0)
// -- into part[request][slice][2] (word 0 test cells, word 1 relevant ones).
constexpr int RK_THREADS = PU_THREADS;
constexpr int RK_QUEUE = 2 * RK_THREADS;   // fewer than RK_THREADS cells wait when up to RK_THREADS more arrive

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
  __shared__ int32_t queue_j[HELDOUT ? RK_QUEUE : 1];
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
  int mu = 0;
  while (mu < ku && ui[mu] >= 0) ++mu;  // uniform: the user's own neighbour list
  auto predict = [&](int64_t j) {
    return pu_predict(train, nq, j, q_off, q_idx, q_milli, ui, uv, mu, qw, uw, dmean, sequential != 0,
                      [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; });
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
QRLSH_EXPORT size_t qrlsh_evaluate_ranking_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices) {
  if (m <= 0 || nq <= 0) return 0;
  size_t rows = 0, select = 0;
  if (qr_select_compact_plan("qrlsh_evaluate_ranking_workspace_bytes", m, nq, k, slices, &rows, &select) != QRLSH_OK)
    return 0;
  const size_t part = (size_t)m * (size_t)rk_sweep_slices(m, nq, slices) * 2 * sizeof(long long);
  return rows + select + (part + 255) / 256 * 256;
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
    QR_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "%s: the workspace must be 16-byte aligned", who);
    if (!workspace || workspace_bytes < need) {
      qrlsh_set_error("%s: needs %zu workspace bytes, got %zu", who, need, workspace ? workspace_bytes : 0);
      return QRLSH_EWORKSPACE;
    }
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(flags_out, 0, sizeof(uint32_t), st) != hipSuccess ||
      hipMemsetAsync(totals_out, 0, 16 * sizeof(int64_t), st) != hipSuccess) {
    qrlsh_set_error("%s: hipMemsetAsync failed", who);
    return QRLSH_EHIP;
  }
  if (m == 0) return QRLSH_OK;
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  int32_t *rows = reinterpret_cast<int32_t *>(ws);
  long long *part = reinterpret_cast<long long *>(ws + rows_bytes + select_bytes);
  const int64_t checks = nq > m ? nq : m;
  QR_LAUNCH("rank_check", predict_users_check_kernel, dim3((unsigned)ceil_div64(checks, 256)), dim3(256), 0, st, q_off,
            q_idx, nq, users, m, nu, flags_out);
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
                                   ws + rows_bytes, st);
  if (rs != QRLSH_OK) return rs;
  QR_LAUNCH("rank_score", rank_score_kernel, dim3((unsigned)ceil_div64(m, RS_WAVES)), dim3(RS_WAVES * WAVE), 0, st, truth,
            nu, nq, users, m, (int)k, relevant, (const int32_t *)idx_out, (const int32_t *)avail_out,
            reinterpret_cast<const long long *>(gain), reinterpret_cast<const long long *>(gain_prefix),
            (const long long *)part, S, reinterpret_cast<long long *>(per_user_out),
            reinterpret_cast<unsigned long long *>(totals_out), flags_out);
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}
