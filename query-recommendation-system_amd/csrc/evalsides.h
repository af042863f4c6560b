// evalsides.h -- the one copy of the prediction arithmetic that predict.hip and rankgrid.hip share: numpy's pairwise
// sum, weighted_average, the two sides of a cell, the blend, the byte staging of a user's row in LDS and the checks of
// a grid's cuts.  Both files are compiled with -ffp-contract=off (see the Makefile): float64 as the reference's Python
// computes it.
#pragma once
#include "common.h"

constexpr int PRED_MAXK = 64;  // longest neighbour list handled (K = round(log_1.5 n) <= 51 for n < 1e9)
constexpr int PR_MAXQ = 128 * 1024;   // longest row staged in LDS as bytes

struct Pairwise8 {
  // numpy's float64 pairwise_sum for n <= 128 (loops_utils.h.src), fed one element at a time: element t of n.
  // n < 8: plain running sum.  Otherwise elements [0, n - n % 8) go round-robin into 8 accumulators, which
  // are combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) when the first tail element (or the
  // end) arrives; tail elements are then added one by one.
  double r0, r1, r2, r3, r4, r5, r6, r7, res;
  int n, body, t;
  bool seq;
  __device__ void begin(int n_, bool sequential) {
    n = n_;
    seq = sequential || n_ < 8;
    body = n_ - (n_ % 8);
    t = 0;
    r0 = r1 = r2 = r3 = r4 = r5 = r6 = r7 = 0.0;
    res = 0.0;
  }
  __device__ void add(double v) {
    if (seq) {
      res += v;
    } else if (t < body) {
      const bool first = t < 8;
      switch (t & 7) {
        case 0: r0 = first ? v : r0 + v; break;
        case 1: r1 = first ? v : r1 + v; break;
        case 2: r2 = first ? v : r2 + v; break;
        case 3: r3 = first ? v : r3 + v; break;
        case 4: r4 = first ? v : r4 + v; break;
        case 5: r5 = first ? v : r5 + v; break;
        case 6: r6 = first ? v : r6 + v; break;
        default: r7 = first ? v : r7 + v; break;
      }
      if (t + 1 == body) res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    } else {
      res += v;
    }
    ++t;
  }
  // elements [k0, k0 + 8) of the list at once (k0 a multiple of 8; v[u] of elements past n are ignored): the
  // accumulator of element k0 + u is r<u>, known at compile time -- no per-element dispatch
  __device__ void add8(const double (&v)[8], int k0) {
    if (!seq && k0 < body) {   // a whole chunk of the round-robin part (body is a multiple of 8)
      if (k0 == 0) {
        r0 = v[0]; r1 = v[1]; r2 = v[2]; r3 = v[3]; r4 = v[4]; r5 = v[5]; r6 = v[6]; r7 = v[7];
      } else {
        r0 += v[0]; r1 += v[1]; r2 += v[2]; r3 += v[3]; r4 += v[4]; r5 += v[5]; r6 += v[6]; r7 += v[7];
      }
      if (k0 + 8 == body) res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < n) res += v[u];
    }
    t = k0 + 8;
  }
  __device__ double end() const { return res; }
};

// weighted_average (recommender.py:36-47) over a neighbour list of n entries: rating(k) = the user's / query's
// rating of neighbour k, sim(k) its similarity.  RatingAt / SimAt are callables (gathers).
template <typename RatingAt, typename SimAt>
__device__ static inline double weighted_average(int n, bool sequential, RatingAt rating, SimAt sim) {
  if (n == 0) return 0.0;
  Pairwise8 prod;
  prod.begin(n, sequential);
  unsigned long long nz = 0;
  // eight neighbours at a time: their list entries, then their ratings, are independent loads in flight together
  // (a dependent index -> rating round trip per neighbour otherwise); the additions keep the list order
  for (int k0 = 0; k0 < n; k0 += 8) {
    int32_t r[8];
    double sv[8], pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      r[u] = 0;
      sv[u] = 0.0;
      if (k0 + u < n) {
        sv[u] = sim(k0 + u);
        r[u] = rating(k0 + u);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      pv[u] = (double)r[u] * sv[u];
      if (r[u] != 0) nz |= 1ull << (k0 + u);   // r[u] = 0 past the end
    }
    prod.add8(pv, k0);
  }
  // the weights of the rated neighbours, in list order, eight at a time as well
  Pairwise8 w;
  const int m = __popcll(nz);
  w.begin(m, sequential);
  for (int k0 = 0; k0 < m; k0 += 8) {
    double wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      wv[u] = 0.0;
      if (nz) {
        wv[u] = sim(__ffsll((long long)nz) - 1);
        nz &= nz - 1;
      }
    }
    w.add8(wv, k0);
  }
  const double wsum = w.end();
  if (wsum == 0.0) return 0.0;
  return prod.end() / wsum;
}

// The prediction of cell (i, j) as if ratings[i][j] were 0, in three parts, so that a grid sweep (evaluate_grid_kernel,
// rank_grid_sweep_kernel) computes a side once per list cut and the blend once per setting, with the arithmetic of
// this one copy.  The cell's own rating is never part of either side (a list entry naming j itself, or a user list
// naming i, reads as 0 -- decided by the index, not by the rating).  rating_at(q) = ratings[i][q] (LDS bytes or the
// row in memory).  An index outside the matrix is not gathered (flag bit 1 of predict_users_check_kernel).
// ev_query_side: the query side over the first n entries of the list that starts at q_idx[lo] (n <= PRED_MAXK).
template <typename RatingAt>
__device__ static inline double ev_query_side(int64_t nq, int64_t j, int64_t lo, int n,
                                              const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli,
                                              bool sequential, RatingAt rating_at, bool &outside) {
  return weighted_average(
      n, sequential,
      [&](int k) {
        const int32_t q = q_idx[lo + k];
        if ((uint32_t)q >= (uint32_t)nq) {  // flagged (bit 1); never gathered
          outside = true;
          return (int32_t)0;
        }
        return q == j ? (int32_t)0 : rating_at(q);
      },
      [&](int k) { return (double)q_milli[lo + k] / 1000.0; });
}

// ev_user_side: the user side over the first mu entries of user i's list (ui / uv)
__device__ static inline double ev_user_side(const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, int64_t i,
                                             int64_t j, const int32_t *__restrict__ ui, const double *__restrict__ uv,
                                             int mu, bool sequential) {
  return weighted_average(
      mu, sequential,
      [&](int k) {
        const int64_t u = ui[k];
        return (u >= nu || u == i) ? (int32_t)0 : ratings[u * nq + j];   // u >= 0 for k < mu
      },
      [&](int k) { return uv[k]; });
}

// ev_blend: recommender.py:324-331 in the reference's operand order, before rounding; branch as EvalStats::add takes it
__device__ static inline double ev_blend(double qp, double up, double qw, double uw, double dmean, int &branch) {
  double r;
  if (up == 0.0 && qp == 0.0) r = 0.0;
  else if (up == 0.0) r = qp * (qw + (uw * 0.5)) + dmean * (uw * 0.5);
  else if (qp == 0.0) r = up * (uw + (qw * 0.5)) + dmean * (qw * 0.5);
  else r = qp * qw + up * uw;
  branch = up == 0.0 ? 0 : (qp == 0.0 ? 1 : 2);
  return r;
}

// The byte staging of one user's row (every thread of a THREADS-thread workgroup calls it; nq <= PR_MAXQ): lrow[j] =
// (uint8_t)row[j], and -> whether every value fits a byte, i.e. whether the gathers may read lrow instead of the row.
// *wide is an LDS word of the caller.  Two barriers; the second stands behind the last write of lrow.
template <int THREADS>
__device__ static inline bool ev_stage_row(const int32_t *__restrict__ row, int64_t nq, uint8_t *lrow, int *wide) {
  if (threadIdx.x == 0) *wide = 0;
  __syncthreads();
  bool bad = false;
  for (int64_t j = threadIdx.x; j < nq; j += THREADS) {
    const int32_t v = row[j];
    bad |= (v < 0) | (v > 255);
    lrow[j] = (uint8_t)v;
  }
  if (bad) *wide = 1;
  __syncthreads();
  return *wide == 0;
}

// ---- a grid's cuts (qrlsh_evaluate_grid, qrlsh_evaluate_ranking_grid) ----
__device__ static inline double eg_pick(const double (&a)[QRLSH_GRID_MAX_CUTS], int c) {   // c uniform; no indexed array
  return c == 0 ? a[0] : (c == 1 ? a[1] : (c == 2 ? a[2] : a[3]));
}

// flag bit 3: a negative cut (threads 0 .. 7 of one workgroup look at one cut each)
__device__ static inline void eg_check_cuts(int t, const int32_t *__restrict__ q_cuts, int ncq,
                                            const int32_t *__restrict__ u_cuts, int ncu, uint32_t *__restrict__ flags) {
  bool bad = false;
  if (t < QRLSH_GRID_MAX_CUTS) bad = t < ncq && q_cuts[t] < 0;
  else if (t < 2 * QRLSH_GRID_MAX_CUTS) bad = t - QRLSH_GRID_MAX_CUTS < ncu && u_cuts[t - QRLSH_GRID_MAX_CUTS] < 0;
  if (bad) atomicOr(flags, 8u);
}

// The lists' flags, launched from either file (predict.hip): bit 0 a list longer than PRED_MAXK, bit 1 an index outside
// [0, nq), bit 2 a user id outside [0, nu) (users may be NULL with m = 0: no ids to check).  *flags is or-ed into.
int qr_lists_check(const char *label, const int64_t *q_off, const int32_t *q_idx, int64_t nq, const int32_t *users,
                   int64_t m, int64_t nu, uint32_t *flags, hipStream_t st);
