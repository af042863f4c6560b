// evalsides.h -- the one copy of what every consumer of a prediction shares (predict.hip, evaluate.hip, rankeval.hip,
// rankgrid.hip): numpy's pairwise sum, weighted_average, the two sides of a cell, the blend, the prediction of one
// cell, the length of a user's list, the byte staging of a user's row in LDS, the queue of a sweep's taken cells and
// the checks of a grid's cuts.  All four files are compiled with -ffp-contract=off (see the Makefile): float64 as the
// reference's Python computes it.
#pragma once
#include "common.h"

constexpr int PRED_MAXK = 64;  // longest neighbour list handled (K = round(log_1.5 n) <= 51 for n < 1e9)
constexpr int PR_MAXQ = 128 * 1024;   // longest row staged in LDS as bytes
// the geometry of predict_users_kernel (predict.hip), which rank_sweep_kernel (rankeval.hip) writes the same rows with
constexpr int PU_THREADS = 1024;
constexpr int PU_AUTO_GROUPS = 4096;   // column slices: about this many workgroups, at least PU_THREADS columns each

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

// The prediction of cell (i, j), in three parts, so that a grid sweep (evaluate_grid_kernel, rank_grid_sweep_kernel)
// computes a side once per list cut and the blend once per setting, with the arithmetic of this one copy.
// rating_at(q) = ratings[i][q] (LDS bytes or the row in memory).  An index outside the matrix is not gathered (flag bit
// 1 of predict_users_check_kernel).
// HELD = true (evaluation): the cell is rated and predicted as if ratings[i][j] were 0 -- its own rating is never part
// of either side (a list entry naming j itself, or a user list naming i, reads as 0: decided by the index, not by the
// rating), and a user-list entry >= nu is not gathered.  HELD = false (serving): the cell is unrated, so neither index
// test is made.  The tests of the user side are NOT given to serving: that would change its hot loop.
// ev_query_side: the query side over the first n entries of the list that starts at q_idx[lo] (n <= PRED_MAXK).
template <bool HELD, typename RatingAt>
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
        return HELD && q == j ? (int32_t)0 : rating_at(q);
      },
      [&](int k) { return (double)q_milli[lo + k] / 1000.0; });
}

// ev_user_side: the user side over the first mu entries of user i's list (ui / uv)
template <bool HELD>
__device__ static inline double ev_user_side(const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, int64_t i,
                                             int64_t j, const int32_t *__restrict__ ui, const double *__restrict__ uv,
                                             int mu, bool sequential) {
  return weighted_average(
      mu, sequential,
      [&](int k) {
        const int64_t u = ui[k];
        return HELD && (u >= nu || u == i) ? (int32_t)0 : ratings[u * nq + j];   // u >= 0 for k < mu
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

// the blend rounded as Python's round() does (half to even), for the callers that have no use for the branch
__device__ static inline int32_t ev_blend_round(double qp, double up, double qw, double uw, double dmean) {
  int branch;
  return (int32_t)rint(ev_blend(qp, up, qw, uw, dmean, branch));
}

// The three parts together, over the CSR lists (similarity = milli / 1000.0, a true division): the prediction of cell
// (i, j) of the row whose own neighbour list is ui / uv / mu.  A list longer than PRED_MAXK is not walked and an index
// outside the matrix is not gathered: the prediction is 0 (flagged by predict_users_check_kernel).  -> the prediction;
// branch as EvalStats::add takes it.  One copy, for predict_users_kernel and rank_sweep_kernel (HELD = false; nu and i
// are not looked at) and for evaluate_kernel and evaluate_cells_kernel (HELD = true).
template <bool HELD, typename RatingAt>
__device__ static inline int32_t ev_predict(const int32_t *__restrict__ ratings, int64_t nu, int64_t nq, int64_t i, int64_t j,
                                            const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx,
                                            const int32_t *__restrict__ q_milli, const int32_t *__restrict__ ui,
                                            const double *__restrict__ uv, int mu, double qw, double uw, double dmean,
                                            bool sequential, RatingAt rating_at, int &branch) {
  branch = 0;
  const int64_t lo = q_off[j], n64 = q_off[j + 1] - lo;
  if (n64 < 0 || n64 > PRED_MAXK) return 0;  // flagged (bit 0); never walked
  bool outside = false;
  const double qp = ev_query_side<HELD>(nq, j, lo, (int)n64, q_idx, q_milli, sequential, rating_at, outside);
  const double up = ev_user_side<HELD>(ratings, nu, nq, i, j, ui, uv, mu, sequential);
  const double r = ev_blend(qp, up, qw, uw, dmean, branch);
  return outside ? 0 : (int32_t)rint(r);
}

// the length of a user's own neighbour list: ku slots, -1 padded
__device__ static inline int ev_list_len(const int32_t *ui, int ku) {
  int m = 0;
  while (m < ku && ui[m] >= 0) ++m;
  return m;
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

// The queue of a sweep's taken cells (every thread of a THREADS-thread workgroup calls it).  The workgroup walks the
// columns [j0, j1) THREADS at a time; take(j, j < j1, value) says whether this thread's column is taken (never when it
// lies past j1), may set the value that travels with it, and may do the column's own side work.  The taken columns are
// queued in LDS in column order (block scan); whenever THREADS of them wait every thread consumes one, and what is
// left is drained at the end, so the lanes stay full however thin the taken cells are.  one(slot, j, value, active):
// slot = the cell's rank among the taken cells of [j0, j1); every thread is called at each drain, active = whether it
// holds a cell (j and value are 0 otherwise) -- a caller whose waves need not stay whole returns at once when it is not.
// j and value arrive already taken from the queue, so a caller never indexes the ring.  Callers: evaluate_kernel and
// evaluate_grid_kernel.  rank_sweep_kernel and rank_grid_sweep_kernel carry the same ring and barriers written out:
// through this function they measured slower (see there); a change to the protocol has to be made in all three places.
// queue_j / queue_v: LDS, EV_QUEUE_SLOTS<THREADS> words each (fewer than THREADS cells wait when up to THREADS more
// arrive); queue_v is the literal nullptr when no value travels.  wsum: the scan's LDS, THREADS / WAVE words.
template <int THREADS> constexpr int EV_QUEUE_SLOTS = 2 * THREADS;

template <int THREADS, typename QueueV, typename Take, typename One>
__device__ static inline void ev_cell_queue(int64_t j0, int64_t j1, int32_t *queue_j, QueueV queue_v, uint32_t *wsum,
                                            Take take, One one) {
  constexpr uint32_t MASK = EV_QUEUE_SLOTS<THREADS> - 1;
  constexpr bool VALUES = !std::is_null_pointer<QueueV>::value;   // by the type: a test of the pointer is not free
  const int t = threadIdx.x;
  uint32_t head = 0, tail = 0;  // uniform
  auto drain = [&](bool active) {
    int32_t j = 0, v = 0;
    if (active) {
      j = queue_j[(head + t) & MASK];
      if constexpr (VALUES) v = queue_v[(head + t) & MASK];
    }
    one(head + t, j, v, active);
  };
  for (int64_t base = j0; base < j1; base += THREADS) {
    const int64_t j = base + t;
    int32_t v = 0;
    const bool taken = take(j, j < j1, v);
    uint32_t total;
    const uint32_t pos = block_excl_scan<THREADS>(taken ? 1u : 0u, wsum, total);
    if (taken) {
      queue_j[(tail + pos) & MASK] = (int32_t)j;
      if constexpr (VALUES) queue_v[(tail + pos) & MASK] = v;
    }
    tail += total;
    if (tail - head >= (uint32_t)THREADS) {  // uniform
      __syncthreads();
      drain(true);
      head += THREADS;
    }
    // the next scan's first barrier stands between these reads of the queue and the writes that follow it
  }
  __syncthreads();
  drain((uint32_t)t < tail - head);
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

// The lists' flags (predict_users_check_kernel of predict.hip, launched from every file under the caller's label): bit 0 a
// list longer than PRED_MAXK, bit 1 an index outside [0, nq), bit 2 a user id outside [0, nu) (users may be NULL: no
// ids to check).  One thread per list and per id; nothing is launched when there is neither.  *flags is or-ed into.
void qr_lists_check(const char *label, const int64_t *q_off, const int32_t *q_idx, int64_t nq, const int32_t *users,
                    int64_t m, int64_t nu, uint32_t *flags, hipStream_t st);
