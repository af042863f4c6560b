// userlists.hip -- the user-similarity lists stay exact when users rate queries: no re-clustering, no full recompute.
//
// The lists of qrlsh/users.py only ever name users of one cluster, so a batch of rating edits that touches the rows R
// can change the lists of R's clusters only.  With the cluster labels and K held fixed (as K is on the query side,
// replace.hip) the update is exact:
//   a row shorter than K was never cut: it holds every positive neighbour.  A row of exactly K entries that loses
//   none of them can only be pushed by new values -- the candidates its cut threw away are unchanged and still rank
//   below it.  Only a FULL row that names a changed user may need what the cut threw away: mark picks those rows, and
//   they are scored against their whole cluster like the changed rows themselves (S = R + picked).  Every other row
//   of a touched cluster is the first K of the merge of its stored entries outside R with the new scores of its
//   cluster's changed users; ties go by id both ways.
//
//   ratings_set    the cell edits, one lane per cell
//   rows_stats     mean (float64) and squared norm (int64) of the truncated centred row, one workgroup per row
//   pairs_score    the hot kernel: few pairs of very long rows.  Grid = (column slice, tile of US_TP consecutive pairs);
//                  a run of pairs with the same first row centres that row's slice once into LDS and streams the other
//                  rows past it, centring them in registers: nothing centred is ever written to memory.  16-byte
//                  loads on the address's own alignment (a row starts wherever row * nq lands), scalar head and tail.
//                  Exact integer partial dots go to [slice][pair]; a finish kernel sums them (any order: integers)
//                  and ends with the score kernels' own float64 expression.
//   cluster_pairs  count / fill: (S[x], v) for every other member v of S[x]'s cluster in member order, so the slot of
//                  (row, member) is off[x] + pos(v) - (pos(v) > pos(row)): nobody searches.
//   lists_mark     one lane per stored entry; a picked row enters the pick map once and adds its pair count.
//   lists_apply    one wave per row of a touched cluster: the best K (K <= 64: one per lane) of any number of
//                  candidates, taken in chunks of 64 that are ranked against the best so far.
#include "userlists.h"

constexpr int US_THREADS = 256;
constexpr int US_TP = 8;             // pairs per tile
constexpr int US_MAXCOLS = 4096;     // columns per slice at most (the first row's centred slice: 16 KB of LDS)
constexpr int US_MINCOLS = 256;
constexpr int US_VPT = US_MAXCOLS / 4 / US_THREADS;   // 16-byte vectors per lane and row slice (4)
constexpr int US_WANT_WG = 2048;     // workgroups wanted before slices stop shrinking (256 CUs x 8)

// ---- the cell edits ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(US_THREADS) void ratings_set_kernel(int32_t *__restrict__ ratings, int64_t nu, int64_t nq,
                                                                const uint32_t *__restrict__ users,
                                                                const uint32_t *__restrict__ queries,
                                                                const int32_t *__restrict__ values, int64_t m,
                                                                uint32_t *__restrict__ flag) {
  bool wrong = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = users[i], q = queries[i];
    if (u >= nu || q >= nq) wrong = true;
    else ratings[u * nq + q] = values[i];
  }
  if (__ballot(wrong) && lane_id() == 0) atomicOr(flag, 1u);
}

QRLSH_EXPORT int qrlsh_ratings_set(int32_t *ratings, int64_t nu, int64_t nq, const uint32_t *users,
                                   const uint32_t *queries, const int32_t *values, int64_t m, uint32_t *flag_out,
                                   void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && m >= 0 && nu < (1ll << 31) && nq < (1ll << 31),
               "qrlsh_ratings_set: bad sizes nu=%lld nq=%lld m=%lld", (long long)nu, (long long)nq, (long long)m);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(ratings && users && queries && values && flag_out, "qrlsh_ratings_set: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_ratings_set", flag_out, 0, sizeof(uint32_t), st);
  QR_LAUNCH("ratings_set", ratings_set_kernel, dim3(rm_grid(m, US_THREADS)), dim3(US_THREADS), 0, st, ratings, nu, nq,
            users, queries, values, m, flag_out);
  QR_LAUNCH_CHECK("qrlsh_ratings_set");
  return QRLSH_OK;
}

// ---- mean and squared norm of chosen rows -----------------------------------------------------------------------------
// 1024 lanes walk the row twice (sum and count, then the centred squares: the row is in L2 by then) in 16-byte vectors
// on the row's own alignment, four loads in flight per lane; the scalars before and behind go to lanes 0 .. 2, 64 .. 66
constexpr int UST_THREADS = 1024;

template <typename F> __device__ static inline void us_walk_row(const int32_t *row, int64_t elem0, int64_t nq, F f) {
  const int t = threadIdx.x;
  const int64_t h = (4 - (elem0 & 3)) & 3, head = h < nq ? h : nq, nvec = (nq - head) >> 2, tail0 = head + 4 * nvec;
  if (t < head) f(row[t]);
  if (t >= WAVE && t - WAVE < nq - tail0) f(row[tail0 + t - WAVE]);
  const us_i32x4 *v = reinterpret_cast<const us_i32x4 *>(row + head);
  for (int64_t i0 = 0; i0 < nvec; i0 += 4 * UST_THREADS) {
    us_i32x4 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = i0 + t + j * UST_THREADS;
      x[j] = i < nvec ? v[i] : us_i32x4{0, 0, 0, 0};   // zeros add nothing to either pass
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) f(x[j].x), f(x[j].y), f(x[j].z), f(x[j].w);
  }
}

// all lanes call it; every lane gets the workgroup's two sums (exact integers: any order).  s: 2 * 16 words of LDS.
__device__ static inline void us_block_sum2(int64_t &a, int64_t &b, int64_t *s) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) {
    a += __shfl_xor(a, m, WAVE);
    b += __shfl_xor(b, m, WAVE);
  }
  __syncthreads();   // s may still be read from an earlier call
  if (lane == 0) {
    s[w] = a;
    s[16 + w] = b;
  }
  __syncthreads();
  a = b = 0;
#pragma unroll
  for (int i = 0; i < UST_THREADS / WAVE; ++i) {
    a += s[i];
    b += s[16 + i];
  }
}

__global__ __launch_bounds__(UST_THREADS) void user_rows_stats_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                     int64_t nq, const uint32_t *__restrict__ rows,
                                                                     double *__restrict__ mean_out,
                                                                     int64_t *__restrict__ norm2_out) {
  __shared__ int64_t s[32];
  const int64_t u = rows ? (int64_t)rows[blockIdx.x] : (int64_t)blockIdx.x;
  if (u >= nu) return;   // uniform
  const int32_t *row = ratings + u * nq;
  int64_t sum = 0, cnt = 0;
  us_walk_row(row, u * nq, nq, [&](int32_t x) {
    sum += x;
    cnt += x != 0;
  });
  us_block_sum2(sum, cnt, s);
  const double mean = cnt ? (double)sum / (double)cnt : 0.0;
  int64_t n2 = 0, unused = 0;
  us_walk_row(row, u * nq, nq, [&](int32_t x) {
    const int64_t v = us_centre(x, mean);
    n2 += v * v;
  });
  us_block_sum2(n2, unused, s);
  if (threadIdx.x == 0) {
    mean_out[u] = mean;
    norm2_out[u] = n2;
  }
}

QRLSH_EXPORT int qrlsh_user_rows_stats(const int32_t *ratings, int64_t nu, int64_t nq, const uint32_t *rows, int64_t m,
                                       double *mean, int64_t *norm2, void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && m >= 0 && nu < (1ll << 31) && nq < (1ll << 31) && (rows || m == nu),
               "qrlsh_user_rows_stats: bad sizes nu=%lld nq=%lld m=%lld", (long long)nu, (long long)nq, (long long)m);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(m < (1ll << 31), "qrlsh_user_rows_stats: m=%lld", (long long)m);
  QR_CHECK_ARG((ratings || nq == 0) && mean && norm2, "qrlsh_user_rows_stats: null pointer");
  QR_CHECK_ALIGNED("qrlsh_user_rows_stats", "ratings", qr_addr(ratings), 16);
  QR_LAUNCH("user_rows_stats", user_rows_stats_kernel, dim3((unsigned)m), dim3(UST_THREADS), 0,
            static_cast<hipStream_t>(stream), ratings, nu, nq, rows, mean, norm2);
  QR_LAUNCH_CHECK("qrlsh_user_rows_stats");
  return QRLSH_OK;
}

// ---- scoring a few pairs of very long rows ----------------------------------------------------------------------------
struct UsSlices {
  int64_t cols, count;
};
// columns per slice: as few slices as fill the machine (every slice of a run reads the first row once more), within
// [US_MINCOLS, US_MAXCOLS]
static UsSlices us_slices(int64_t nq, int64_t n) {
  UsSlices s;
  const int64_t tiles = ceil_div64(n, US_TP);
  int64_t want = ceil_div64(US_WANT_WG, tiles > 0 ? tiles : 1);
  const int64_t lo = ceil_div64(nq, US_MAXCOLS), hi = ceil_div64(nq, US_MINCOLS);
  want = want < lo ? lo : want > hi ? hi : want;
  if (want < 1) want = 1;
  s.cols = ceil_div64(ceil_div64(nq, want), 4) * 4;
  if (s.cols < 4) s.cols = 4;
  s.count = ceil_div64(nq, s.cols);
  if (s.count < 1) s.count = 1;
  return s;
}

__global__ __launch_bounds__(US_THREADS) void user_pairs_score_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                     int64_t nq, const double *__restrict__ mean,
                                                                     const uint64_t *__restrict__ pairs, int64_t n,
                                                                     int64_t slice_cols, int64_t pitch,
                                                                     int64_t *__restrict__ partial) {
  __shared__ __attribute__((aligned(16))) int32_t sa[US_MAXCOLS + 4];   // the first row's centred slice, shifted so that its vectors are aligned
  __shared__ int64_t wdot[US_TP][US_THREADS / WAVE];
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * slice_cols;
  const int len = (int)min(slice_cols, nq - c0);
  const int64_t p0 = (int64_t)blockIdx.y * US_TP;
  const int np = (int)min((int64_t)US_TP, n - p0);
  int64_t cur_a = -1;
  int sh = 0;   // column c0 + k of the first row sits at sa[sh + k]
  for (int k = 0; k < np; ++k) {
    const uint64_t pr = pairs[p0 + k];
    const int64_t a = (int64_t)(pr >> 32), b = (int64_t)(pr & 0xFFFFFFFFull);
    if (a != cur_a) {   // uniform
      cur_a = a;
      __syncthreads();   // the lanes still reading the previous first row
      const bool ok = a < nu;
      const int64_t e0 = ok ? a * nq + c0 : 0;
      const UsPiece pc = us_piece(e0, len);
      sh = (4 - pc.head) & 3;
      const double ma = ok ? mean[a] : 0.0;
      const int32_t *src = ratings + e0;
      if (t < pc.head) sa[sh + t] = ok ? us_centre(src[t], ma) : 0;
      if (t >= WAVE && t - WAVE < pc.tail) sa[sh + pc.tail0 + t - WAVE] = ok ? us_centre(src[pc.tail0 + t - WAVE], ma) : 0;
      const us_i32x4 *v = reinterpret_cast<const us_i32x4 *>(src + pc.head);
      us_i32x4 x[US_VPT];
#pragma unroll
      for (int j = 0; j < US_VPT; ++j) {
        const int i = t + j * US_THREADS;
        x[j] = (ok && i < pc.nvec) ? v[i] : us_i32x4{0, 0, 0, 0};
      }
#pragma unroll
      for (int j = 0; j < US_VPT; ++j) {
        const int i = t + j * US_THREADS;
        if (i < pc.nvec) {
          us_i32x4 c;
          c.x = us_centre(x[j].x, ma), c.y = us_centre(x[j].y, ma), c.z = us_centre(x[j].z, ma), c.w = us_centre(x[j].w, ma);
          *reinterpret_cast<us_i32x4 *>(&sa[sh + pc.head + 4 * i]) = c;
        }
      }
      __syncthreads();
    }
    int64_t dot = 0;
    if (b < nu && a < nu) {   // uniform
      const int64_t e0 = b * nq + c0;
      const UsPiece pc = us_piece(e0, len);
      const double mb = mean[b];
      const int32_t *src = ratings + e0;
      const us_i32x4 *v = reinterpret_cast<const us_i32x4 *>(src + pc.head);
      us_i32x4 x[US_VPT];
#pragma unroll
      for (int j = 0; j < US_VPT; ++j) {   // every load of the piece is in flight before the first use
        const int i = t + j * US_THREADS;
        x[j] = i < pc.nvec ? v[i] : us_i32x4{0, 0, 0, 0};
      }
      if (t < pc.head) dot += (int64_t)sa[sh + t] * us_centre(src[t], mb);
      if (t >= WAVE && t - WAVE < pc.tail) dot += (int64_t)sa[sh + pc.tail0 + t - WAVE] * us_centre(src[pc.tail0 + t - WAVE], mb);
#pragma unroll
      for (int j = 0; j < US_VPT; ++j) {
        const int i = t + j * US_THREADS;
        if (i < pc.nvec) {
          const int32_t *q = &sa[sh + pc.head + 4 * i];
          dot += (int64_t)q[0] * us_centre(x[j].x, mb) + (int64_t)q[1] * us_centre(x[j].y, mb) +
                 (int64_t)q[2] * us_centre(x[j].z, mb) + (int64_t)q[3] * us_centre(x[j].w, mb);
        }
      }
    }
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) dot += __shfl_xor(dot, m, WAVE);
    if (lane == 0) wdot[k][w] = dot;
  }
  __syncthreads();
  if (t < np) {
    int64_t s = 0;
#pragma unroll
    for (int i = 0; i < US_THREADS / WAVE; ++i) s += wdot[t][i];
    partial[(int64_t)blockIdx.x * pitch + p0 + t] = s;
  }
}

// one wave per pair: the lanes share the slices (a handful of pairs has hundreds of them)
__global__ __launch_bounds__(US_THREADS) void user_pairs_finish_kernel(const int64_t *__restrict__ partial, int64_t slices,
                                                                      const uint64_t *__restrict__ pairs, int64_t n,
                                                                      int64_t nu, const int64_t *__restrict__ norm2,
                                                                      int32_t *__restrict__ milli) {
  const int lane = lane_id();
  const int64_t i = (int64_t)blockIdx.x * (US_THREADS / WAVE) + (threadIdx.x >> 6);
  if (i >= n) return;   // (wave-uniform)
  int64_t dot = 0;
  for (int64_t s = lane; s < slices; s += WAVE) dot += partial[s * n + i];
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) dot += __shfl_xor(dot, m, WAVE);
  if (lane != 0) return;
  const uint64_t pr = pairs[i];
  const int64_t a = (int64_t)(pr >> 32), b = (int64_t)(pr & 0xFFFFFFFFull);
  const int64_t na = a < nu ? norm2[a] : 0, nb = b < nu ? norm2[b] : 0;
  double cs = 0.0;
  if (na != 0 && nb != 0) cs = (double)dot / (sqrt((double)na) * sqrt((double)nb));
  milli[i] = (int32_t)rint(cs * 1000.0);
}

// workspace: one partial dot product per (slice of the columns, pair)
static int64_t *pairs_score_layout(QrCarve &c, int64_t nq, int64_t n) {
  return c.take<int64_t>((size_t)us_slices(nq, n).count * (size_t)n, 8);
}
QRLSH_EXPORT size_t qrlsh_user_pairs_score_workspace_bytes(int64_t nq, int64_t n) {
  if (nq <= 0 || n <= 0) return 16;
  return QR_LAYOUT_BYTES(pairs_score_layout, nq, n);
}

QRLSH_EXPORT int qrlsh_user_pairs_score(const int32_t *ratings, int64_t nu, int64_t nq, const double *mean,
                                        const int64_t *norm2, const uint64_t *pairs, int64_t n, int32_t *milli_out,
                                        void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && n >= 0 && nu < (1ll << 31) && nq < (1ll << 31) && n < (1ll << 32),
               "qrlsh_user_pairs_score: bad sizes nu=%lld nq=%lld n=%lld", (long long)nu, (long long)nq, (long long)n);
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(mean && norm2 && pairs && milli_out && workspace && (ratings || nq == 0),
               "qrlsh_user_pairs_score: null pointer");
  QR_CHECK_ALIGNED("qrlsh_user_pairs_score", "ratings", qr_addr(ratings), 16);
  QR_CHECK_WORKSPACE("qrlsh_user_pairs_score", workspace, workspace_bytes, qrlsh_user_pairs_score_workspace_bytes(nq, n));
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  int64_t *partial = pairs_score_layout(c, nq, n);
  int64_t slices = 0;
  if (nq > 0) {
    const UsSlices s = us_slices(nq, n);
    slices = s.count;
    const int64_t tiles = ceil_div64(n, US_TP);
    // tiles go on the grid's y axis (65 535 at most): more pairs than that are served in several launches
    constexpr int64_t Y = 65535;
    for (int64_t t0 = 0; t0 < tiles; t0 += Y) {
      const int64_t ty = tiles - t0 < Y ? tiles - t0 : Y, pbase = t0 * US_TP;
      const int64_t cnt = n - pbase < ty * US_TP ? n - pbase : ty * US_TP;
      // a launch sees its own pairs as 0 .. cnt-1; the row pitch of the partial sums stays n
      QR_LAUNCH("user_pairs_score", user_pairs_score_kernel, dim3((unsigned)slices, (unsigned)ty), dim3(US_THREADS), 0, st,
                ratings, nu, nq, mean, pairs + pbase, cnt, s.cols, n, partial + pbase);
    }
  }
  QR_LAUNCH("user_pairs_finish", user_pairs_finish_kernel, dim3((unsigned)ceil_div64(n, US_THREADS / WAVE)), dim3(US_THREADS), 0, st,
            (const int64_t *)partial, slices, pairs, n, nu, norm2, milli_out);
  QR_LAUNCH_CHECK("qrlsh_user_pairs_score");
  return QRLSH_OK;
}

// ---- the pairs of chosen rows with their clusters ---------------------------------------------------------------------
// cluster structure: label int32 [nu] dense in [0, nc), c_off int64 [nc + 1], c_mem int32 [nu] (members ascending
// within a cluster), c_pos int32 [nu] (a user's place in its cluster)
__device__ static inline bool ul_cluster(const int32_t *label, const int64_t *c_off, int64_t nc, int64_t u, int64_t &lo,
                                         int64_t &size) {
  const int64_t c = label[u];
  if (c < 0 || c >= nc) return false;
  lo = c_off[c];
  size = c_off[c + 1] - lo;
  return size > 0;
}

__global__ __launch_bounds__(US_THREADS) void user_cluster_pairs_count_kernel(const uint32_t *__restrict__ rows, int64_t s,
                                                                             const int32_t *__restrict__ label,
                                                                             const int64_t *__restrict__ c_off, int64_t nu,
                                                                             int64_t nc, uint64_t *__restrict__ off) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= s) return;
  const int64_t u = rows[x];
  int64_t lo = 0, size = 0;
  off[x] = (u < nu && ul_cluster(label, c_off, nc, u, lo, size)) ? (uint64_t)(size - 1) : 0ull;
}

// one wave per row: member j of the cluster goes to slot off[x] + j - (j > the row's own place)
__global__ __launch_bounds__(US_THREADS) void user_cluster_pairs_fill_kernel(const uint32_t *__restrict__ rows, int64_t s,
                                                                            const int32_t *__restrict__ label,
                                                                            const int64_t *__restrict__ c_off,
                                                                            const int32_t *__restrict__ c_mem,
                                                                            const int32_t *__restrict__ c_pos, int64_t nu,
                                                                            int64_t nc, const int64_t *__restrict__ off,
                                                                            uint64_t *__restrict__ pairs) {
  const int lane = lane_id();
  constexpr int WPB = US_THREADS / WAVE;
  for (int64_t x = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); x < s; x += (int64_t)gridDim.x * WPB) {
    const int64_t u = rows[x];
    int64_t lo = 0, size = 0;
    if (u >= nu || !ul_cluster(label, c_off, nc, u, lo, size)) continue;
    const int64_t pu = c_pos[u], base = off[x], end = off[x + 1];
    for (int64_t j = lane; j < size; j += WAVE) {
      if (j == pu) continue;
      const int64_t at = base + j - (j > pu);
      if (at < end) pairs[at] = ((uint64_t)u << 32) | (uint32_t)c_mem[lo + j];
    }
  }
}

static bool ul_sizes_ok(int64_t nu, int64_t nc) { return nu >= 0 && nu < (1ll << 31) && nc >= 0 && nc <= nu; }

QRLSH_EXPORT int qrlsh_user_cluster_pairs_count(const uint32_t *rows, int64_t s, const int32_t *label, const int64_t *c_off,
                                                int64_t nu, int64_t nc, int64_t *off_out, void *stream) {
  QR_CHECK_ARG(s >= 0 && s < (1ll << 31) && ul_sizes_ok(nu, nc), "qrlsh_user_cluster_pairs_count: bad sizes s=%lld nu=%lld nc=%lld",
               (long long)s, (long long)nu, (long long)nc);
  if (s == 0) return QRLSH_OK;
  QR_CHECK_ARG(rows && label && c_off && off_out, "qrlsh_user_cluster_pairs_count: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint64_t *off = reinterpret_cast<uint64_t *>(off_out);
  QR_LAUNCH("user_cluster_pairs_count", user_cluster_pairs_count_kernel, dim3((unsigned)ceil_div64(s, US_THREADS)),
            dim3(US_THREADS), 0, st, rows, s, label, c_off, nu, nc, off);
  qr_scan_u64(off, s, off + s, nullptr, st);   // rows are few: the one-workgroup scan
  QR_LAUNCH_CHECK("qrlsh_user_cluster_pairs_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_user_cluster_pairs_fill(const uint32_t *rows, int64_t s, const int32_t *label, const int64_t *c_off,
                                               const int32_t *c_mem, const int32_t *c_pos, int64_t nu, int64_t nc,
                                               const int64_t *off, uint64_t *pairs_out, void *stream) {
  QR_CHECK_ARG(s >= 0 && s < (1ll << 31) && ul_sizes_ok(nu, nc), "qrlsh_user_cluster_pairs_fill: bad sizes s=%lld nu=%lld nc=%lld",
               (long long)s, (long long)nu, (long long)nc);
  if (s == 0) return QRLSH_OK;
  QR_CHECK_ARG(rows && label && c_off && c_mem && c_pos && off && pairs_out, "qrlsh_user_cluster_pairs_fill: null pointer");
  QR_LAUNCH("user_cluster_pairs_fill", user_cluster_pairs_fill_kernel, dim3(rm_grid(s, US_THREADS / WAVE)), dim3(US_THREADS), 0,
            static_cast<hipStream_t>(stream), rows, s, label, c_off, c_mem, c_pos, nu, nc, off, pairs_out);
  QR_LAUNCH_CHECK("qrlsh_user_cluster_pairs_fill");
  return QRLSH_OK;
}

// ---- the lists ----------------------------------------------------------------------------------------------------------
// dense lists: idx int32 [nu][K] (-1 past the end), milli int32 [nu][K] (0 past the end), len int32 [nu]; a row is
// ordered by value descending, then id ascending, and holds positive values only.
//
// one lane per stored entry: a row outside R with exactly K entries, one of them in R, enters the pick map; whoever
// sets its bit adds the row's pair count (cluster size - 1) to out3[2]
__global__ __launch_bounds__(US_THREADS) void user_lists_mark_kernel(const int32_t *__restrict__ idx,
                                                                    const int32_t *__restrict__ len, int64_t nu, int K,
                                                                    const uint2 *__restrict__ changed,
                                                                    const int32_t *__restrict__ label,
                                                                    const int64_t *__restrict__ c_off, int64_t nc,
                                                                    uint2 *__restrict__ pick, uint64_t *__restrict__ out3) {
  bool bad = false;
  const int64_t all = nu * K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < all; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = e / K;
    const int k = (int)(e - v * K), L = len[v];
    if (L < 0 || L > K) {
      bad = true;
      continue;
    }
    if (k >= L) continue;
    const int64_t d = idx[e];
    if (d < 0 || d >= nu) {
      bad = true;
      continue;
    }
    if (L != K || idmap_has(changed[v >> 5], (uint32_t)v) || !idmap_has(changed[d >> 5], (uint32_t)d)) continue;
    uint32_t *bits = reinterpret_cast<uint32_t *>(pick + (v >> 5));
    const uint32_t m = 1u << (v & 31);
    if (__hip_atomic_load(bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) continue;
    if (atomicOr(bits, m) & m) continue;
    int64_t lo = 0, size = 0;
    if (ul_cluster(label, c_off, nc, v, lo, size))
      atomicAdd(reinterpret_cast<unsigned long long *>(out3 + 2), (unsigned long long)(size - 1));
  }
  if (__ballot(bad) && lane_id() == 0) atomicOr(reinterpret_cast<unsigned long long *>(out3 + 1), ~0ull);
}

QRLSH_EXPORT int qrlsh_user_lists_mark(const int32_t *idx, const int32_t *len, int64_t nu, int32_t K, const void *changed_map,
                                       const int32_t *label, const int64_t *c_off, int64_t nc, void *pick_map_out,
                                       uint64_t *out3, void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= UL_MAXK, "qrlsh_user_lists_mark: K=%d must be in [1, %d]", K, UL_MAXK);
  QR_CHECK_ARG(ul_sizes_ok(nu, nc), "qrlsh_user_lists_mark: bad sizes nu=%lld nc=%lld", (long long)nu, (long long)nc);
  if (nu == 0) return QRLSH_OK;
  QR_CHECK_ARG(idx && len && changed_map && label && c_off && pick_map_out && out3, "qrlsh_user_lists_mark: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const IdMap pk = idmap_layout(pick_map_out, nu);
  QR_MEMSET("qrlsh_user_lists_mark", pk.w, 0, (size_t)(pk.nw + 1) * 8, st);
  QR_MEMSET("qrlsh_user_lists_mark", out3, 0, 3 * sizeof(uint64_t), st);
  QR_LAUNCH("user_lists_mark", user_lists_mark_kernel, dim3(rm_grid(nu * K, US_THREADS)), dim3(US_THREADS), 0, st, idx, len,
            nu, (int)K, (const uint2 *)idmap_layout(changed_map, nu).w, label, c_off, nc, pk.w, out3);
  idmap_finish(pk, out3, st);
  QR_LAUNCH_CHECK("qrlsh_user_lists_mark");
  return QRLSH_OK;
}

// the best 64 of the 64 held and 64 offered words, in order, one per lane (a one-wave workgroup calls it: the barriers
// cost nothing).  Non-zero words are distinct (distinct ids), so their ranks are.
__device__ static inline uint64_t ul_merge(uint64_t best, uint64_t cand, uint64_t *slot) {
  const int lane = threadIdx.x;
  int rb = 0, rc = 0;
#pragma unroll 8
  for (int j = 0; j < WAVE; ++j) {
    const uint64_t kb = __shfl(best, j, WAVE), kc = __shfl(cand, j, WAVE);
    rb += (kb > best) + (kc > best);
    rc += (kb > cand) + (kc > cand);
  }
  __syncthreads();
  slot[lane] = 0;
  __syncthreads();
  if (best != 0 && rb < WAVE) slot[rb] = best;
  if (cand != 0 && rc < WAVE) slot[rc] = cand;
  __syncthreads();
  return slot[lane];
}

// one wave (= one workgroup) per row of the matrix; rows of untouched clusters leave without a write
__global__ __launch_bounds__(WAVE) void user_lists_apply_kernel(int32_t *__restrict__ idx, int32_t *__restrict__ milli,
                                                               int32_t *__restrict__ len, int64_t nu, int K,
                                                               const uint2 *__restrict__ changed,
                                                               const uint2 *__restrict__ pick,
                                                               const int32_t *__restrict__ label,
                                                               const int64_t *__restrict__ c_off,
                                                               const int32_t *__restrict__ c_mem,
                                                               const int32_t *__restrict__ c_pos, int64_t nc,
                                                               const int64_t *__restrict__ off,
                                                               const int32_t *__restrict__ pair_milli, int64_t n_pairs) {
  __shared__ uint64_t slot[WAVE];
  const int lane = threadIdx.x;
  for (int64_t v = blockIdx.x; v < nu; v += gridDim.x) {
    int64_t lo = 0, size = 0;
    if (!ul_cluster(label, c_off, nc, v, lo, size)) continue;   // (uniform: the whole wave serves one row)
    const uint2 wr = changed[v >> 5], wp = pick[v >> 5];
    const bool in_s = idmap_has(wr, (uint32_t)v) || idmap_has(wp, (uint32_t)v);
    const int64_t pv = c_pos[v];
    const int64_t base = in_s ? off[idmap_rank(wr, (uint32_t)v) + idmap_rank(wp, (uint32_t)v)] : 0;
    uint64_t best = 0;
    bool touched = in_s, merged = false;
    if (!in_s) {   // the stored entries outside R (holes close in the merge)
      const int L = len[v];
      if (lane < L && lane < K) {
        const int64_t d = idx[v * K + lane];
        const int32_t mi = milli[v * K + lane];
        if (d >= 0 && d < nu && mi > 0 && !idmap_has(changed[d >> 5], (uint32_t)d)) best = ul_key(mi, d);
      }
    }
    for (int64_t j0 = 0; j0 < size; j0 += WAVE) {
      const int64_t j = j0 + lane;
      uint64_t cand = 0;
      bool is_r = false;
      if (j < size && j != pv) {
        const int64_t m = c_mem[lo + j];
        int64_t at = -1;
        if (in_s) {
          at = base + j - (j > pv);
        } else if (m >= 0 && m < nu) {
          const uint2 mr = changed[m >> 5];
          if (idmap_has(mr, (uint32_t)m)) {   // the pair (m, v) in the block of m's row
            is_r = true;
            at = off[idmap_rank(mr, (uint32_t)m) + idmap_rank(pick[m >> 5], (uint32_t)m)] + pv - (pv > j);
          }
        }
        if (at >= 0 && at < n_pairs) {
          const int32_t mi = pair_milli[at];
          if (mi > 0) cand = ul_key(mi, m);
        }
      }
      touched |= __ballot(is_r) != 0;
      if (__ballot(cand != 0)) {
        best = ul_merge(best, cand, slot);
        merged = true;
      }
    }
    if (!touched) continue;
    if (!merged) best = ul_merge(best, 0, slot);
    const bool valid = lane < K && best != 0;
    const int cnt = __popcll(__ballot(valid));
    if (lane < K) {
      idx[v * K + lane] = valid ? 0x7FFFFFFF - (int32_t)(uint32_t)best : -1;
      milli[v * K + lane] = valid ? (int32_t)(best >> 32) : 0;
    }
    if (lane == 0) len[v] = cnt;
  }
}

QRLSH_EXPORT int qrlsh_user_lists_apply(int32_t *idx, int32_t *milli, int32_t *len, int64_t nu, int32_t K,
                                        const void *changed_map, const void *pick_map, int64_t s, const int32_t *label,
                                        const int64_t *c_off, const int32_t *c_mem, const int32_t *c_pos, int64_t nc,
                                        const int64_t *off, const int32_t *pair_milli, int64_t n_pairs, void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= UL_MAXK, "qrlsh_user_lists_apply: K=%d must be in [1, %d]", K, UL_MAXK);
  QR_CHECK_ARG(ul_sizes_ok(nu, nc) && s >= 0 && s <= nu && n_pairs >= 0 && n_pairs < (1ll << 32),
               "qrlsh_user_lists_apply: bad sizes nu=%lld nc=%lld s=%lld pairs=%lld", (long long)nu, (long long)nc,
               (long long)s, (long long)n_pairs);
  if (s == 0 || nu == 0) return QRLSH_OK;
  QR_CHECK_ARG(idx && milli && len && changed_map && pick_map && label && c_off && c_mem && c_pos && off &&
                   (pair_milli || n_pairs == 0),
               "qrlsh_user_lists_apply: null pointer");
  QR_LAUNCH("user_lists_apply", user_lists_apply_kernel, dim3((unsigned)(nu < 16384 ? nu : 16384)),
            dim3(WAVE), 0, static_cast<hipStream_t>(stream), idx, milli, len, nu, (int)K,
            (const uint2 *)idmap_layout(changed_map, nu).w,
            (const uint2 *)idmap_layout(pick_map, nu).w, label, c_off, c_mem, c_pos, nc, off, pair_milli,
            n_pairs);
  QR_LAUNCH_CHECK("qrlsh_user_lists_apply");
  return QRLSH_OK;
}
