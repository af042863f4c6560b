// usercolumns.hip -- the matrix of the live user lists (userlists.hip) follows queries that are appended, removed or
// given new ratings: which rows a batch of column operations changes, and the matrix in its new column space.
//
// The centring mean of a row is taken over its non-zero ratings and zeros stay zero, so a column operation changes a
// user's centred row only where the user's old and new values in the affected columns differ: those rows are R, and
// userlists.hip's update rule (mark, rescore S = R + picked, merge the rest) holds word for word over the new columns.
//
//   columns_changed  one lane per (row, affected column) cell: old value against incoming value, the row enters the id
//                    map where they differ (bit tested before the atomic: a wave's cells share a few map words)
//   columns_move     the hot kernel: out[u][j] = src[j] >= 0 ? in[u][src[j]] : block[u][~src[j]].  Grid = (tile of
//                    UC_TILE output columns, group of rows).  A workgroup serves rows that are 4 apart: u * nq2 is the
//                    same modulo 4 for all of them, so the tile splits into scalar head, 16-byte vectors and scalar tail
//                    in one way (us_piece) and the lane's slice of src -- read once -- stays in registers for every row.
//                    Per row all loads are issued (4-byte gathers: a removal shifts them against the stores; src is
//                    monotone, so a wave's gathers stay within a few lines), then the 16-byte stores.  No LDS.
#include "idmap.h"

constexpr int UC_THREADS = 256;
constexpr int UC_VPT = 4;                             // 16-byte vectors per lane and row
constexpr int UC_TILE = UC_THREADS * UC_VPT * 4;      // output columns per workgroup (4096)
constexpr int UC_ROWS = 8;                            // rows per workgroup and trip, 4 apart
constexpr int UC_MAXY = 16383;                        // trips side by side (grid y = 4 * this at most)
typedef int32_t uc_i32x4 __attribute__((ext_vector_type(4)));

// ---- which rows change ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UC_THREADS) void ratings_columns_changed_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                            int64_t nq, const int32_t *__restrict__ cols,
                                                                            const int32_t *__restrict__ block, int64_t m,
                                                                            uint2 *__restrict__ map,
                                                                            uint64_t *__restrict__ out2) {
  bool wrong = false;
  const int64_t all = nu * m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < all; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u = e / m, c = cols[e - u * m];
    if (c < -1 || c >= nq) {
      wrong = true;
      continue;
    }
    const int32_t was = c >= 0 ? ratings[u * nq + c] : 0, now = block ? block[e] : 0;
    if (was != now) idmap_set(map, (uint32_t)u);
  }
  if (__ballot(wrong) && lane_id() == 0) atomicOr(reinterpret_cast<unsigned long long *>(out2 + 1), 1ull);
}

QRLSH_EXPORT int qrlsh_ratings_columns_changed(const int32_t *ratings, int64_t nu, int64_t nq, const int32_t *cols,
                                               const int32_t *block, int64_t m, void *changed_map_out, uint64_t *out2,
                                               void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && m >= 0 && nu < (1ll << 31) && nq < (1ll << 31) && m < (1ll << 31),
               "qrlsh_ratings_columns_changed: bad sizes nu=%lld nq=%lld m=%lld", (long long)nu, (long long)nq, (long long)m);
  if (m == 0 || nu == 0) return QRLSH_OK;
  QR_CHECK_ARG((ratings || nq == 0) && cols && changed_map_out && out2, "qrlsh_ratings_columns_changed: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const IdMap mp = idmap_layout(changed_map_out, nu);
  QR_MEMSET("qrlsh_ratings_columns_changed", mp.w, 0, (size_t)(mp.nw + 1) * 8, st);
  QR_MEMSET("qrlsh_ratings_columns_changed", out2, 0, 2 * sizeof(uint64_t), st);
  QR_LAUNCH("ratings_columns_changed", ratings_columns_changed_kernel, dim3(rm_grid(nu * m, UC_THREADS)), dim3(UC_THREADS),
            0, st, ratings, nu, nq, cols, block, m, mp.w, out2);
  idmap_finish(mp, out2, st);
  QR_LAUNCH_CHECK("qrlsh_ratings_columns_changed");
  return QRLSH_OK;
}

// ---- the matrix in its new column space -------------------------------------------------------------------------------
// what a lane holds of src for the whole kernel: its vectors' 4 * UC_VPT columns and one scalar column (head or tail)
__device__ static inline bool uc_valid(int32_t s, int64_t nq, int64_t m) { return s >= 0 ? s < nq : ~s < m; }

__global__ __launch_bounds__(UC_THREADS) void ratings_columns_move_kernel(const int32_t *__restrict__ in, int64_t nu,
                                                                         int64_t nq, const int32_t *__restrict__ src,
                                                                         int64_t nq2, const int32_t *__restrict__ block,
                                                                         int64_t m, int32_t *__restrict__ out,
                                                                         int64_t trips, uint32_t *__restrict__ flag) {
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * UC_TILE;
  const int len = (int)min((int64_t)UC_TILE, nq2 - c0);
  const int r = blockIdx.y & 3;   // rows r, r + 4, ...: (u * nq2 + c0) & 3 is that of row r
  // lanes below `head` and lanes 64 .. 64 + tail - 1 take the scalars before and behind the aligned middle
  const int h = (int)((4 - (((int64_t)r * nq2 + c0) & 3)) & 3);
  const int head = h < len ? h : len, nvec = (len - head) >> 2, tail0 = head + 4 * nvec, tail = len - tail0;
  const int sc = t < head ? t : (t >= WAVE && t - WAVE < tail) ? tail0 + t - WAVE : -1;

  int32_t s[UC_VPT][4], ss = 0;
  uint32_t ok = 0, ld = 0;        // bit 4 j + e (16: the scalar): the column is valid / is loaded (an absent block is zeros)
  bool wrong = false;
#pragma unroll
  for (int j = 0; j < UC_VPT; ++j) {
    const int i = t + j * UC_THREADS;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[j][e] = 0;
      if (i < nvec) {
        const int32_t v = src[c0 + head + 4 * i + e];
        s[j][e] = v;
        if (uc_valid(v, nq, m)) {
          ok |= 1u << (4 * j + e);
          if (v >= 0 || block) ld |= 1u << (4 * j + e);
        } else {
          wrong = true;
        }
      }
    }
  }
  if (sc >= 0) {
    ss = src[c0 + sc];
    if (uc_valid(ss, nq, m)) {
      ok |= 1u << 16;
      if (ss >= 0 || block) ld |= 1u << 16;
    } else {
      wrong = true;
    }
  }
  if (blockIdx.y < 4 && __ballot(wrong) && lane_id() == 0) atomicOr(flag, 1u);

  for (int64_t trip = blockIdx.y >> 2; trip < trips; trip += gridDim.y >> 2) {
    for (int k = 0; k < UC_ROWS; ++k) {
      const int64_t u = r + 4 * (trip * UC_ROWS + k);
      if (u >= nu) break;   // uniform
      const int32_t *rin = in + u * nq, *rbl = block + u * m;
      int32_t *ro = out + u * nq2 + c0;
      uc_i32x4 x[UC_VPT];
      int32_t xs = 0;
#pragma unroll
      for (int j = 0; j < UC_VPT; ++j) {   // every load of the row's piece is in flight before the first store
        int32_t y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int32_t v = s[j][e];
          const int32_t *p = v >= 0 ? rin + v : rbl + ~v;
          y[e] = (ld >> (4 * j + e)) & 1u ? *p : 0;
        }
        x[j] = uc_i32x4{y[0], y[1], y[2], y[3]};
      }
      if ((ld >> 16) & 1u) xs = *(ss >= 0 ? rin + ss : rbl + ~ss);
#pragma unroll
      for (int j = 0; j < UC_VPT; ++j) {
        const int i = t + j * UC_THREADS;
        const uint32_t k4 = (ok >> (4 * j)) & 15u;
        int32_t *q = ro + head + 4 * i;
        if (k4 == 15u) {
          *reinterpret_cast<uc_i32x4 *>(q) = x[j];
        } else if (k4) {   // a column of the vector is refused: the others one by one
          if (k4 & 1u) q[0] = x[j].x;
          if (k4 & 2u) q[1] = x[j].y;
          if (k4 & 4u) q[2] = x[j].z;
          if (k4 & 8u) q[3] = x[j].w;
        }
      }
      if ((ok >> 16) & 1u) ro[sc] = xs;
    }
  }
}

QRLSH_EXPORT int qrlsh_ratings_columns_move(const int32_t *in, int64_t nu, int64_t nq, const int32_t *src, int64_t nq2,
                                            const int32_t *block, int64_t m, int32_t *out, uint32_t *flag_out,
                                            void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && nq2 >= 0 && m >= 0 && nu < (1ll << 31) && nq < (1ll << 31) && nq2 < (1ll << 31) &&
                   m < (1ll << 31),
               "qrlsh_ratings_columns_move: bad sizes nu=%lld nq=%lld nq2=%lld m=%lld", (long long)nu, (long long)nq,
               (long long)nq2, (long long)m);
  if (m == 0 || nu == 0) return QRLSH_OK;
  QR_CHECK_ARG(flag_out && (nq2 == 0 || (src && out)) && (in || nq == 0), "qrlsh_ratings_columns_move: null pointer");
  QR_CHECK_ALIGNED("qrlsh_ratings_columns_move", "out", qr_addr(out), 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_ratings_columns_move", flag_out, 0, sizeof(uint32_t), st);
  if (nq2 == 0) return QRLSH_OK;
  const int64_t trips = ceil_div64(ceil_div64(nu, 4), UC_ROWS);
  const unsigned gy = 4u * (unsigned)(trips < UC_MAXY ? trips : UC_MAXY);
  QR_LAUNCH("ratings_columns_move", ratings_columns_move_kernel, dim3((unsigned)ceil_div64(nq2, UC_TILE), gy),
            dim3(UC_THREADS), 0, st, in, nu, nq, src, nq2, block, m, out, trips, flag_out);
  QR_LAUNCH_CHECK("qrlsh_ratings_columns_move");
  return QRLSH_OK;
}
