// userrows.hip -- users join and leave the live user lists (userlists.hip) without a rebuild: the most similar existing
// user of every new row, the matrix in its new row space, and the lists under the new numbering.
//
// Labels and K stay those of the build.  A batch of new rows is userlists.hip's update with R = the new ids over grown
// arrays (no stored entry names a new id: nothing is picked); a removal is the same update with R = the removed rows
// whose statistics are zero (their scores are 0, positive-only lists drop them), followed by the renumbering.
//
//   rows_nearest    the hot kernel: m new rows against all nu existing rows, m x nu regular pairs.  Grid = (slice of
//                   UR_COLS columns, tile of UR_TM new rows, group of existing rows that are 4 apart).  A workgroup
//                   centres its tile's slice once into LDS; each wave then streams existing rows past it: 16-byte loads
//                   on the row's own alignment, centred in registers, one 16-byte LDS read per staged row and vector.
//                   Rows 4 apart start at the same offset modulo 4, so the tile is staged shifted to THEIR alignment and
//                   every LDS read is an aligned vector.  The UR_TM sums of a lane are reduced across the wave by a
//                   halving butterfly (10 shuffles instead of 48) and added to dots int64 [nu][m] with 64-bit integer
//                   atomics: exact integers, any order.  A finish kernel, one workgroup per new row, evaluates the score
//                   kernels' float64 expression and takes the maximum by the lists' key (value, then lower id).
//   rows_move       out[u2] = src[u2] >= 0 ? in[src[u2]] : block[~src[u2]], out of place.  16-byte stores on the output's
//                   alignment with scalar head and tail; 16-byte loads where the source row piece shares that alignment
//                   (always when nq % 4 == 0), 4-byte loads otherwise.
//   lists_renumber  one lane per entry of the new lists: row src[u2] of the old ones, every id through new_pos.
#include "userlists.h"

constexpr int UR_THREADS = 256;
constexpr int UR_WAVES = UR_THREADS / WAVE;
constexpr int UR_TM = 8;                           // new rows staged per workgroup
constexpr int UR_VPT = 4;                          // 16-byte vectors per lane and existing row
constexpr int UR_COLS = WAVE * UR_VPT * 4;         // columns per slice (1024): a wave holds a row's slice in registers
constexpr int UR_PITCH = UR_COLS + 4;              // LDS row pitch in words (a multiple of 4; room for the shift)
constexpr int UR_GROUP = 128;                      // existing rows per workgroup and tile, 4 apart (32 per wave)
constexpr int UR_MAXY = 65535;                     // tiles side by side
constexpr int UR_MAXZ = 4096;                      // groups side by side (grid z = 4 * this at most)

// the UR_TM sums of every lane -> the wave's total of sum ur_row(lane) in v[0] of every lane
__device__ static inline int ur_row(int lane) { return ((lane & 1) << 2) | (lane & 2) | ((lane >> 2) & 1); }
__device__ static inline int64_t ur_reduce(int64_t (&v)[UR_TM], int lane) {
#pragma unroll
  for (int n = UR_TM / 2, mask = 1; n >= 1; n >>= 1, mask <<= 1) {
    const bool upper = lane & mask;   // the upper lane of a pair keeps the upper half of the sums
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const int64_t give = upper ? v[i] : v[i + n], keep = upper ? v[i + n] : v[i];
      v[i] = keep + __shfl_xor(give, mask, WAVE);
    }
  }
  int64_t s = v[0];
#pragma unroll
  for (int mask = UR_TM; mask < WAVE; mask <<= 1) s += __shfl_xor(s, mask, WAVE);
  return s;
}

__global__ __launch_bounds__(UR_THREADS) void user_rows_nearest_kernel(const int32_t *__restrict__ ratings, int64_t nu,
                                                                      int64_t nq, const double *__restrict__ mean,
                                                                      const int32_t *__restrict__ rows, int64_t m,
                                                                      const double *__restrict__ rmean, int64_t tiles,
                                                                      int64_t groups, int64_t *__restrict__ dots) {
  __shared__ __attribute__((aligned(16))) int32_t sa[UR_TM][UR_PITCH];
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * UR_COLS;
  const int len = (int)min((int64_t)UR_COLS, nq - c0);
  const int r = blockIdx.z & 3;   // existing rows r, r + 4, ...: (u * nq + c0) & 3 is that of row r
  const UsPiece pc = us_piece((int64_t)r * nq + c0, len);
  const int sh = (4 - pc.head) & 3;   // column c0 + k of a staged row sits at sa[.][sh + k]: sh + head is 0 or 4
  // the scalar column of this lane in every existing row (lanes below head, lanes 32 .. 32 + tail - 1), or -1
  const int sc = lane < pc.head ? lane : (lane >= 32 && lane - 32 < pc.tail) ? pc.tail0 + lane - 32 : -1;
  const bool scalars = pc.head + pc.tail > 0;   // uniform
  const int mine = ur_row(lane);

  for (int64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int64_t k0 = tile * UR_TM;
    const int nk = (int)min((int64_t)UR_TM, m - k0);
    __syncthreads();   // the waves still reading the previous tile
    for (int k = 0; k < nk; ++k) {
      const int32_t *src = rows + (k0 + k) * nq + c0;
      const double mk = rmean[k0 + k];
      for (int c = t; c < len; c += UR_THREADS) sa[k][sh + c] = us_centre(src[c], mk);
    }
    __syncthreads();
    for (int64_t g = blockIdx.z >> 2; g < groups; g += gridDim.z >> 2) {
      const int64_t u0 = r + 4 * (g * UR_GROUP + w);   // this wave's rows: u0, u0 + 16, ...
      us_i32x4 nx[UR_VPT];
      if (u0 < nu) {
        const us_i32x4 *v = reinterpret_cast<const us_i32x4 *>(ratings + u0 * nq + c0 + pc.head);
#pragma unroll
        for (int j = 0; j < UR_VPT; ++j) {
          const int i = lane + j * WAVE;
          nx[j] = i < pc.nvec ? v[i] : us_i32x4{0, 0, 0, 0};
        }
      }
      for (int jr = 0; jr < UR_GROUP / UR_WAVES; ++jr) {
        const int64_t u = u0 + 4 * UR_WAVES * jr;
        if (u >= nu) break;   // wave-uniform
        us_i32x4 x[UR_VPT];
#pragma unroll
        for (int j = 0; j < UR_VPT; ++j) x[j] = nx[j];
        const int64_t un = u + 4 * UR_WAVES;
        if (jr + 1 < UR_GROUP / UR_WAVES && un < nu) {   // the next row's loads are in flight during this row's sums
          const us_i32x4 *v = reinterpret_cast<const us_i32x4 *>(ratings + un * nq + c0 + pc.head);
#pragma unroll
          for (int j = 0; j < UR_VPT; ++j) {
            const int i = lane + j * WAVE;
            nx[j] = i < pc.nvec ? v[i] : us_i32x4{0, 0, 0, 0};
          }
        }
        const double mb = mean[u];
        int64_t acc[UR_TM];
#pragma unroll
        for (int k = 0; k < UR_TM; ++k) acc[k] = 0;
        if (scalars) {
          const int sci = sc >= 0 ? sc : 0;   // lanes without a scalar column add 0 times a word that exists
          const int64_t y = sc >= 0 ? us_centre(ratings[u * nq + c0 + sci], mb) : 0;
#pragma unroll
          for (int k = 0; k < UR_TM; ++k)
            if (k < nk) acc[k] += y * sa[k][sh + sci];
        }
#pragma unroll
        for (int j = 0; j < UR_VPT; ++j) {
          // vectors past the piece hold zeros: whatever the LDS words behind the slice hold, the products are 0
          const int64_t y0 = us_centre(x[j].x, mb), y1 = us_centre(x[j].y, mb), y2 = us_centre(x[j].z, mb),
                        y3 = us_centre(x[j].w, mb);
          const int at = sh + pc.head + 4 * (lane + j * WAVE);
#pragma unroll
          for (int k = 0; k < UR_TM; ++k) {
            if (k < nk) {   // uniform
              const us_i32x4 q = *reinterpret_cast<const us_i32x4 *>(&sa[k][at]);
              acc[k] += y0 * q.x + y1 * q.y + y2 * q.z + y3 * q.w;
            }
          }
        }
        const int64_t sum = ur_reduce(acc, lane);
        if (lane < UR_TM && mine < nk && sum != 0)
          atomicAdd(reinterpret_cast<unsigned long long *>(dots + u * m + k0 + mine), (unsigned long long)sum);
      }
    }
  }
}

// one workgroup per new row: the scores of the row against every existing user, and the best by (value, lower id)
__global__ __launch_bounds__(UR_THREADS) void user_rows_nearest_finish_kernel(const int64_t *__restrict__ dots, int64_t nu,
                                                                             int64_t m, const int64_t *__restrict__ norm2,
                                                                             const int64_t *__restrict__ rnorm2,
                                                                             int32_t *__restrict__ best_user,
                                                                             int32_t *__restrict__ best_milli,
                                                                             int32_t *__restrict__ milli_out) {
  __shared__ uint64_t wbest[UR_WAVES];
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  for (int64_t k = blockIdx.x; k < m; k += gridDim.x) {
    const int64_t na = rnorm2[k];
    uint64_t best = 0;
    for (int64_t u = t; u < nu; u += UR_THREADS) {
      const int64_t dot = dots[u * m + k], nb = norm2[u];
      double cs = 0.0;
      if (na != 0 && nb != 0) cs = (double)dot / (sqrt((double)na) * sqrt((double)nb));
      const int32_t mi = (int32_t)rint(cs * 1000.0);
      if (milli_out) milli_out[k * nu + u] = mi;
      if (mi > 0) {
        const uint64_t key = ul_key(mi, u);
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int mask = 1; mask < WAVE; mask <<= 1) {
      const uint64_t o = __shfl_xor(best, mask, WAVE);
      best = o > best ? o : best;
    }
    __syncthreads();   // wbest may still be read for the previous row
    if (lane == 0) wbest[w] = best;
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < UR_WAVES; ++i) best = wbest[i] > best ? wbest[i] : best;
      best_user[k] = best ? 0x7FFFFFFF - (int32_t)(uint32_t)best : -1;
      best_milli[k] = (int32_t)(best >> 32);
    }
  }
}

static bool ur_nearest_sizes_ok(int64_t nu, int64_t nq, int64_t m) {
  return nu >= 0 && nq >= 0 && m >= 0 && nu < (1ll << 31) && nq < (1ll << 31) && m < (1ll << 31) &&
         (nu == 0 || m <= ((1ll << 32) - 1) / nu);
}

// workspace: the dot product of every (user, batch row)
static int64_t *rows_nearest_layout(QrCarve &c, int64_t nu, int64_t m) {
  return c.take<int64_t>((size_t)nu * (size_t)m, 8);
}
QRLSH_EXPORT size_t qrlsh_user_rows_nearest_workspace_bytes(int64_t nu, int64_t m) {
  if (nu <= 0 || m <= 0 || nu >= (1ll << 31) || m > ((1ll << 32) - 1) / nu) return 16;
  return QR_LAYOUT_BYTES(rows_nearest_layout, nu, m);
}

QRLSH_EXPORT int qrlsh_user_rows_nearest(const int32_t *ratings, int64_t nu, int64_t nq, const double *mean,
                                         const int64_t *norm2, const int32_t *rows, int64_t m, const double *rows_mean,
                                         const int64_t *rows_norm2, int32_t *best_user_out, int32_t *best_milli_out,
                                         int32_t *milli_out, void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(ur_nearest_sizes_ok(nu, nq, m), "qrlsh_user_rows_nearest: bad sizes nu=%lld nq=%lld m=%lld (m * nu < 2^32)",
               (long long)nu, (long long)nq, (long long)m);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(rows_mean && rows_norm2 && best_user_out && best_milli_out && workspace && (rows || nq == 0) &&
                   (nu == 0 || (mean && norm2 && (ratings || nq == 0))),
               "qrlsh_user_rows_nearest: null pointer");
  QR_CHECK_ALIGNED("qrlsh_user_rows_nearest", "ratings and rows", qr_addr(ratings) | qr_addr(rows), 16);
  QR_CHECK_ALIGNED("qrlsh_user_rows_nearest", "the workspace", qr_addr(workspace), 8);
  QR_CHECK_WORKSPACE("qrlsh_user_rows_nearest", workspace, workspace_bytes, qrlsh_user_rows_nearest_workspace_bytes(nu, m));
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  int64_t *dots = rows_nearest_layout(c, nu, m);
  if (nu > 0) QR_MEMSET("qrlsh_user_rows_nearest", dots, 0, (size_t)nu * (size_t)m * sizeof(int64_t), st);
  if (nu > 0 && nq > 0) {
    const int64_t tiles = ceil_div64(m, UR_TM), groups = ceil_div64(ceil_div64(nu, 4), UR_GROUP);
    const dim3 grid((unsigned)ceil_div64(nq, UR_COLS), (unsigned)(tiles < UR_MAXY ? tiles : UR_MAXY),
                    4u * (unsigned)(groups < UR_MAXZ ? groups : UR_MAXZ));
    QR_LAUNCH("user_rows_nearest", user_rows_nearest_kernel, grid, dim3(UR_THREADS), 0, st, ratings, nu, nq, mean, rows, m,
              rows_mean, tiles, groups, dots);
  }
  QR_LAUNCH("user_rows_nearest_finish", user_rows_nearest_finish_kernel, dim3((unsigned)(m < 16384 ? m : 16384)),
            dim3(UR_THREADS), 0, st, (const int64_t *)dots, nu, m, norm2, rows_norm2, best_user_out, best_milli_out,
            milli_out);
  QR_LAUNCH_CHECK("qrlsh_user_rows_nearest");
  return QRLSH_OK;
}

// ---- the matrix in its new row space ----------------------------------------------------------------------------------
constexpr int UM_VPT = 4;                               // 16-byte vectors per lane and row
constexpr int UM_TILE = UR_THREADS * UM_VPT * 4;        // columns per workgroup (4096)
constexpr int UM_MAXY = 16384;                          // rows side by side

__global__ __launch_bounds__(UR_THREADS) void ratings_rows_move_kernel(const int32_t *__restrict__ in, int64_t nu,
                                                                      int64_t nq, const int32_t *__restrict__ src,
                                                                      int64_t nu2, const int32_t *__restrict__ block,
                                                                      int64_t m, int32_t *__restrict__ out,
                                                                      uint32_t *__restrict__ flag) {
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * UM_TILE;
  const int len = (int)min((int64_t)UM_TILE, nq - c0);
  for (int64_t u2 = blockIdx.y; u2 < nu2; u2 += gridDim.y) {
    const int64_t s = src[u2];
    if (s >= 0 ? s >= nu : ~s >= m) {   // uniform: the row stays unwritten
      if (blockIdx.x == 0 && t == 0) atomicOr(flag, 1u);
      continue;
    }
    const int32_t *from = (s >= 0 ? in + s * nq : block + ~s * nq) + c0;
    int32_t *to = out + u2 * nq + c0;
    const UsPiece pc = us_piece(u2 * nq + c0, len);   // by the output's alignment
    const bool same = (reinterpret_cast<uintptr_t>(from + pc.head) & 15) == 0;   // uniform
    us_i32x4 x[UM_VPT];
    if (same) {
      const us_i32x4 *v = reinterpret_cast<const us_i32x4 *>(from + pc.head);
#pragma unroll
      for (int j = 0; j < UM_VPT; ++j) {
        const int i = t + j * UR_THREADS;
        x[j] = i < pc.nvec ? v[i] : us_i32x4{0, 0, 0, 0};
      }
    } else {
#pragma unroll
      for (int j = 0; j < UM_VPT; ++j) {
        const int i = t + j * UR_THREADS;
        const int32_t *p = from + pc.head + 4 * i;
        x[j] = i < pc.nvec ? us_i32x4{p[0], p[1], p[2], p[3]} : us_i32x4{0, 0, 0, 0};
      }
    }
    if (t < pc.head) to[t] = from[t];
    if (t >= WAVE && t - WAVE < pc.tail) to[pc.tail0 + t - WAVE] = from[pc.tail0 + t - WAVE];
#pragma unroll
    for (int j = 0; j < UM_VPT; ++j) {
      const int i = t + j * UR_THREADS;
      if (i < pc.nvec) *reinterpret_cast<us_i32x4 *>(to + pc.head + 4 * i) = x[j];
    }
  }
}

QRLSH_EXPORT int qrlsh_ratings_rows_move(const int32_t *in, int64_t nu, int64_t nq, const int32_t *src, int64_t nu2,
                                         const int32_t *block, int64_t m, int32_t *out, uint32_t *flag_out, void *stream) {
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && nu2 >= 0 && m >= 0 && nu < (1ll << 31) && nq < (1ll << 31) && nu2 < (1ll << 31) &&
                   m < (1ll << 31),
               "qrlsh_ratings_rows_move: bad sizes nu=%lld nq=%lld nu2=%lld m=%lld", (long long)nu, (long long)nq,
               (long long)nu2, (long long)m);
  if (nu2 == 0) return QRLSH_OK;
  QR_CHECK_ARG(flag_out && src && (nq == 0 || (out && (in || nu == 0) && (block || m == 0))),
               "qrlsh_ratings_rows_move: null pointer");
  QR_CHECK_ALIGNED("qrlsh_ratings_rows_move", "out", qr_addr(out), 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_ratings_rows_move", flag_out, 0, sizeof(uint32_t), st);
  // nq == 0: one column tile of no columns, so that a src outside range is still seen
  const int64_t tiles = nq > 0 ? ceil_div64(nq, UM_TILE) : 1;
  QR_LAUNCH("ratings_rows_move", ratings_rows_move_kernel, dim3((unsigned)tiles, (unsigned)(nu2 < UM_MAXY ? nu2 : UM_MAXY)),
            dim3(UR_THREADS), 0, st, in, nu, nq, src, nu2, block, m, out, flag_out);
  QR_LAUNCH_CHECK("qrlsh_ratings_rows_move");
  return QRLSH_OK;
}

// ---- the lists under the new numbering ----------------------------------------------------------------------------------
__global__ __launch_bounds__(UR_THREADS) void user_lists_renumber_kernel(const int32_t *__restrict__ idx,
                                                                        const int32_t *__restrict__ milli,
                                                                        const int32_t *__restrict__ len, int64_t nu, int K,
                                                                        const int32_t *__restrict__ src, int64_t nu2,
                                                                        const int32_t *__restrict__ new_pos,
                                                                        int32_t *__restrict__ idx_out,
                                                                        int32_t *__restrict__ milli_out,
                                                                        int32_t *__restrict__ len_out,
                                                                        uint32_t *__restrict__ flag) {
  bool bad = false;
  const int64_t all = nu2 * K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < all; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t u2 = e / K, s = src[u2];
    const int k = (int)(e - u2 * K);
    int32_t d = -1, mi = 0, L = 0;
    if (s >= nu) {
      bad = true;
    } else if (s >= 0) {
      L = len[s];
      if (L < 0 || L > K) {
        bad = true;
        L = 0;
      } else if (k < L) {
        const int64_t o = idx[s * K + k];
        const int64_t n = o >= 0 && o < nu ? new_pos[o] : -1;
        if (n < 0 || n >= nu2) bad = true;   // an entry whose target is gone, or an index outside range
        d = (int32_t)n;
        mi = milli[s * K + k];
      }
    }
    idx_out[e] = d;
    milli_out[e] = mi;
    if (k == 0) len_out[u2] = L;
  }
  if (__ballot(bad) && lane_id() == 0) atomicOr(flag, 1u);
}

QRLSH_EXPORT int qrlsh_user_lists_renumber(const int32_t *idx, const int32_t *milli, const int32_t *len, int64_t nu,
                                           int32_t K, const int32_t *src, int64_t nu2, const int32_t *new_pos,
                                           int32_t *idx_out, int32_t *milli_out, int32_t *len_out, uint32_t *flag_out,
                                           void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= UL_MAXK, "qrlsh_user_lists_renumber: K=%d must be in [1, %d]", K, UL_MAXK);
  QR_CHECK_ARG(nu >= 0 && nu2 >= 0 && nu < (1ll << 31) && nu2 < (1ll << 31),
               "qrlsh_user_lists_renumber: bad sizes nu=%lld nu2=%lld", (long long)nu, (long long)nu2);
  if (nu2 == 0) return QRLSH_OK;
  QR_CHECK_ARG(src && idx_out && milli_out && len_out && flag_out && (nu == 0 || (idx && milli && len && new_pos)),
               "qrlsh_user_lists_renumber: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_user_lists_renumber", flag_out, 0, sizeof(uint32_t), st);
  QR_LAUNCH("user_lists_renumber", user_lists_renumber_kernel, dim3(rm_grid(nu2 * K, UR_THREADS)), dim3(UR_THREADS), 0, st,
            idx, milli, len, nu, (int)K, src, nu2, new_pos, idx_out, milli_out, len_out, flag_out);
  QR_LAUNCH_CHECK("qrlsh_user_lists_renumber");
  return QRLSH_OK;
}
