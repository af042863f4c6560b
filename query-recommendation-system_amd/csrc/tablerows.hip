// tablerows.hip -- dataset rows come and go under a built index: which served queries a batch of rows changes, and (for
// added rows) their new signature rows, in one sweep over the served queries.
//
// A dataset row lives in a slot: slot s owns row s of the permutation table and bit s of every value bitmap.  A query is
// nfeat value ids (bitmap rows; -1 = unconstrained), a batch row is nfeat value ids (its cells): query q matches batch row
// j iff every constrained feature of q holds the cell's value id.  No bitmap is read.
//
//   mark      one lane per served query tests the batch in tiles of 64 rows (cells staged in LDS, feature-major, read
//             wave-uniformly: broadcasts) and keeps a 64-bit match mask per tile.  The wave then walks its lanes that have
//             a non-zero mask, its lanes now being the positions p of that query's row in rounds of 64: ADD marks the query
//             when a matched row has tab[slot][p] < sig[q][p] (unsigned: the -1 of an empty set loses to every value),
//             REMOVE when tab[slot][p] == sig[q][p].  The walk of a query ends at the first round that hits, and a query
//             that is marked is not tested against later tiles.  Table rows are read where they are (L1 / L2).
//   fill      one wave per changed query: lane j tests batch row j of a tile, the ballots are parked in LDS (one word per
//             tile), then lanes are positions: umin of the old value and the matched rows' table values, written once in
//             the index's row format with the exact int64 norm.
//   set_rows  the batch's bits in the value rows and the live row, one lane per (row, feature or live) cell.
#include "idmap.h"

constexpr int TR_THREADS = 256;
constexpr int TR_TILE = 64;        // batch rows per tile: one bit of a lane's mask each
constexpr int TR_MAXF = 63;        // features (the live row is the 64th column of an answer-set query)
constexpr int TR_MAXM = 65536;     // batch rows per call

template <bool U16> __device__ static inline uint32_t tr_word(const void *base, int64_t at) {
  return U16 ? (uint32_t) static_cast<const uint16_t *>(base)[at] : static_cast<const uint32_t *>(base)[at];
}

// ---- which queries change ---------------------------------------------------------------------------------------------
template <bool TAB16, bool SIG16, bool ADD>
__global__ __launch_bounds__(TR_THREADS) void table_rows_mark_kernel(const int32_t *__restrict__ qrows, int64_t n, int nfeat,
                                                                    const int32_t *__restrict__ cells,
                                                                    const int32_t *__restrict__ slots, int m,
                                                                    const void *__restrict__ tab, int P, int64_t stride,
                                                                    const void *__restrict__ sig, uint2 *__restrict__ map,
                                                                    uint64_t *__restrict__ out2) {
  __shared__ int32_t s_cells[TR_MAXF * TR_TILE];  // [f][j]
  __shared__ int32_t s_slots[TR_TILE];
  const int lane = lane_id();
  const int64_t nblk = (n + TR_THREADS - 1) / TR_THREADS;
  for (int64_t qb = blockIdx.x; qb < nblk; qb += gridDim.x) {
    const int64_t wave_q0 = qb * TR_THREADS + (threadIdx.x & ~(WAVE - 1));
    const int64_t q = wave_q0 + lane;
    const bool have = q < n;
    bool matched = false, changed = false;
    for (int j0 = 0; j0 < m; j0 += TR_TILE) {
      const int tm = min(TR_TILE, m - j0);
      __syncthreads();  // the tile before this one has been read
      for (int e = threadIdx.x; e < tm * nfeat; e += TR_THREADS) {
        const int j = e / nfeat, f = e - j * nfeat;
        s_cells[f * TR_TILE + j] = cells[(int64_t)j0 * nfeat + e];
      }
      if ((int)threadIdx.x < tm) s_slots[threadIdx.x] = slots[j0 + threadIdx.x];
      __syncthreads();
      uint64_t mask = 0;
      if (have && !changed) {
        mask = tm == TR_TILE ? ~0ull : (1ull << tm) - 1ull;  // entries past tm are stale: never counted
        for (int f = 0; f < nfeat && mask; ++f) {
          const int32_t v = qrows[q * nfeat + f];
          if (v == -1) continue;
          uint32_t lo = 0, hi = 0;
#pragma unroll 8
          for (int j = 0; j < 32; ++j) {
            lo |= (uint32_t)(s_cells[f * TR_TILE + j] == v) << j;
            hi |= (uint32_t)(s_cells[f * TR_TILE + 32 + j] == v) << j;
          }
          mask &= (uint64_t)hi << 32 | lo;
        }
      }
      matched |= mask != 0;
      uint64_t todo = __ballot(mask != 0);  // wave-uniform from here on
      while (todo) {
        const int L = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t mk = __shfl((unsigned long long)mask, L, WAVE);
        const int64_t qL = wave_q0 + L;
        bool hit = false;
        for (int p0 = 0; p0 < P; p0 += WAVE) {
          const int p = p0 + lane;
          if (p < P) {
            const uint32_t s = tr_word<SIG16>(sig, qL * P + p);
            uint64_t r = mk;
            while (r) {
              const int j = __ffsll((unsigned long long)r) - 1;
              r &= r - 1;
              const uint32_t t = tr_word<TAB16>(tab, (int64_t)s_slots[j] * stride + p);
              hit |= ADD ? t < s : t == s;
            }
          }
          if (__any(hit)) break;
        }
        if (__any(hit)) {
          if (lane == L) changed = true;
          if (lane == 0) idmap_set(map, (uint32_t)qL);
        }
      }
    }
    const uint64_t mb = __ballot(matched);
    if (lane == 0 && mb) atomicAdd(reinterpret_cast<unsigned long long *>(out2), (unsigned long long)__popcll(mb));
  }
}

static int table_rows_check(const char *who, const int32_t *qrows, int64_t n, int32_t nfeat, const int32_t *cells,
                            const int32_t *slots, int64_t m, const void *perm_t, int32_t perm_dtype, int32_t P,
                            int32_t P_stride, const void *sig, int32_t sig_dtype) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && nfeat >= 1 && nfeat <= TR_MAXF && m >= 0 && m <= TR_MAXM,
               "%s: bad sizes n=%lld nfeat=%d m=%lld (n < 2^32 - 1, 1 <= nfeat <= 63, m <= 65536)", who, (long long)n, nfeat,
               (long long)m);
  QR_CHECK_ARG(P >= 1 && P_stride >= P, "%s: bad P=%d P_stride=%d", who, P, P_stride);
  QR_CHECK_ARG((perm_dtype == QRLSH_PERM_U16 || perm_dtype == QRLSH_PERM_I32) &&
                   (sig_dtype == QRLSH_SIG_I32 || (sig_dtype == QRLSH_SIG_U16 && perm_dtype == QRLSH_PERM_U16)),
               "%s: bad formats perm_dtype=%d sig_dtype=%d (compact rows need a uint16 table)", who, perm_dtype, sig_dtype);
  QR_CHECK_ARG(n == 0 || m == 0 || (qrows && cells && slots && perm_t && sig), "%s: null pointer", who);
  return QRLSH_OK;
}

#define TR_DISPATCH(LAUNCH)                                          \
  do {                                                               \
    if (perm_dtype == QRLSH_PERM_I32) LAUNCH(false, false);          \
    else if (sig_dtype == QRLSH_SIG_I32) LAUNCH(true, false);        \
    else LAUNCH(true, true);                                         \
  } while (0)

QRLSH_EXPORT int qrlsh_table_rows_mark(const int32_t *qrows, int64_t n, int32_t nfeat, const int32_t *batch_cells,
                                       const int32_t *batch_slots, int64_t m, const void *perm_t, int32_t perm_dtype,
                                       int32_t P, int32_t P_stride, const void *sig, int32_t sig_dtype, int32_t mode,
                                       void *changed_map, uint64_t *out2, void *stream) {
  const int rc = table_rows_check("qrlsh_table_rows_mark", qrows, n, nfeat, batch_cells, batch_slots, m, perm_t, perm_dtype,
                                  P, P_stride, sig, sig_dtype);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(mode == QRLSH_ROWS_ADD || mode == QRLSH_ROWS_REMOVE, "qrlsh_table_rows_mark: bad mode %d", mode);
  QR_CHECK_ARG(changed_map && out2, "qrlsh_table_rows_mark: null output");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const IdMap mp = idmap_layout(changed_map, n);
  QR_MEMSET("qrlsh_table_rows_mark", mp.w, 0, (size_t)(mp.nw + 1) * 8, st);
  QR_MEMSET("qrlsh_table_rows_mark", out2, 0, 2 * sizeof(uint64_t), st);
  if (n > 0 && m > 0) {
    const dim3 grid(rm_grid(n, TR_THREADS)), block(TR_THREADS);
#define TR_MARK(T16, S16)                                                                                              \
  do {                                                                                                                 \
    if (mode == QRLSH_ROWS_ADD)                                                                                        \
      QR_LAUNCH("table_rows_mark", (table_rows_mark_kernel<T16, S16, true>), grid, block, 0, st, qrows, n, (int)nfeat, \
                batch_cells, batch_slots, (int)m, perm_t, (int)P, (int64_t)P_stride, sig, mp.w, out2);                 \
    else                                                                                                               \
      QR_LAUNCH("table_rows_mark", (table_rows_mark_kernel<T16, S16, false>), grid, block, 0, st, qrows, n, (int)nfeat, \
                batch_cells, batch_slots, (int)m, perm_t, (int)P, (int64_t)P_stride, sig, mp.w, out2);                 \
  } while (0)
    TR_DISPATCH(TR_MARK);
#undef TR_MARK
  }
  idmap_finish(mp, out2 + 1, st);
  QR_LAUNCH_CHECK("qrlsh_table_rows_mark");
  return QRLSH_OK;
}

// ---- the new rows of the changed queries (additions) ------------------------------------------------------------------
template <bool TAB16, bool SIG16>
__global__ __launch_bounds__(TR_THREADS) void table_rows_fill_kernel(const int32_t *__restrict__ qrows, int64_t n, int nfeat,
                                                                    const int32_t *__restrict__ cells,
                                                                    const int32_t *__restrict__ slots, int m,
                                                                    const void *__restrict__ tab, int P, int64_t stride,
                                                                    const void *__restrict__ sig,
                                                                    const uint32_t *__restrict__ ids, int64_t c,
                                                                    void *__restrict__ sig_out,
                                                                    int64_t *__restrict__ norm2_out) {
  extern __shared__ uint64_t s_mask[];  // [waves][tiles]: the match ballots of the wave's query
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int ntiles = (m + TR_TILE - 1) / TR_TILE;
  uint64_t *mk = s_mask + (size_t)wave * ntiles;
  const int64_t nblk = (c + TR_THREADS / WAVE - 1) / (TR_THREADS / WAVE);
  for (int64_t xb = blockIdx.x; xb < nblk; xb += gridDim.x) {
    const int64_t x = xb * (TR_THREADS / WAVE) + wave;
    const int64_t q = x < c ? (int64_t)ids[x] : n;
    const bool have = q < n;  // wave-uniform; an id outside the index writes nothing
    const int32_t mine = have && lane < nfeat ? qrows[q * nfeat + lane] : -1;
    __syncthreads();  // the masks of the round before have been read
    for (int t = 0; t < ntiles; ++t) {
      const int j = t * TR_TILE + lane;
      bool ok = have && j < m;
      for (int f = 0; f < nfeat; ++f) {
        const int32_t v = __shfl(mine, f, WAVE);
        if (v != -1 && ok) ok = cells[(int64_t)j * nfeat + f] == v;
      }
      const uint64_t b = __ballot(ok);
      if (lane == 0) mk[t] = b;
    }
    __syncthreads();
    if (!have) continue;
    int64_t nrm = 0;
    for (int p0 = 0; p0 < P; p0 += WAVE) {
      const int p = p0 + lane;
      const bool in = p < P;
      uint32_t acc = in ? tr_word<SIG16>(sig, q * P + p) : 0u;
      for (int t = 0; t < ntiles; ++t) {
        uint64_t r = mk[t];
        while (r) {
          const int j = t * TR_TILE + __ffsll((unsigned long long)r) - 1;
          r &= r - 1;
          const int64_t slot = slots[j];
          if (in) acc = min(acc, tr_word<TAB16>(tab, slot * stride + p));
        }
      }
      if (in) {
        int64_t v;
        if (SIG16) {
          static_cast<uint16_t *>(sig_out)[x * P + p] = (uint16_t)acc;
          v = acc == 0xFFFFu ? -1 : (int64_t)acc;
        } else {
          static_cast<uint32_t *>(sig_out)[x * P + p] = acc;
          v = (int64_t)(int32_t)acc;
        }
        nrm += v * v;
      }
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) nrm += __shfl_xor(nrm, d, WAVE);
    if (lane == 0) norm2_out[x] = nrm;
  }
}

QRLSH_EXPORT int qrlsh_table_rows_fill(const int32_t *qrows, int64_t n, int32_t nfeat, const int32_t *batch_cells,
                                       const int32_t *batch_slots, int64_t m, const void *perm_t, int32_t perm_dtype,
                                       int32_t P, int32_t P_stride, const void *sig, int32_t sig_dtype,
                                       const uint32_t *changed_ids, int64_t c, void *sig_out, int64_t *norm2_out,
                                       void *stream) {
  const int rc = table_rows_check("qrlsh_table_rows_fill", qrows, n, nfeat, batch_cells, batch_slots, m, perm_t, perm_dtype,
                                  P, P_stride, sig, sig_dtype);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(c >= 0 && c <= n, "qrlsh_table_rows_fill: bad c=%lld (n=%lld)", (long long)c, (long long)n);
  if (c == 0) return QRLSH_OK;
  QR_CHECK_ARG(m > 0 && changed_ids && sig_out && norm2_out, "qrlsh_table_rows_fill: null pointer or an empty batch");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(rm_grid(c, TR_THREADS / WAVE)), block(TR_THREADS);
  const size_t lds = (size_t)(TR_THREADS / WAVE) * ((m + TR_TILE - 1) / TR_TILE) * sizeof(uint64_t);
#define TR_FILL(T16, S16)                                                                                                  \
  QR_LAUNCH("table_rows_fill", (table_rows_fill_kernel<T16, S16>), grid, block, lds, st, qrows, n, (int)nfeat,            \
            batch_cells, batch_slots, (int)m, perm_t, (int)P, (int64_t)P_stride, sig, changed_ids, c, sig_out, norm2_out)
  TR_DISPATCH(TR_FILL);
#undef TR_FILL
  QR_LAUNCH_CHECK("qrlsh_table_rows_fill");
  return QRLSH_OK;
}

// ---- the batch's bits -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TR_THREADS) void bitmaps_set_rows_kernel(uint32_t *__restrict__ bitmaps, int64_t wpr,
                                                                     const int32_t *__restrict__ cells,
                                                                     const int32_t *__restrict__ slots, int64_t m,
                                                                     int nfeat, int64_t live_row, int on) {
  const int64_t all = m * (nfeat + 1);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < all; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / (nfeat + 1);
    const int f = (int)(e - j * (nfeat + 1));
    const int64_t row = f < nfeat ? (int64_t)cells[j * nfeat + f] : live_row;
    const int64_t slot = slots[j];
    if (row < 0 || slot < 0 || (slot >> 5) >= wpr) continue;  // nothing outside a bitmap row is touched
    uint32_t *w = bitmaps + row * wpr + (slot >> 5);
    const uint32_t bit = 1u << (slot & 31);
    if (on) atomicOr(w, bit);
    else atomicAnd(w, ~bit);
  }
}

QRLSH_EXPORT int qrlsh_bitmaps_set_rows(uint32_t *bitmaps, int64_t words_per_row, const int32_t *batch_cells,
                                        const int32_t *batch_slots, int64_t m, int32_t nfeat, int64_t live_row, int32_t on,
                                        void *stream) {
  QR_CHECK_ARG(words_per_row > 0 && m >= 0 && m < (1ll << 31) && nfeat >= 1 && nfeat <= TR_MAXF && live_row >= 0 &&
                   (on == 0 || on == 1),
               "qrlsh_bitmaps_set_rows: bad arguments words_per_row=%lld m=%lld nfeat=%d live_row=%lld on=%d",
               (long long)words_per_row, (long long)m, nfeat, (long long)live_row, on);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(bitmaps && batch_cells && batch_slots, "qrlsh_bitmaps_set_rows: null pointer");
  QR_LAUNCH("bitmaps_set_rows", bitmaps_set_rows_kernel, dim3(rm_grid(m * (nfeat + 1), TR_THREADS)), dim3(TR_THREADS), 0,
            static_cast<hipStream_t>(stream), bitmaps, words_per_row, batch_cells, batch_slots, m, (int)nfeat, live_row,
            (int)on);
  QR_LAUNCH_CHECK("qrlsh_bitmaps_set_rows");
  return QRLSH_OK;
}
