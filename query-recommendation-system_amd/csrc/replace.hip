// replace.hip -- queries of a built index get new rows in place: ids, n, b and the directory width stay as they are.
//
// R is a set of m distinct ids, given ascending (rids), with the id map of remove.hip over it; batch row x goes to id
// rids[x].  A band's order is "top 32 bits of mix64(key), then id ascending", so the band after the replacement is the
// old band without the records of R -- the SURVIVORS, in place order -- merged with the batch records sorted by
// (mix bits, id).  A replaced id sits in the middle of the id range: among equal mix bits a batch record goes where
// its id puts it, not behind the old records as an appended one does.
//
//   rows:   one lane per 16 bytes (8 / 4 / 2 for other widths) of a batch row: row x overwrites row rids[x].
//   index:  sort:  the batch as the build sorts it (mix bits 32..64, payload = batch index, which is the id order).
//           count: one workgroup per (tile of RM_TILE records, band) counts its survivors (ids read, one map load
//                  each) and writes the composite (mix bits << 32 | id) of every record that leaves to slot rank_R(id)
//                  of the band's "left" list.  Slots ascend by id, so a stable sort on bits 32..64 orders the list by
//                  (mix bits, id): half the passes of a 64-bit sort.  A scan over all (band, tile) counts follows.
//           rank:  one lane per sorted batch record j: p = old records that order before (bits, id) (old directory,
//                  then a binary search on the composite), q = records of the left list that do; s_j = p - q survivors
//                  order before it and it is written at s_j + j.  The left list was chosen over counting the removed
//                  records in front of p from the tile counts plus a sweep of p's tile: that sweep reads up to
//                  RM_TILE ids per batch record, the list costs two searches of log2(m) steps.
//           fill:  the tile ranks its survivors with ballots; survivor number s of the band goes to
//                  s + #{j : s_j <= s}.  Two searches per tile narrow the batch range to [jlo, jhi); a tile whose range
//                  is empty is a copy shifted by jlo.  A survivor whose id is in the pick map also leaves its key as
//                  the probe key of that row, as the removal does.
//           The directory is index_dir_kernel over the output.  12 B read + 12 B written per band record, plus 4 B for
//           the ids of the count pass and 8 B for the directory's read.
//   lists:  rows outside R keep their stored entries whose dst is outside R and gain the replaced queries that now
//           name them; a row of exactly K entries that loses one is picked (qrlsh_lists_remove_mark over R) and probed
//           again, rows of R are probed with their new rows.  That is the merge of lists.hip with R as the dropped
//           ids and rids as the record ids: qrlsh_lists_replace_* live there.
#include "idmap.h"

__device__ static inline uint32_t rp_top32(uint64_t k) { return (uint32_t)(qr_mix64(k) >> 32); }

// ---- rows -----------------------------------------------------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(RM_THREADS) void rows_replace_kernel(V *__restrict__ rows, int64_t chunks,
                                                                 int64_t *__restrict__ norm2, int64_t n,
                                                                 const uint32_t *__restrict__ rids,
                                                                 const V *__restrict__ new_rows,
                                                                 const int64_t *__restrict__ new_norm2, int64_t m) {
  const int64_t all = m * chunks;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < all; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t x = g / chunks, c = g - x * chunks;
    const int64_t i = rids[x];
    if (i >= n) continue;  // never, for ids the map build accepted
    rows[i * chunks + c] = new_rows[g];
    if (c == 0 && norm2) norm2[i] = new_norm2[x];
  }
}

template <typename V>
static void rows_replace_launch(void *rows, int64_t row_bytes, int64_t *norm2, int64_t n, const uint32_t *rids,
                                const void *new_rows, const int64_t *new_norm2, int64_t m, hipStream_t st) {
  const int64_t chunks = row_bytes / (int64_t)sizeof(V);
  QR_LAUNCH("rows_replace", rows_replace_kernel<V>, dim3(rm_grid(m * chunks, RM_THREADS)), dim3(RM_THREADS), 0, st,
            static_cast<V *>(rows), chunks, norm2, n, rids, static_cast<const V *>(new_rows), new_norm2, m);
}

QRLSH_EXPORT int qrlsh_rows_replace(void *rows, int64_t row_bytes, int64_t *norm2, int64_t n, const uint32_t *ids,
                                    const void *new_rows, const int64_t *new_norm2, int64_t m, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && m >= 0 && m <= n && row_bytes > 0 && row_bytes % 2 == 0,
               "qrlsh_rows_replace: bad sizes n=%lld m=%lld row_bytes=%lld (a multiple of 2)", (long long)n, (long long)m,
               (long long)row_bytes);
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(rows && ids && new_rows && (!norm2 || new_norm2), "qrlsh_rows_replace: null pointer");
  QR_CHECK_ALIGNED("qrlsh_rows_replace", "rows", qr_addr(rows) | qr_addr(new_rows), 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (row_bytes % 16 == 0) rows_replace_launch<uint4>(rows, row_bytes, norm2, n, ids, new_rows, new_norm2, m, st);
  else if (row_bytes % 8 == 0) rows_replace_launch<uint2>(rows, row_bytes, norm2, n, ids, new_rows, new_norm2, m, st);
  else if (row_bytes % 4 == 0) rows_replace_launch<uint32_t>(rows, row_bytes, norm2, n, ids, new_rows, new_norm2, m, st);
  else rows_replace_launch<uint16_t>(rows, row_bytes, norm2, n, ids, new_rows, new_norm2, m, st);
  QR_LAUNCH_CHECK("qrlsh_rows_replace");
  return QRLSH_OK;
}

// ---- index ----------------------------------------------------------------------------------------------------------
// one workgroup per (tile, band): tile_cnt[band * tiles + tile] = survivors of the tile; a record that leaves writes
// its composite to left[band][rank_R(id)]
__global__ __launch_bounds__(RM_THREADS) void index_replace_count_kernel(const uint64_t *__restrict__ keys,
                                                                        const uint32_t *__restrict__ ids, int64_t n,
                                                                        int64_t m, const uint2 *__restrict__ rm,
                                                                        uint64_t *__restrict__ tile_cnt,
                                                                        uint64_t *__restrict__ left) {
  __shared__ uint32_t wc[RM_PER * 4];
  const int64_t t = blockIdx.y, tile = blockIdx.x;
  const int64_t o = tile * RM_TILE;
  const uint32_t *bi = ids + t * n;
  const uint64_t *bk = keys + t * n;
  uint32_t id[RM_PER];
  uint2 w[RM_PER];
  bool keep[RM_PER];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {  // every load of the tile is issued before the first is used
    const int64_t x = o + (int64_t)k * RM_THREADS + threadIdx.x;
    id[k] = x < n ? bi[x] : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const bool ok = (int64_t)id[k] < n;  // false past the band's end (and for an id no build writes)
    w[k] = ok ? rm[id[k] >> 5] : make_uint2(0u, 0u);
    keep[k] = ok && !idmap_has(w[k], id[k]);
  }
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const int64_t x = o + (int64_t)k * RM_THREADS + threadIdx.x;
    if (keep[k] || (int64_t)id[k] >= n) continue;
    const int64_t j = idmap_rank(w[k], id[k]);
    if (j < m) left[t * m + j] = (uint64_t)rp_top32(bk[x]) << 32 | id[k];
  }
  uint32_t before[RM_PER];
  const uint32_t kept = rm_tile_prefix(keep, wc, before);
  if (threadIdx.x == 0) tile_cnt[t * gridDim.x + tile] = kept;
}

// first position of [L, R) of a sorted band whose (mix bits, id) is not below c = bits << 32 | id
__device__ static inline uint32_t rp_lower_band(const uint64_t *bk, const uint32_t *bi, uint32_t L, uint32_t R, uint64_t c) {
  while (L < R) {
    const uint32_t mid = L + (R - L) / 2;
    if (((uint64_t)rp_top32(bk[mid]) << 32 | bi[mid]) < c) L = mid + 1;
    else R = mid;
  }
  return L;
}

// one lane per (band, sorted batch record j): s[band][j] = survivors that order before it; the record goes to s + j
__global__ __launch_bounds__(RM_THREADS) void index_replace_rank_kernel(
    const uint64_t *__restrict__ okeys, const uint32_t *__restrict__ oids, const uint32_t *__restrict__ odir, int64_t n,
    int d, const uint64_t *__restrict__ bkeys, const uint32_t *__restrict__ bx, const uint32_t *__restrict__ rids,
    const uint64_t *__restrict__ left, int64_t m, uint32_t *__restrict__ s_out, uint64_t *__restrict__ keys_out,
    uint32_t *__restrict__ ids_out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t t = blockIdx.y;
  const uint64_t key = bkeys[t * m + j];
  const uint32_t x = bx[t * m + j];
  if ((int64_t)x >= m) return;  // never, for the payload the sort wrote
  const uint32_t id = rids[x];
  const uint64_t h = qr_mix64(key);
  const uint64_t c = (h >> 32) << 32 | id;
  const uint32_t *bd = odir + t * ((1ll << d) + 1);
  const uint32_t p = rp_lower_band(okeys + t * n, oids + t * n, bd[h >> (64 - d)], bd[(h >> (64 - d)) + 1], c);
  const uint64_t *lf = left + t * m;
  int64_t L = 0, R = m;
  while (L < R) {
    const int64_t mid = L + (R - L) / 2;
    if (lf[mid] < c) L = mid + 1;
    else R = mid;
  }
  const int64_t s = (int64_t)p - L;  // >= 0: every record of the left list below c is an old record below c
  s_out[t * m + j] = (uint32_t)s;
  const int64_t pos = s + j;
  if (s < 0 || pos >= n) return;  // never, for a band that holds every id once
  keys_out[t * n + pos] = key;
  ids_out[t * n + pos] = id;
}

// #{j in [L, R) : s[j] <= v} + L for the non-decreasing s
__device__ static inline int64_t rp_upper(const uint32_t *s, int64_t L, int64_t R, int64_t v) {
  while (L < R) {
    const int64_t mid = L + (R - L) / 2;
    if ((int64_t)s[mid] <= v) L = mid + 1;
    else R = mid;
  }
  return L;
}

// one workgroup per (tile, band); tile_off = the exclusive scan of the counts over the bands back to back
__global__ __launch_bounds__(RM_THREADS) void index_replace_fill_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ids, int64_t n, int64_t m,
    const uint2 *__restrict__ rm, const uint2 *__restrict__ pick, int64_t n_pick, const uint64_t *__restrict__ tile_off,
    const uint32_t *__restrict__ s_all, uint64_t *__restrict__ keys_out, uint32_t *__restrict__ ids_out,
    uint64_t *__restrict__ pick_keys_out) {
  __shared__ uint32_t wc[RM_PER * 4];
  const int64_t t = blockIdx.y, tile = blockIdx.x;
  const int64_t o = tile * RM_TILE;
  const uint32_t *bi = ids + t * n;
  const uint64_t *bk = keys + t * n;
  uint32_t id[RM_PER];
  uint64_t key[RM_PER];
  bool keep[RM_PER];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {  // every load of the tile is issued before the first is used
    const int64_t x = o + (int64_t)k * RM_THREADS + threadIdx.x;
    id[k] = x < n ? bi[x] : 0xFFFFFFFFu;
    key[k] = x < n ? bk[x] : 0;
  }
  const int64_t base = (int64_t)tile_off[t * gridDim.x + tile] - t * (n - m);  // survivors of the band before the tile
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const bool ok = (int64_t)id[k] < n;
    const uint2 w = ok ? rm[id[k] >> 5] : make_uint2(0u, 0u);
    keep[k] = ok && !idmap_has(w, id[k]);
  }
  uint32_t before[RM_PER];
  const uint32_t kept = rm_tile_prefix(keep, wc, before);
  if (kept == 0 || base < 0) return;
  const uint32_t *s = s_all + t * m;
  const int64_t jlo = rp_upper(s, 0, m, base);                  // batch records before the tile's first survivor
  const int64_t jhi = rp_upper(s, jlo, m, base + kept - 1);     // ... and before its last
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    if (!keep[k]) continue;
    const int64_t sv = base + before[k];
    const int64_t pos = sv + (jlo == jhi ? jlo : rp_upper(s, jlo, jhi, sv));
    if (pos < n) {  // always, for a band that holds every id once
      keys_out[t * n + pos] = key[k];
      ids_out[t * n + pos] = id[k];
    }
    if (pick) {
      const uint2 pw = pick[id[k] >> 5];
      const int64_t j = idmap_rank(pw, id[k]);
      if (idmap_has(pw, id[k]) && j < n_pick) pick_keys_out[t * n_pick + j] = key[k];
    }
  }
}

struct RpWs {
  uint64_t *ktmp, *left_a, *left_b, *tile_off, *sums;
  uint32_t *bx, *xtmp, *s;
  void *sort_ws;
  size_t sort_bytes;
};
static RpWs rp_layout(QrCarve &c, int64_t n, int64_t m, int32_t b) {
  RpWs w;
  const size_t bm = (size_t)b * (size_t)m;
  const int64_t tiles = ceil_div64(n, RM_TILE) * b;
  w.ktmp = c.take<uint64_t>(bm);
  w.left_a = c.take<uint64_t>(bm);
  w.left_b = c.take<uint64_t>(bm);
  w.bx = c.take<uint32_t>(bm);
  w.xtmp = c.take<uint32_t>(bm);
  w.s = c.take<uint32_t>(bm);
  w.tile_off = c.take<uint64_t>((size_t)(tiles + 1));
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(tiles, SCANL_CHUNK) + 1));
  w.sort_bytes = qrlsh_sort_workspace_bytes(m, b);
  w.sort_ws = c.take_bytes(w.sort_bytes);
  return w;
}

QRLSH_EXPORT size_t qrlsh_index_replace_workspace_bytes(int64_t n, int64_t m, int32_t b) {
  if (n <= 0 || m <= 0 || b <= 0) return 0;
  return QR_LAYOUT_BYTES(rp_layout, n, m, b);
}

QRLSH_EXPORT int qrlsh_index_replace(const uint64_t *keys, const uint32_t *ids, const uint32_t *dir, int64_t n, int32_t b,
                                     const void *replaced_map, const uint32_t *replaced_ids, uint64_t *new_keys, int64_t m,
                                     const void *pick_map, int64_t n_pick, uint64_t *keys_out, uint32_t *ids_out,
                                     uint32_t *dir_out, uint64_t *pick_keys_out, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && b > 0 && b <= 65535 && m >= 0 && m <= n && n_pick >= 0 && n_pick <= n - m,
               "qrlsh_index_replace: bad sizes n=%lld b=%d m=%lld n_pick=%lld", (long long)n, b, (long long)m,
               (long long)n_pick);
  if (m == 0) return QRLSH_OK;  // nothing changes: the outputs are not written
  QR_CHECK_ARG(keys && ids && dir && replaced_map && replaced_ids && new_keys && keys_out && ids_out && dir_out &&
                   workspace && (n_pick == 0 || (pick_map && pick_keys_out)),
               "qrlsh_index_replace: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_index_replace", workspace, workspace_bytes, qrlsh_index_replace_workspace_bytes(n, m, b));
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  const RpWs w = rp_layout(c, n, m, b);
  const int64_t tiles = ceil_div64(n, RM_TILE), all = tiles * b;
  const uint2 *rm = idmap_layout(replaced_map, n).w;
  const uint2 *pk = n_pick > 0 ? idmap_layout(pick_map, n).w : nullptr;
  int rc = qrlsh_sort_u64(new_keys, w.ktmp, w.bx, w.xtmp, m, b, 32, 64, QRLSH_SORT_MIX | QRLSH_SORT_IOTA, 0, w.sort_ws,
                          w.sort_bytes, stream);
  if (rc < 0) return rc;
  const uint64_t *sk = rc == 1 ? w.ktmp : new_keys;
  const uint32_t *sx = rc == 1 ? w.xtmp : w.bx;
  const dim3 grid((unsigned)tiles, (unsigned)b), block(RM_THREADS);
  QR_LAUNCH("index_replace_count", index_replace_count_kernel, grid, block, 0, st, keys, ids, n, m, rm, w.tile_off, w.left_a);
  qr_scan_u64(w.tile_off, all, w.tile_off + all, w.sums, st);
  rc = qrlsh_sort_u64(w.left_a, w.left_b, nullptr, nullptr, m, b, 32, 64, 0, 0, w.sort_ws, w.sort_bytes, stream);
  if (rc < 0) return rc;
  QR_LAUNCH("index_replace_rank", index_replace_rank_kernel, dim3((unsigned)ceil_div64(m, RM_THREADS), (unsigned)b), block,
            0, st, keys, ids, dir, n, (int)qrlsh_index_dir_bits(n), sk, sx, replaced_ids,
            (const uint64_t *)(rc == 1 ? w.left_b : w.left_a), m, w.s, keys_out, ids_out);
  QR_LAUNCH("index_replace_fill", index_replace_fill_kernel, grid, block, 0, st, keys, ids, n, m, rm, pk, n_pick,
            (const uint64_t *)w.tile_off, (const uint32_t *)w.s, keys_out, ids_out, pick_keys_out);
  return qr_index_dir(keys_out, n, b, dir_out, st, "qrlsh_index_replace");
}
