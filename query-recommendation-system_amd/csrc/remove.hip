// remove.hip -- queries leave a built index: the band arrays, the rows and the top-K lists shrink without a rebuild.
//
// Remove a set R of ids from 0 .. n-1 and renumber the survivors by rank: new id = old id - |{r in R : r < old id}|,
// a monotone map.  A built band is the (key, id) records sorted stably by the top 32 bits of mix64(key), ids ascending
// among equal bits, so the band of the survivors is the old band FILTERED in place order with the ids remapped -- byte
// for byte what qrlsh_index_build makes of the survivors' keys.  No sort: one stable stream compaction per band.
//
//   id map:   R as a bitmap with per-word prefix counts, one 8-byte entry {bits, members below the word} per 32 ids: a
//             single load answers "is id removed" and "how many removed ids lie below it" (shard.hip's id set keeps the
//             two in separate arrays; the compaction asks both of every record, so they share a load here).
//   index:    count: one workgroup per tile of RM_TILE records of one band counts its survivors; an exclusive scan over
//             all (band, tile) counts gives every tile its output position (each band has n - |R| survivors, so the scan
//             over the bands back to back IS the flat [b][n - |R|] position); fill: the tile reads its ids again and its
//             keys once, ranks every survivor inside the tile with wave ballots, and writes key and remapped id.  The
//             same pass writes the keys of the records a second map picks (the probe keys of the rows to re-probe).
//             The directory is index_dir_kernel over the output (one more read of the new keys).
//   rows:     one lane per 16 bytes of a surviving row (8, 4 or 2 when the row's width is no multiple of 16): row i goes
//             to row i - rank(i).
//   lists:    a stored row with fewer than K entries was never cut: it loses its removed entries and is renumbered.  A
//             row with exactly K entries that loses one may need candidates the cut threw away: mark puts it into the
//             pick map and it is probed again against the shrunk index.  count / fill compact the stored entries the
//             same way as the bands (tiles, a scan, ballots): a kept entry's output position is the kept entries before
//             it plus the re-probed entries of the picked rows below its src; the head entry of a picked row leaves
//             that row's output position for the copy of the re-probed lists (qr_lists_fill_probed, lists.hip).  Every
//             entry places itself.
#include "idmap.h"

QRLSH_EXPORT size_t qrlsh_idmap_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return QR_LAYOUT_BYTES(idmap_layout, n);
}

__global__ __launch_bounds__(RM_THREADS) void idmap_mark_kernel(const uint32_t *__restrict__ ids, int64_t m, int64_t n,
                                                               uint2 *__restrict__ map, uint64_t *__restrict__ out2) {
  bool wrong = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t id = ids[i];
    if ((int64_t)id >= n) wrong = true;
    else idmap_set(map, id);
  }
  if (__ballot(wrong) && lane_id() == 0) atomicOr(reinterpret_cast<unsigned long long *>(out2 + 1), 1ull);
}

__global__ __launch_bounds__(RM_THREADS) void idmap_popc_kernel(const uint2 *__restrict__ map, int64_t nw,
                                                               uint64_t *__restrict__ cnt) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w <= nw) cnt[w] = w < nw ? (uint64_t)__popc(map[w].x) : 0ull;  // one entry past the end: the scan leaves the total there
}

__global__ __launch_bounds__(RM_THREADS) void idmap_pack_kernel(uint2 *__restrict__ map, int64_t nw,
                                                               const uint64_t *__restrict__ cnt,
                                                               uint64_t *__restrict__ count_out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w <= nw) map[w].y = (uint32_t)cnt[w];
  if (w == nw && count_out) *count_out = cnt[nw];
}

// the bits are set: prefix counts into the entries, the member count to *count_out (may be null)
void idmap_finish(const IdMap &m, uint64_t *count_out, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div64(m.nw + 1, RM_THREADS)), block(RM_THREADS);
  QR_LAUNCH("idmap_popc", idmap_popc_kernel, grid, block, 0, st, (const uint2 *)m.w, m.nw, m.cnt);
  qr_scan_u64(m.cnt, m.nw + 1, m.cnt + m.nw + 1, m.sums, st);
  QR_LAUNCH("idmap_pack", idmap_pack_kernel, grid, block, 0, st, m.w, m.nw, (const uint64_t *)m.cnt, count_out);
}

QRLSH_EXPORT int qrlsh_idmap_build(const uint32_t *ids, int64_t m, int64_t n, void *map, size_t map_bytes, uint64_t *out2,
                                   void *stream) {
  QR_CHECK_ARG(m >= 0 && n >= 0 && n < (1ll << 32) - 1, "qrlsh_idmap_build: bad sizes m=%lld n=%lld", (long long)m,
               (long long)n);
  QR_CHECK_ARG(map && out2 && (m == 0 || ids), "qrlsh_idmap_build: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_idmap_build", map, map_bytes, qrlsh_idmap_workspace_bytes(n));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const IdMap w = idmap_layout(map, n);
  QR_MEMSET("qrlsh_idmap_build", w.w, 0, (size_t)(w.nw + 1) * 8, st);
  QR_MEMSET("qrlsh_idmap_build", out2, 0, 2 * sizeof(uint64_t), st);
  if (m > 0)
    QR_LAUNCH("idmap_mark", idmap_mark_kernel, dim3(rm_grid(m, RM_THREADS)), dim3(RM_THREADS), 0, st, ids, m, n, w.w, out2);
  idmap_finish(w, out2, st);
  QR_LAUNCH_CHECK("qrlsh_idmap_build");
  return QRLSH_OK;
}

__global__ __launch_bounds__(RM_THREADS) void idmap_list_kernel(const uint2 *__restrict__ map, int64_t nw,
                                                               uint32_t *__restrict__ ids_out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nw) return;
  const uint2 e = map[w];
  uint32_t m = e.x;
  uint64_t at = e.y;
  while (m) {
    const int bit = __ffs((int)m) - 1;
    ids_out[at++] = (uint32_t)(w * 32 + bit);
    m &= m - 1;
  }
}

QRLSH_EXPORT int qrlsh_idmap_list(const void *map, int64_t n, uint32_t *ids_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && map, "qrlsh_idmap_list: bad arguments");
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(ids_out, "qrlsh_idmap_list: null ids_out");
  const IdMap w = idmap_layout(map, n);
  QR_LAUNCH("idmap_list", idmap_list_kernel, dim3((unsigned)ceil_div64(w.nw, RM_THREADS)), dim3(RM_THREADS), 0,
            static_cast<hipStream_t>(stream), (const uint2 *)w.w, w.nw, ids_out);
  QR_LAUNCH_CHECK("qrlsh_idmap_list");
  return QRLSH_OK;
}

// pos_out[i] = the rank of i among the ids outside the map, or -1 for a member
__global__ __launch_bounds__(RM_THREADS) void idmap_positions_kernel(const uint2 *__restrict__ map, int64_t n,
                                                                    int64_t *__restrict__ pos_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint2 w = map[i >> 5];
    pos_out[i] = idmap_has(w, (uint32_t)i) ? -1 : i - (int64_t)idmap_rank(w, (uint32_t)i);
  }
}

QRLSH_EXPORT int qrlsh_idmap_positions(const void *map, int64_t n, int64_t *pos_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && map, "qrlsh_idmap_positions: bad arguments");
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(pos_out, "qrlsh_idmap_positions: null pos_out");
  const IdMap w = idmap_layout(map, n);
  QR_LAUNCH("idmap_positions", idmap_positions_kernel, dim3(rm_grid(n, RM_THREADS)), dim3(RM_THREADS), 0,
            static_cast<hipStream_t>(stream), (const uint2 *)w.w, n, pos_out);
  QR_LAUNCH_CHECK("qrlsh_idmap_positions");
  return QRLSH_OK;
}

// ---- rows -----------------------------------------------------------------------------------------------------------
// one lane per piece of a row; V = the widest vector that divides the row (16 bytes for every width the hot path makes)
template <typename V>
__global__ __launch_bounds__(RM_THREADS) void rows_remove_kernel(const V *__restrict__ rows, int64_t chunks,
                                                                const int64_t *__restrict__ norm2, int64_t n,
                                                                const uint2 *__restrict__ rm, V *__restrict__ rows_out,
                                                                int64_t *__restrict__ norm2_out) {
  const int64_t all = n * chunks;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < all; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = g / chunks, c = g - i * chunks;
    const uint2 w = rm[i >> 5];
    if (idmap_has(w, (uint32_t)i)) continue;
    const int64_t o = i - (int64_t)idmap_rank(w, (uint32_t)i);
    rows_out[o * chunks + c] = rows[g];
    if (c == 0 && norm2) norm2_out[o] = norm2[i];
  }
}

template <typename V>
static void rows_remove_launch(const void *rows, int64_t row_bytes, const int64_t *norm2, int64_t n, const uint2 *rm,
                               void *rows_out, int64_t *norm2_out, hipStream_t st) {
  const int64_t chunks = row_bytes / (int64_t)sizeof(V);
  QR_LAUNCH("rows_remove", rows_remove_kernel<V>, dim3(rm_grid(n * chunks, RM_THREADS)), dim3(RM_THREADS), 0, st,
            static_cast<const V *>(rows), chunks, norm2, n, rm, static_cast<V *>(rows_out), norm2_out);
}

QRLSH_EXPORT int qrlsh_rows_remove(const void *rows, int64_t row_bytes, const int64_t *norm2, int64_t n,
                                   const void *removed_map, void *rows_out, int64_t *norm2_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && row_bytes > 0 && row_bytes % 2 == 0,
               "qrlsh_rows_remove: bad sizes n=%lld row_bytes=%lld (a multiple of 2)", (long long)n, (long long)row_bytes);
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(rows && removed_map && rows_out && (!norm2 || norm2_out), "qrlsh_rows_remove: null pointer");
  QR_CHECK_ALIGNED("qrlsh_rows_remove", "rows", qr_addr(rows) | qr_addr(rows_out), 16);
  const uint2 *rm = idmap_layout(removed_map, n).w;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // every row starts on a multiple of its width from a 16-byte aligned base: the widest vector that divides the width
  if (row_bytes % 16 == 0) rows_remove_launch<uint4>(rows, row_bytes, norm2, n, rm, rows_out, norm2_out, st);
  else if (row_bytes % 8 == 0) rows_remove_launch<uint2>(rows, row_bytes, norm2, n, rm, rows_out, norm2_out, st);
  else if (row_bytes % 4 == 0) rows_remove_launch<uint32_t>(rows, row_bytes, norm2, n, rm, rows_out, norm2_out, st);
  else rows_remove_launch<uint16_t>(rows, row_bytes, norm2, n, rm, rows_out, norm2_out, st);
  QR_LAUNCH_CHECK("qrlsh_rows_remove");
  return QRLSH_OK;
}

// ---- index ----------------------------------------------------------------------------------------------------------
// one workgroup per (tile, band).  count: tile_off[band * tiles + tile] = survivors of the tile.  fill: tile_off is the
// exclusive scan of those counts = the tile's first position in the flat [b][n_out] output.
template <bool FILL>
__global__ __launch_bounds__(RM_THREADS) void index_remove_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ ids, int64_t n, int64_t n_out, int64_t total_out,
    const uint2 *__restrict__ rm, const uint2 *__restrict__ pick, int64_t n_pick, uint64_t *__restrict__ tile_off,
    uint64_t *__restrict__ keys_out, uint32_t *__restrict__ ids_out, uint64_t *__restrict__ pick_keys_out) {
  __shared__ uint32_t wc[RM_PER * 4];
  const int64_t t = blockIdx.y, tile = blockIdx.x;
  const int64_t o = tile * RM_TILE;
  const uint32_t *bi = ids + t * n;
  const uint64_t *bk = keys + t * n;
  uint32_t id[RM_PER];
  uint64_t key[RM_PER];
  uint2 w[RM_PER];
  bool keep[RM_PER];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {  // every load of the tile is issued before the first is used
    const int64_t x = o + (int64_t)k * RM_THREADS + threadIdx.x;
    id[k] = x < n ? bi[x] : 0xFFFFFFFFu;
    key[k] = FILL && x < n ? bk[x] : 0;
  }
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const bool ok = (int64_t)id[k] < n;  // false past the band's end (and for an id no build writes)
    w[k] = ok ? rm[id[k] >> 5] : make_uint2(0u, 0u);
    keep[k] = ok && !idmap_has(w[k], id[k]);
  }
  uint32_t before[RM_PER];
  const uint32_t kept = rm_tile_prefix(keep, wc, before);
  if (!FILL) {
    if (threadIdx.x == 0) tile_off[t * gridDim.x + tile] = kept;
    return;
  }
  const uint64_t base = tile_off[t * gridDim.x + tile];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    if (!keep[k]) continue;
    const int64_t pos = (int64_t)(base + before[k]);
    if (pos < total_out) {  // always, for a band that holds every id once
      keys_out[pos] = key[k];
      ids_out[pos] = id[k] - idmap_rank(w[k], id[k]);
    }
    if (pick) {
      const uint2 pw = pick[id[k] >> 5];
      const int64_t j = idmap_rank(pw, id[k]);
      if (idmap_has(pw, id[k]) && j < n_pick) pick_keys_out[t * n_pick + j] = key[k];
    }
  }
  (void)n_out;
}

// workspace: tile counts / offsets u64 [b * tiles + 1] | scan sums
struct IrWs {
  uint64_t *tile_off, *sums;
};
static IrWs ir_layout(QrCarve &c, int64_t n, int32_t b) {
  const int64_t all = ceil_div64(n, RM_TILE) * b;
  IrWs w;
  w.tile_off = c.take<uint64_t>((size_t)(all + 1));
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(all, SCANL_CHUNK) + 1));
  return w;
}
QRLSH_EXPORT size_t qrlsh_index_remove_workspace_bytes(int64_t n, int32_t b) {
  if (n <= 0 || b <= 0) return 0;
  return QR_LAYOUT_BYTES(ir_layout, n, b);
}

QRLSH_EXPORT int qrlsh_index_remove(const uint64_t *keys, const uint32_t *ids, int64_t n, int32_t b, const void *removed_map,
                                    int64_t n_removed, const void *pick_map, int64_t n_pick, uint64_t *keys_out,
                                    uint32_t *ids_out, uint32_t *dir_out, uint64_t *pick_keys_out, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && b > 0 && b <= 65535 && n_removed >= 0 && n_removed <= n && n_pick >= 0 &&
                   n_pick <= n - n_removed,
               "qrlsh_index_remove: bad sizes n=%lld b=%d n_removed=%lld n_pick=%lld", (long long)n, b, (long long)n_removed,
               (long long)n_pick);
  if (n_removed == 0 || n_removed == n) return QRLSH_OK;  // nothing leaves / nothing stays: the outputs are not written
  QR_CHECK_ARG(keys && ids && removed_map && keys_out && ids_out && dir_out && workspace &&
                   (n_pick == 0 || (pick_map && pick_keys_out)),
               "qrlsh_index_remove: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_index_remove", workspace, workspace_bytes, qrlsh_index_remove_workspace_bytes(n, b));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_out = n - n_removed, tiles = ceil_div64(n, RM_TILE), all = tiles * b;
  QrCarve c(workspace);
  const IrWs w = ir_layout(c, n, b);
  uint64_t *tile_off = w.tile_off, *sums = w.sums;
  const uint2 *rm = idmap_layout(removed_map, n).w;
  const uint2 *pk = n_pick > 0 ? idmap_layout(pick_map, n).w : nullptr;
  const dim3 grid((unsigned)tiles, (unsigned)b), block(RM_THREADS);
  QR_LAUNCH("index_remove_count", index_remove_kernel<false>, grid, block, 0, st, keys, ids, n, n_out, n_out * b, rm, pk,
            n_pick, tile_off, keys_out, ids_out, pick_keys_out);
  qr_scan_u64(tile_off, all, tile_off + all, sums, st);
  QR_LAUNCH("index_remove_fill", index_remove_kernel<true>, grid, block, 0, st, keys, ids, n, n_out, n_out * b, rm, pk,
            n_pick, tile_off, keys_out, ids_out, pick_keys_out);
  return qr_index_dir(keys_out, n_out, b, dir_out, st, "qrlsh_index_remove");
}

// ---- lists ----------------------------------------------------------------------------------------------------------
// one lane per stored entry whose dst is removed and whose src stays: a row of exactly K entries enters the pick map
__global__ __launch_bounds__(RM_THREADS) void lists_remove_mark_kernel(const int32_t *__restrict__ src,
                                                                      const int32_t *__restrict__ dst, int64_t n_edges,
                                                                      int64_t n, int K, const uint2 *__restrict__ rm,
                                                                      uint2 *__restrict__ pick,
                                                                      uint64_t *__restrict__ out2) {
  bool wrong = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = src[e], d = dst[e];
    const int64_t sp = e > 0 ? (int64_t)src[e - 1] : -1;
    if (s < 0 || s >= n || d < 0 || d >= n || sp > s) {
      wrong = true;
      continue;
    }
    if (!idmap_has(rm[d >> 5], (uint32_t)d) || idmap_has(rm[s >> 5], (uint32_t)s)) continue;
    int64_t L = 0, R = e;  // the row's first entry
    while (L < R) {
      const int64_t mid = L + (R - L) / 2;
      if ((int64_t)src[mid] < s) L = mid + 1;
      else R = mid;
    }
    if (L + K - 1 < n_edges && (int64_t)src[L + K - 1] == s) idmap_set(pick, (uint32_t)s);
  }
  if (__ballot(wrong) && lane_id() == 0) atomicOr(reinterpret_cast<unsigned long long *>(out2 + 1), ~0ull);
}

QRLSH_EXPORT int qrlsh_lists_remove_mark(const int32_t *src, const int32_t *dst, int64_t n_edges, int64_t n, int32_t K,
                                         const void *removed_map, void *pick_map_out, uint64_t *out2, void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= RM_MAXK, "qrlsh_lists_remove_mark: K=%d not in [1, %d]", K, RM_MAXK);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31),
               "qrlsh_lists_remove_mark: n=%lld and n_edges=%lld must stay below 2^31", (long long)n, (long long)n_edges);
  QR_CHECK_ARG(removed_map && pick_map_out && out2 && (n_edges == 0 || (src && dst)), "qrlsh_lists_remove_mark: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const IdMap pk = idmap_layout(pick_map_out, n);
  QR_MEMSET("qrlsh_lists_remove_mark", pk.w, 0, (size_t)(pk.nw + 1) * 8, st);
  QR_MEMSET("qrlsh_lists_remove_mark", out2, 0, 2 * sizeof(uint64_t), st);
  if (n_edges > 0)
    QR_LAUNCH("lists_remove_mark", lists_remove_mark_kernel, dim3(rm_grid(n_edges, RM_THREADS)), dim3(RM_THREADS), 0, st, src,
              dst, n_edges, n, (int)K, (const uint2 *)idmap_layout(removed_map, n).w, pk.w, out2);
  idmap_finish(pk, out2, st);
  QR_LAUNCH_CHECK("qrlsh_lists_remove_mark");
  return QRLSH_OK;
}

struct LrWs {
  uint64_t *tile_off, *sums, *pick_base;
  uint32_t *bad;
  int64_t tiles, rows;
};
static LrWs lr_layout(QrCarve &c, int64_t n, int64_t n_edges) {
  LrWs w;
  w.tiles = ceil_div64(n_edges, RM_TILE);
  w.rows = n < n_edges ? n : n_edges;  // no more picked rows than rows, or than entries
  w.tile_off = c.take<uint64_t>((size_t)(w.tiles + 1));
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(w.tiles, SCANL_CHUNK) + 1));
  w.pick_base = c.take<uint64_t>((size_t)w.rows);
  w.bad = c.take<uint32_t>(4);
  return w;
}

QRLSH_EXPORT size_t qrlsh_lists_remove_workspace_bytes(int64_t n, int64_t n_edges) {
  if (n < 0 || n_edges < 0) return 0;
  return QR_LAYOUT_BYTES(lr_layout, n, n_edges);
}

// one workgroup per tile of stored entries.  An entry is kept when its src and dst stay and its row is not picked.
// count: tile_off[tile] = kept entries.  fill: a kept entry goes to (kept entries before it) + (re-probed entries of the
// picked rows below its src); the first entry of a picked row leaves pick_base[j] = that sum for the row itself.
template <bool FILL>
__global__ __launch_bounds__(RM_THREADS) void lists_remove_kernel(
    const int32_t *__restrict__ src, const int32_t *__restrict__ dst, const int32_t *__restrict__ val, int64_t n_edges,
    int64_t n, const uint2 *__restrict__ rm, const uint2 *__restrict__ pick, const int64_t *__restrict__ re_off,
    int64_t n_pick, uint64_t *__restrict__ tile_off, uint32_t *__restrict__ bad, int64_t total,
    uint64_t *__restrict__ pick_base, int32_t *__restrict__ src_out, int32_t *__restrict__ dst_out,
    int32_t *__restrict__ val_out) {
  __shared__ uint32_t wc[RM_PER * 4];
  const int64_t o = (int64_t)blockIdx.x * RM_TILE;
  int32_t s[RM_PER], d[RM_PER], v[RM_PER], sp[RM_PER];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const int64_t e = o + (int64_t)k * RM_THREADS + threadIdx.x;
    const bool live = e < n_edges;
    s[k] = live ? src[e] : -1;
    d[k] = live ? dst[e] : -1;
    v[k] = FILL && live ? val[e] : 0;
    sp[k] = live && e > 0 ? src[e - 1] : -1;
  }
  uint2 ws[RM_PER], wd[RM_PER], wp[RM_PER];
  bool keep[RM_PER], head[RM_PER];
  bool wrong = false;
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const int64_t e = o + (int64_t)k * RM_THREADS + threadIdx.x;
    const bool ok = e < n_edges && s[k] >= 0 && s[k] < n && d[k] >= 0 && d[k] < n && sp[k] <= s[k];
    wrong |= e < n_edges && !ok;
    ws[k] = ok ? rm[s[k] >> 5] : make_uint2(0u, 0u);
    wd[k] = ok ? rm[d[k] >> 5] : make_uint2(0u, 0u);
    wp[k] = ok && pick ? pick[s[k] >> 5] : make_uint2(0u, 0u);
    const bool picked = ok && idmap_has(wp[k], (uint32_t)s[k]);
    keep[k] = ok && !picked && !idmap_has(ws[k], (uint32_t)s[k]) && !idmap_has(wd[k], (uint32_t)d[k]);
    head[k] = picked && sp[k] != s[k];
  }
  uint32_t before[RM_PER];
  const uint32_t kept = rm_tile_prefix(keep, wc, before);
  if (!FILL) {
    if (threadIdx.x == 0) tile_off[blockIdx.x] = kept;
    if (__ballot(wrong) && lane_id() == 0) atomicOr(bad, 1u);
    return;
  }
  const uint64_t base = tile_off[blockIdx.x];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    if (!keep[k] && !head[k]) continue;
    const int64_t j = idmap_rank(wp[k], (uint32_t)s[k]);  // picked rows below src
    if (j > n_pick) continue;                             // never, for the pick map of these lists
    const int64_t at = (int64_t)(base + before[k]) + (n_pick > 0 ? re_off[j] : 0);
    if (head[k]) {
      if (j < n_pick) pick_base[j] = (uint64_t)at;
      continue;
    }
    if (at >= total) continue;  // never, for the total the count gave
    src_out[at] = s[k] - (int32_t)idmap_rank(ws[k], (uint32_t)s[k]);
    dst_out[at] = d[k] - (int32_t)idmap_rank(wd[k], (uint32_t)d[k]);
    val_out[at] = v[k];
  }
}

// *total_out = kept stored entries + re-probed entries, or ~0 when the stored lists break the contract
__global__ void lists_remove_total_kernel(const uint64_t *__restrict__ kept, const int64_t *__restrict__ re_off,
                                          int64_t n_pick, const uint32_t *__restrict__ bad,
                                          uint64_t *__restrict__ total_out) {
  if (threadIdx.x == 0) *total_out = *bad ? ~0ull : *kept + (n_pick > 0 ? (uint64_t)re_off[n_pick] : 0ull);
}

static int lr_args(const char *who, const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                   int32_t K, const void *removed_map, const void *pick_map, const int64_t *re_off, int64_t n_pick,
                   const void *workspace, size_t workspace_bytes) {
  QR_CHECK_ARG(K >= 1 && K <= RM_MAXK, "%s: K=%d not in [1, %d]", who, K, RM_MAXK);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31) && n_pick >= 0 && n_pick <= n &&
                   n_pick <= n_edges,
               "%s: n=%lld and n_edges=%lld must stay below 2^31, n_pick=%lld below both", who, (long long)n,
               (long long)n_edges, (long long)n_pick);
  QR_CHECK_ARG(removed_map && workspace && (n_edges == 0 || (src && dst && val)) && (n_pick == 0 || (pick_map && re_off)),
               "%s: null pointer", who);
  QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, qrlsh_lists_remove_workspace_bytes(n, n_edges));
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_lists_remove_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                          int64_t n, int32_t K, const void *removed_map, const void *pick_map,
                                          const int64_t *re_off, int64_t n_pick, void *workspace, size_t workspace_bytes,
                                          uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(total_out, "qrlsh_lists_remove_count: null total_out");
  const int rc = lr_args("qrlsh_lists_remove_count", src, dst, val, n_edges, n, K, removed_map, pick_map, re_off, n_pick,
                         workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  const LrWs w = lr_layout(c, n, n_edges);
  QR_MEMSET("qrlsh_lists_remove_count", w.bad, 0, 16, st);
  QR_MEMSET("qrlsh_lists_remove_count", w.tile_off, 0, sizeof(uint64_t), st);
  if (w.rows > 0) QR_MEMSET("qrlsh_lists_remove_count", w.pick_base, 0, (size_t)w.rows * 8, st);
  if (n_edges > 0) {
    const uint2 *rm = idmap_layout(removed_map, n).w;
    const uint2 *pk = n_pick > 0 ? idmap_layout(pick_map, n).w : nullptr;
    QR_LAUNCH("lists_remove_count", lists_remove_kernel<false>, dim3((unsigned)w.tiles), dim3(RM_THREADS), 0, st, src, dst,
              val, n_edges, n, rm, pk, re_off, n_pick, w.tile_off, w.bad, (int64_t)0, w.pick_base, nullptr, nullptr, nullptr);
    qr_scan_u64(w.tile_off, w.tiles, w.tile_off + w.tiles, w.sums, st);
  }
  QR_LAUNCH("lists_remove_total", lists_remove_total_kernel, dim3(1), dim3(64), 0, st,
            (const uint64_t *)(w.tile_off + w.tiles), re_off, n_pick, (const uint32_t *)w.bad, total_out);
  QR_LAUNCH_CHECK("qrlsh_lists_remove_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_lists_remove_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                         int64_t n, int32_t K, const void *removed_map, const void *pick_map,
                                         const int64_t *re_off, const int32_t *re_idx, const int32_t *re_milli,
                                         const uint32_t *re_self, int64_t n_pick, void *workspace, size_t workspace_bytes,
                                         int64_t total, int32_t *src_out, int32_t *dst_out, int32_t *val_out, void *stream) {
  const int rc = lr_args("qrlsh_lists_remove_fill", src, dst, val, n_edges, n, K, removed_map, pick_map, re_off, n_pick,
                         workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(total >= 0 && total <= n_edges + n_pick * (int64_t)K, "qrlsh_lists_remove_fill: bad total %lld",
               (long long)total);
  if (total == 0) return QRLSH_OK;
  QR_CHECK_ARG(src_out && dst_out && val_out && (n_pick == 0 || re_self), "qrlsh_lists_remove_fill: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  const LrWs w = lr_layout(c, n, n_edges);
  if (n_edges > 0) {
    const uint2 *rm = idmap_layout(removed_map, n).w;
    const uint2 *pk = n_pick > 0 ? idmap_layout(pick_map, n).w : nullptr;
    QR_LAUNCH("lists_remove_fill", lists_remove_kernel<true>, dim3((unsigned)w.tiles), dim3(RM_THREADS), 0, st, src, dst, val,
              n_edges, n, rm, pk, re_off, n_pick, w.tile_off, w.bad, total, w.pick_base, src_out, dst_out, val_out);
  }
  // the re-probed lists: list j at pick_base[j], src = the row's new id
  qr_lists_fill_probed(re_off, re_idx, re_milli, re_self, 0, n_pick, (int)K, w.pick_base, n_pick, false, total, src_out,
                       dst_out, val_out, st);
  QR_LAUNCH_CHECK("qrlsh_lists_remove_fill");
  return QRLSH_OK;
}
