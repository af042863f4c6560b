// listcut.hip -- the list length of the stored top-K lists changes in place: a cut to a smaller K, and the two passes a
// regrow to a larger K needs before the probe.
//
// Stored lists are COO src / dst / val ordered by src, then value descending, then dst ascending, at most K_old per src.
// The first c entries of a row are therefore the row a run with K = c would have stored, and entry i of the flat lists
// survives a cut to K_new exactly when
//
//        i < K_new  ||  src[i - K_new] != src[i]
//
// (the entry K_new places back belongs to another row <=> fewer than K_new entries of its own row precede it).  That is a
// stream compaction with a predicate on src alone: no row bounds, no ranks, no per-row work.
//
//   cut:    count: one workgroup per tile of LC_TILE entries loads its src as 16-byte vectors, puts them into LDS behind a
//           halo of the max(K_old, K_new) entries before the tile (rows straddle tiles: the predicate looks back across
//           the tile's start), evaluates the predicate and leaves the tile's survivors in tile_off; the same pass checks
//           the contract (src ascending and inside [0, n), no row longer than K_old: src[i - K_old] == src[i]).  One scan.
//           fill: the same tile image again, a wave scan of the per-vector survivor counts gives every vector its place,
//           dst / val are loaded (16 bytes) only for vectors that hold a survivor; the survivors meet in LDS in output
//           order and leave as consecutive words per lane, every output written once (a lane storing its own four
//           entries 16 bytes from its neighbour's took 0.41 ms where this takes 0.27 at 65.5 M entries).
//           No atomic on a shared cursor, no serial walk of a row, no scratch.
//   regrow: mark: the rows that may be missing candidates are those of exactly K_old entries -- entry i is the head of one
//           iff it is a run head and src[i + K_old - 1] == src[i].  They enter an id map (remove.hip's layout).
//           pick keys: per band, a record whose id is in that map writes its key to pick_keys_out[band][rank(id)]: the
//           probe keys of the picked rows, taken from the index itself (qrlsh_index_remove writes them only on its way
//           through a removal).
//           The substitution of the probed lists for the picked rows is the removal's own count / fill with an empty
//           removed map (qrlsh_lists_remove_*: every stored entry read once, every entry places itself).
#include "idmap.h"

constexpr int LC_THREADS = 256;
constexpr int LC_VEC = 2;                           // 16-byte vectors per lane, LC_THREADS vectors apart
constexpr int LC_TILE = LC_THREADS * LC_VEC * 4;    // entries per workgroup
constexpr int LC_HALO = RM_MAXK;                    // entries before the tile that the predicate may look at
static_assert(LC_HALO == LC_THREADS, "one lane loads one halo entry");

struct LcWs {
  uint64_t *tile_off, *sums;
  uint32_t *bad;
  int64_t tiles;
};
static LcWs lc_layout(QrCarve &c, int64_t n_edges) {
  LcWs w;
  w.tiles = ceil_div64(n_edges, LC_TILE);
  w.tile_off = c.take<uint64_t>((size_t)(w.tiles + 1));
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(w.tiles, SCANL_CHUNK) + 1));
  w.bad = c.take<uint32_t>(4);
  return w;
}

QRLSH_EXPORT size_t qrlsh_lists_cut_workspace_bytes(int64_t n_edges) {
  if (n_edges < 0) return 0;
  return QR_LAYOUT_BYTES(lc_layout, n_edges);
}

// four consecutive entries from e on; past the end: -1 (no id)
__device__ static inline int4 lc_load4(const int32_t *__restrict__ a, int64_t e, int64_t n_edges) {
  if (e + 3 < n_edges) return *reinterpret_cast<const int4 *>(a + e);
  int4 v;
  v.x = e < n_edges ? a[e] : -1;
  v.y = e + 1 < n_edges ? a[e + 1] : -1;
  v.z = e + 2 < n_edges ? a[e + 2] : -1;
  v.w = e + 3 < n_edges ? a[e + 3] : -1;
  return v;
}

// count: tile_off[tile] = survivors of the tile, *bad |= 1 on a contract break.  fill: tile_off = the exclusive scan.
template <bool FILL>
__global__ __launch_bounds__(LC_THREADS) void lists_cut_kernel(
    const int32_t *__restrict__ src, const int32_t *__restrict__ dst, const int32_t *__restrict__ val, int64_t n_edges,
    int64_t n, int K_old, int K_new, uint64_t *__restrict__ tile_off, uint32_t *__restrict__ bad, int64_t total,
    int32_t *__restrict__ src_out, int32_t *__restrict__ dst_out, int32_t *__restrict__ val_out) {
  __shared__ __attribute__((aligned(16))) int32_t s[LC_HALO + LC_TILE];
  __shared__ uint32_t wc[LC_VEC * 4];
  __shared__ int32_t sd[FILL ? LC_TILE : 1], sv_[FILL ? LC_TILE : 1];  // the fill's surviving dst / val in output order
  const int t = threadIdx.x, lane = lane_id(), wave = t >> 6;
  const int64_t o = (int64_t)blockIdx.x * LC_TILE;
  int4 mine[LC_VEC];
#pragma unroll
  for (int k = 0; k < LC_VEC; ++k) mine[k] = lc_load4(src, o + ((int64_t)k * LC_THREADS + t) * 4, n_edges);
  {
    const int back = K_old > K_new ? K_old : K_new;  // <= LC_HALO
    const int64_t e = o - LC_HALO + t;
    s[t] = t >= LC_HALO - back && e >= 0 ? src[e] : -1;  // -1 before the lists' start: equal to no id
  }
#pragma unroll
  for (int k = 0; k < LC_VEC; ++k) *reinterpret_cast<int4 *>(&s[LC_HALO + (k * LC_THREADS + t) * 4]) = mine[k];
  __syncthreads();
  uint32_t mask[LC_VEC], cnt[LC_VEC];
  bool wrong = false;
#pragma unroll
  for (int k = 0; k < LC_VEC; ++k) {
    const int j0 = LC_HALO + (k * LC_THREADS + t) * 4;
    const int32_t v[4] = {mine[k].x, mine[k].y, mine[k].z, mine[k].w};
    mask[k] = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + c;
      const int64_t i = o + (j - LC_HALO);
      if (i >= n_edges) continue;
      if (!FILL) wrong |= v[c] < 0 || v[c] >= n || s[j - 1] > v[c] || s[j - K_old] == v[c];
      if (i < K_new || s[j - K_new] != v[c]) mask[k] |= 1u << c;
    }
    cnt[k] = (uint32_t)__popc(mask[k]);
  }
  uint32_t inc[LC_VEC], before[LC_VEC];
#pragma unroll
  for (int k = 0; k < LC_VEC; ++k) {
    inc[k] = wave_incl_scan(cnt[k]);
    if (lane == WAVE - 1) wc[k * 4 + wave] = inc[k];
  }
  __syncthreads();
  uint32_t run = 0;
#pragma unroll
  for (int k = 0; k < LC_VEC; ++k)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave) before[k] = run + inc[k] - cnt[k];
      run += wc[k * 4 + w];
    }
  if (!FILL) {
    if (t == 0) tile_off[blockIdx.x] = run;
    if (__ballot(wrong) && lane == 0) atomicOr(bad, 1u);
    return;
  }
  // the survivors meet in LDS in output order (every read of the tile image is behind the barrier above), then leave as
  // consecutive words per lane
  const int64_t base = (int64_t)tile_off[blockIdx.x];
#pragma unroll
  for (int k = 0; k < LC_VEC; ++k) {
    if (!mask[k]) continue;
    const int64_t e = o + ((int64_t)k * LC_THREADS + t) * 4;
    const int4 d4 = lc_load4(dst, e, n_edges), v4 = lc_load4(val, e, n_edges);
    const int32_t sv[4] = {mine[k].x, mine[k].y, mine[k].z, mine[k].w};
    const int32_t dv[4] = {d4.x, d4.y, d4.z, d4.w};
    const int32_t vv[4] = {v4.x, v4.y, v4.z, v4.w};
    uint32_t at = before[k];  // < LC_TILE
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!((mask[k] >> c) & 1u)) continue;
      s[at] = sv[c];
      sd[at] = dv[c];
      sv_[at] = vv[c];
      ++at;
    }
  }
  __syncthreads();
  for (uint32_t r = t; r < run; r += LC_THREADS) {
    const int64_t at = base + r;
    if (at >= total) break;  // never, for the total the count gave
    src_out[at] = s[r];
    dst_out[at] = sd[r];
    val_out[at] = sv_[r];
  }
}

// *total_out = the survivors, or ~0 when the stored lists break the contract
__global__ void lists_cut_total_kernel(const uint64_t *__restrict__ kept, const uint32_t *__restrict__ bad,
                                       uint64_t *__restrict__ total_out) {
  if (threadIdx.x == 0) *total_out = *bad ? ~0ull : *kept;
}

static int lc_args(const char *who, const int32_t *src, int64_t n_edges, int64_t n, int32_t K_old, int32_t K_new,
                   const void *workspace, size_t workspace_bytes) {
  QR_CHECK_ARG(K_old >= 1 && K_old <= RM_MAXK && K_new >= 1 && K_new <= RM_MAXK, "%s: K_old=%d, K_new=%d not in [1, %d]",
               who, K_old, K_new, RM_MAXK);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31),
               "%s: n=%lld and n_edges=%lld must stay below 2^31", who, (long long)n, (long long)n_edges);
  QR_CHECK_ARG(workspace && (n_edges == 0 || src), "%s: null pointer", who);
  QR_CHECK_ALIGNED(who, "the lists", qr_addr(src), 16);
  QR_CHECK_ARG(workspace_bytes >= qrlsh_lists_cut_workspace_bytes(n_edges), "%s: workspace %zu < %zu bytes", who,
               workspace_bytes, qrlsh_lists_cut_workspace_bytes(n_edges));
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_lists_cut_count(const int32_t *src, int64_t n_edges, int64_t n, int32_t K_old, int32_t K_new,
                                       void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(total_out, "qrlsh_lists_cut_count: null total_out");
  const int rc = lc_args("qrlsh_lists_cut_count", src, n_edges, n, K_old, K_new, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  const LcWs w = lc_layout(c, n_edges);
  QR_MEMSET("qrlsh_lists_cut_count", w.bad, 0, 16, st);
  QR_MEMSET("qrlsh_lists_cut_count", w.tile_off, 0, sizeof(uint64_t), st);
  if (n_edges > 0) {
    QR_LAUNCH("lists_cut_count", lists_cut_kernel<false>, dim3((unsigned)w.tiles), dim3(LC_THREADS), 0, st, src,
              (const int32_t *)nullptr, (const int32_t *)nullptr, n_edges, n, (int)K_old, (int)K_new, w.tile_off, w.bad,
              (int64_t)0, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
    qr_scan_u64(w.tile_off, w.tiles, w.tile_off + w.tiles, w.sums, st);
  }
  QR_LAUNCH("lists_cut_total", lists_cut_total_kernel, dim3(1), dim3(64), 0, st, (const uint64_t *)(w.tile_off + w.tiles),
            (const uint32_t *)w.bad, total_out);
  QR_LAUNCH_CHECK("qrlsh_lists_cut_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_lists_cut_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                                      int32_t K_old, int32_t K_new, const void *workspace, size_t workspace_bytes,
                                      int64_t total, int32_t *src_out, int32_t *dst_out, int32_t *val_out, void *stream) {
  const int rc = lc_args("qrlsh_lists_cut_fill", src, n_edges, n, K_old, K_new, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(total >= 0 && total <= n_edges, "qrlsh_lists_cut_fill: bad total %lld", (long long)total);
  if (total == 0) return QRLSH_OK;
  QR_CHECK_ARG(dst && val && src_out && dst_out && val_out, "qrlsh_lists_cut_fill: null pointer");
  QR_CHECK_ALIGNED("qrlsh_lists_cut_fill", "the lists", qr_addr(dst) | qr_addr(val), 16);
  QrCarve c(workspace);
  const LcWs w = lc_layout(c, n_edges);
  QR_LAUNCH("lists_cut_fill", lists_cut_kernel<true>, dim3((unsigned)w.tiles), dim3(LC_THREADS), 0,
            static_cast<hipStream_t>(stream), src, dst, val, n_edges, n, (int)K_old, (int)K_new, w.tile_off, w.bad, total,
            src_out, dst_out, val_out);
  QR_LAUNCH_CHECK("qrlsh_lists_cut_fill");
  return QRLSH_OK;
}

// ---- regrow: the rows of exactly K_old entries -----------------------------------------------------------------------
// one lane per stored entry; a run head whose row reaches K_old entries enters the pick map
__global__ __launch_bounds__(RM_THREADS) void lists_regrow_mark_kernel(const int32_t *__restrict__ src, int64_t n_edges,
                                                                      int64_t n, int K_old, uint2 *__restrict__ pick,
                                                                      uint64_t *__restrict__ out2) {
  bool wrong = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = src[e];
    const int64_t sp = e > 0 ? (int64_t)src[e - 1] : -1;
    if (s < 0 || s >= n || sp > s) {
      wrong = true;
      continue;
    }
    if (sp == s) continue;  // not a run head
    if (e + K_old < n_edges && (int64_t)src[e + K_old] == s) wrong = true;  // a row longer than K_old
    else if (e + K_old - 1 < n_edges && (int64_t)src[e + K_old - 1] == s) idmap_set(pick, (uint32_t)s);
  }
  if (__ballot(wrong) && lane_id() == 0) atomicOr(reinterpret_cast<unsigned long long *>(out2 + 1), ~0ull);
}

QRLSH_EXPORT int qrlsh_lists_regrow_mark(const int32_t *src, int64_t n_edges, int64_t n, int32_t K_old, void *pick_map_out,
                                         uint64_t *out2, void *stream) {
  QR_CHECK_ARG(K_old >= 1 && K_old <= RM_MAXK, "qrlsh_lists_regrow_mark: K_old=%d not in [1, %d]", K_old, RM_MAXK);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31),
               "qrlsh_lists_regrow_mark: n=%lld and n_edges=%lld must stay below 2^31", (long long)n, (long long)n_edges);
  QR_CHECK_ARG(pick_map_out && out2 && (n_edges == 0 || src), "qrlsh_lists_regrow_mark: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const IdMap pk = idmap_layout(pick_map_out, n);
  QR_MEMSET("qrlsh_lists_regrow_mark", pk.w, 0, (size_t)(pk.nw + 1) * 8, st);
  QR_MEMSET("qrlsh_lists_regrow_mark", out2, 0, 2 * sizeof(uint64_t), st);
  if (n_edges > 0)
    QR_LAUNCH("lists_regrow_mark", lists_regrow_mark_kernel, dim3(rm_grid(n_edges, RM_THREADS)), dim3(RM_THREADS), 0, st, src,
              n_edges, n, (int)K_old, pk.w, out2);
  idmap_finish(pk, out2, st);
  QR_LAUNCH_CHECK("qrlsh_lists_regrow_mark");
  return QRLSH_OK;
}

// ---- regrow: the keys the picked rows are indexed under ---------------------------------------------------------------
// grid.y = band; keys are read for the picked records only
__global__ __launch_bounds__(RM_THREADS) void index_pick_keys_kernel(const uint64_t *__restrict__ keys,
                                                                    const uint32_t *__restrict__ ids, int64_t n,
                                                                    const uint2 *__restrict__ pick, int64_t n_pick,
                                                                    uint64_t *__restrict__ pick_keys_out) {
  const int64_t band = blockIdx.y;
  const uint32_t *bi = ids + band * n;
  const uint64_t *bk = keys + band * n;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t id = bi[x];
    if ((int64_t)id >= n) continue;  // an id no build writes
    const uint2 pw = pick[id >> 5];
    if (!idmap_has(pw, id)) continue;
    const int64_t j = idmap_rank(pw, id);
    if (j < n_pick) pick_keys_out[band * n_pick + j] = bk[x];
  }
}

QRLSH_EXPORT int qrlsh_index_pick_keys(const uint64_t *keys, const uint32_t *ids, int64_t n, int32_t b, const void *pick_map,
                                       int64_t n_pick, uint64_t *pick_keys_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && b > 0 && b <= 65535 && n_pick >= 0 && n_pick <= n,
               "qrlsh_index_pick_keys: bad sizes n=%lld b=%d n_pick=%lld", (long long)n, b, (long long)n_pick);
  if (n_pick == 0) return QRLSH_OK;
  QR_CHECK_ARG(keys && ids && pick_map && pick_keys_out, "qrlsh_index_pick_keys: null pointer");
  const uint2 *pk = idmap_layout(pick_map, n).w;
  QR_LAUNCH("index_pick_keys", index_pick_keys_kernel, dim3(rm_grid(n, RM_THREADS), (unsigned)b), dim3(RM_THREADS), 0,
            static_cast<hipStream_t>(stream), keys, ids, n, pk, n_pick, pick_keys_out);
  QR_LAUNCH_CHECK("qrlsh_index_pick_keys");
  return QRLSH_OK;
}
