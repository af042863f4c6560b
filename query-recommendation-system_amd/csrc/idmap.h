// idmap.h -- what the kernels that take queries out of a built index (remove.hip) and put others in their place
// (replace.hip) share, and the list merge (lists.hip) with them: the tile geometry of their compactions, the capped
// grid of the grid-stride kernels, the id map, and the stable compaction of a tile.
#pragma once
#include "common.h"

constexpr int RM_THREADS = 256;
constexpr int RM_PER = 8;                       // records (list entries) per lane, RM_THREADS apart
constexpr int RM_TILE = RM_THREADS * RM_PER;    // records per workgroup: qrlsh/_lib.py REMOVE_TILE
constexpr int RM_GRID = 2048;                   // workgroups of the grid-stride kernels (256 CUs x 8)
constexpr int RM_MAXK = QRLSH_INDEX_MAX_K;

static inline unsigned rm_grid(int64_t work, int64_t per_block) {
  const int64_t g = ceil_div64(work, per_block);
  return (unsigned)(g < RM_GRID ? (g > 0 ? g : 1) : RM_GRID);
}

// ---- id map ---------------------------------------------------------------------------------------------------------
// words uint2 [nw + 1] {bits, members below the word} (entry nw: no bits, the member count) | popcounts u64 [nw + 2] |
// scan scratch           (nw = ceil(n / 32))
struct IdMap {
  uint2 *w;
  uint64_t *cnt, *sums;
  int64_t nw;
};
static IdMap idmap_layout(QrCarve &c, int64_t n) {
  IdMap m;
  m.nw = (n + 31) / 32;
  m.w = c.take<uint2>((size_t)(m.nw + 1));
  m.cnt = c.take<uint64_t>((size_t)(m.nw + 2));
  m.sums = c.take<uint64_t>((size_t)(ceil_div64(m.nw + 1, SCANL_CHUNK) + 2));
  return m;
}
static IdMap idmap_layout(const void *map, int64_t n) {
  QrCarve c(map);
  return idmap_layout(c, n);
}

__device__ static inline bool idmap_has(uint2 w, uint32_t id) { return (w.x >> (id & 31u)) & 1u; }
// members below id (w = the entry of id's word)
__device__ static inline uint32_t idmap_rank(uint2 w, uint32_t id) {
  return w.y + (uint32_t)__popc(w.x & ((1u << (id & 31u)) - 1u));
}
// test before set (shard.hip, idset_mark_kernel: an atomic on a bit that is already set is the expensive way to find out)
__device__ static inline void idmap_set(uint2 *map, uint32_t id) {
  uint32_t *bits = reinterpret_cast<uint32_t *>(map + (id >> 5));
  const uint32_t m = 1u << (id & 31u);
  if (!(__hip_atomic_load(bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(bits, m);
}

// the bits are set: prefix counts into the entries, the member count to *count_out (may be null)  (remove.hip)
void idmap_finish(const IdMap &m, uint64_t *count_out, hipStream_t st);

// ---- stable compaction of a tile ------------------------------------------------------------------------------------
// element (k, thread) of the tile is its element k * RM_THREADS + thread.  wc: RM_PER * 4 words of LDS.  -> before[k] =
// kept elements of the tile that precede element (k, thread); returns the tile's kept total.  All threads call it.
__device__ static inline uint32_t rm_tile_prefix(const bool (&keep)[RM_PER], uint32_t *wc, uint32_t (&before)[RM_PER]) {
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  uint32_t in_wave[RM_PER];
#pragma unroll
  for (int k = 0; k < RM_PER; ++k) {
    const uint64_t bal = __ballot(keep[k]);
    in_wave[k] = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wc[k * 4 + wave] = (uint32_t)__popcll(bal);
  }
  __syncthreads();
  uint32_t run = 0;
#pragma unroll
  for (int k = 0; k < RM_PER; ++k)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v == wave) before[k] = run + in_wave[k];
      run += wc[k * 4 + v];
    }
  __syncthreads();  // wc may be rewritten by the caller's next tile
  return run;
}
