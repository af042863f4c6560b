// sort.hip -- batched stable LSD radix sort of uint64 keys (+ optional uint32 payload) and qrlsh_owner_bounds.
//
// Replaces the reference's dict-of-lists buckets (lsh.py:9-15, 31-38), its Python set
// de-duplication (lsh.py:41, 53) and its per-query argsort (recommender.py:206) with one
// primitive.  8 bits per pass; per pass: tile histogram -> exclusive scan -> stable scatter.
// Stability inside a tile comes from wavefront ballots: each lane learns which lanes of
// its wave hold the same digit (8 ballots), ranks itself with a popcount below its lane,
// and the wave keeps running per-digit counters in LDS; the four waves of a workgroup are
// then chained by a 256-entry prefix.
//
// With QRLSH_SORT_MIX the digits come from mix64(key) (a bijection), so after 32 bits
// (4 passes instead of 8) equal keys are adjacent up to 32-bit mix collisions, which the
// pair-emission kernel resolves with a full-key compare.
#include "common.h"

constexpr int SORT_IPT = 16;                          // items per thread
constexpr int SORT_TILE = SORT_THREADS * SORT_IPT;    // 4096 keys per workgroup

// digit source: MODE 0 = the key itself, 1 = mix64(key) (grouping sort), 2 = the key with its
// two 32-bit halves packed next to each other, hi << fold | lo (pairs i << 32 | j sort in
// ceil(2*id_bits / 8) passes instead of 2 * ceil(id_bits / 8)).
// 3 = owner: (key >> shift) / aux, one pass that groups words by the rank owning the id field
// (contiguous shards of aux ids each; at most 256 ranks).
// 4 = host: the word is a pair i << 32 | j; digit = the rank that scores it (qr_pair_host: the owner of i
// or of j, chosen by one bit of mix64(pair) so that every rank gets an equal share whatever the data).
// dmask: the digit mask of the pass, RADIX - 1 except in a last pass narrower than 8 bits ((1 << (bit_hi - shift)) - 1):
// the sort orders by bits [bit_lo, bit_hi) and by nothing above them.  Owner and host digits are not masked.
enum { SM_PLAIN = 0, SM_MIX = 1, SM_FOLD = 2, SM_OWNER = 3, SM_HOST = 4 };
template <int MODE> __device__ static inline uint32_t digit_of(uint64_t key, int shift, uint32_t fold, uint32_t dmask) {
  if (MODE == SM_OWNER || MODE == SM_HOST) {
    const uint64_t o = MODE == SM_HOST ? qr_pair_host(key, fold) : (key >> shift) / fold;
    return o < RADIX ? (uint32_t)o : RADIX - 1;
  }
  uint64_t x = key;
  if (MODE == SM_MIX) x = qr_mix64(key);
  if (MODE == SM_FOLD) x = ((key >> 32) << fold) | (key & ((1ull << fold) - 1ull));
  return (uint32_t)(x >> shift) & dmask;
}

// ghist layout: [batch][digit][tile]
template <int MIX>
__global__ __launch_bounds__(SORT_THREADS) void sort_hist_kernel(const uint64_t *__restrict__ keys, int64_t n,
                                                                 int ntiles, int shift,
                                                                 uint32_t *__restrict__ ghist, uint32_t fold,
                                                                 uint32_t dmask) {
  __shared__ uint32_t h[RADIX];
  const int tile = blockIdx.x, batch = blockIdx.y;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t *k = keys + (size_t)batch * n;
  const int64_t base = (int64_t)tile * SORT_TILE;
  // two keys per lane per step (16-byte loads) when the batch base is 16-byte aligned
  const bool wide = ((((uintptr_t)k) & 15) == 0);
#pragma unroll
  for (int i = 0; i < SORT_IPT / 2; ++i) {
    const int64_t idx0 = base + ((int64_t)i * SORT_THREADS + threadIdx.x) * 2;
    uint64_t kk[2] = {0, 0};
    if (wide && idx0 + 1 < n) {
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      const u64x2 t = *reinterpret_cast<const u64x2 *>(k + idx0);
      kk[0] = t.x;
      kk[1] = t.y;
    } else {
      if (idx0 < n) kk[0] = k[idx0];
      if (idx0 + 1 < n) kk[1] = k[idx0 + 1];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int64_t idx = idx0 + e;
      uint32_t dd = 0;
      if (idx < n) {
        const uint32_t d = digit_of<MIX>(kk[e], shift, fold, dmask);
        if (MIX != SM_OWNER && MIX != SM_HOST) atomicAdd(&h[d], 1u);
        dd = d;
      }
      if (MIX == SM_OWNER || MIX == SM_HOST) {
        // a handful of distinct digits (ranks): one LDS atomic per digit per wave, not per key
        const bool valid = idx < n;
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
          const bool one = (dd >> bit) & 1u;
          const uint64_t bal = __ballot(one);
          m &= one ? bal : ~bal;
        }
        const int lane = threadIdx.x & (WAVE - 1);
        if (valid && (m & ((1ull << lane) - 1ull)) == 0) atomicAdd(&h[dd], (uint32_t)__popcll(m));
      }
    }
  }
  __syncthreads();
  ghist[((size_t)batch * RADIX + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// One workgroup per (digit, batch) row of ghist: exclusive scan of the row's ntiles tile
// counts in place, and the row total to rtot[batch][digit].  The scatter kernel turns the
// 256 row totals into digit bases itself, so a pass needs no single-workgroup scan.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void sort_rowscan_kernel(uint32_t *__restrict__ ghist, int ntiles,
                                                               uint32_t *__restrict__ rtot) {
  constexpr int NW = THREADS / WAVE;
  __shared__ uint32_t wsum[NW];
  const int d = blockIdx.x, batch = blockIdx.y;
  uint32_t *row = ghist + ((size_t)batch * RADIX + d) * ntiles;
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  // rows are scanned from registers: 256 threads x 32 for up to 8192 tiles (33 M keys per batch),
  // 1024 threads x 64 for up to 65536 tiles (268 M keys); longer rows take the chunked loop below
  constexpr int ROW_REG = THREADS == 256 ? 32 : 64;
  const int per = (ntiles + THREADS - 1) / THREADS;
  if (per <= ROW_REG) {
    // blocked layout: thread t owns `per` consecutive tiles; every load is issued before the first
    // add, and the whole row needs one workgroup scan instead of one per THREADS tiles
    const int lo = t * per;
    uint32_t held[ROW_REG], s = 0;
#pragma unroll
    for (int k = 0; k < ROW_REG; ++k) held[k] = (k < per && lo + k < ntiles) ? row[lo + k] : 0u;
#pragma unroll
    for (int k = 0; k < ROW_REG; ++k) s += held[k];
    const uint32_t inc = wave_incl_scan(s);
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - s, tot = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const uint32_t x = wsum[k];
      if (k < w) run += x;
      tot += x;
    }
#pragma unroll
    for (int k = 0; k < ROW_REG; ++k)
      if (k < per && lo + k < ntiles) {
        row[lo + k] = run;
        run += held[k];
      }
    if (t == 0) rtot[(size_t)batch * RADIX + d] = tot;
    return;
  }
  uint32_t carry = 0;
  for (int base = 0; base < ntiles; base += THREADS) {
    const int i = base + t;
    const uint32_t v = i < ntiles ? row[i] : 0;
    const uint32_t inc = wave_incl_scan(v);
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const uint32_t x = wsum[k];
      if (k < w) wbase += x;
      tot += x;
    }
    if (i < ntiles) row[i] = carry + wbase + inc - v;
    carry += tot;
    __syncthreads();
  }
  if (t == 0) rtot[(size_t)batch * RADIX + d] = carry;
}

// one row-scan launch: 256-thread workgroups while a row fits their registers, 1024 above
static void launch_rowscan(uint32_t *ghist, int ntiles, uint32_t *rtot, int nbatch, hipStream_t st) {
  if (ntiles <= 256 * 32)
    QR_LAUNCH("sort_rowscan", sort_rowscan_kernel<256>, dim3(RADIX, nbatch), dim3(256), 0, st, ghist, ntiles, rtot);
  else
    QR_LAUNCH("sort_rowscan", sort_rowscan_kernel<1024>, dim3(RADIX, nbatch), dim3(1024), 0, st, ghist, ntiles, rtot);
}

template <int MIX, bool HAS_VAL, bool IOTA>
__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(const uint64_t *__restrict__ keys_in,
                                                                    const uint32_t *__restrict__ vals_in,
                                                                    uint64_t *__restrict__ keys_out,
                                                                    uint32_t *__restrict__ vals_out, int64_t n,
                                                                    int ntiles, int shift,
                                                                    const uint32_t *__restrict__ goff,
                                                                    const uint32_t *__restrict__ rtot,
                                                                    uint32_t fold, uint32_t dmask) {
  __shared__ uint32_t cnt[SORT_THREADS / WAVE][RADIX];
  __shared__ uint32_t dsum[SORT_THREADS / WAVE];
  const int tile = xcd_tile(blockIdx.x, ntiles), batch = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < SORT_THREADS / WAVE; ++i) cnt[i][threadIdx.x] = 0;
  __syncthreads();

  const size_t boff = (size_t)batch * n;
  const int64_t wbase = (int64_t)tile * SORT_TILE + (int64_t)w * (WAVE * SORT_IPT);
  uint64_t key[SORT_IPT];
  uint32_t val[SORT_IPT];
  uint32_t dr[SORT_IPT];  // digit << 16 | rank within this wave's share of the tile
  const uint64_t lt_mask = (1ull << lane) - 1ull;

#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    const bool valid = idx < n;
    key[k] = valid ? keys_in[boff + idx] : 0;
    if (HAS_VAL) val[k] = IOTA ? (uint32_t)idx : (valid ? vals_in[boff + idx] : 0);
  }
#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    const bool valid = idx < n;
    const uint32_t d = digit_of<MIX>(key[k], shift, fold, dmask);
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t bal = __ballot(one);
      m &= one ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(m & lt_mask);
    uint32_t prev = 0;
    if (valid) {
      prev = cnt[w][d];
      if (below == 0) cnt[w][d] = prev + (uint32_t)__popcll(m);
    }
    dr[k] = (d << 16) | (prev + below);
  }
  __syncthreads();
  {
    // chain the waves: cnt[w][d] becomes the global position of wave w's first key with digit d
    const int d = threadIdx.x;
    // digit base = exclusive prefix of the 256 row totals of this batch
    const uint32_t tot = rtot[(size_t)batch * RADIX + d];
    const uint32_t inc = wave_incl_scan(tot);
    if (lane == WAVE - 1) dsum[w] = inc;
    __syncthreads();
    uint32_t dbase = inc - tot;
#pragma unroll
    for (int k = 0; k < SORT_THREADS / WAVE; ++k)
      if (k < w) dbase += dsum[k];
    uint32_t run = dbase + goff[((size_t)batch * RADIX + d) * ntiles + tile];
#pragma unroll
    for (int i = 0; i < SORT_THREADS / WAVE; ++i) {
      const uint32_t c = cnt[i][d];
      cnt[i][d] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    if (idx < n) {
      const uint32_t d = dr[k] >> 16;
      const size_t dst = boff + cnt[w][d] + (dr[k] & 0xFFFFu);
      keys_out[dst] = key[k];
      if (HAS_VAL) vals_out[dst] = val[k];
    }
  }
}

// Keys-only scatter with LDS staging: after ranking, the tile is laid out in LDS in its
// sorted-by-digit order and written out by consecutive lanes, so a store instruction covers a few
// contiguous runs instead of up to 64 unrelated lines.  Same inputs / outputs as
// sort_scatter_kernel<MODE, false, false>; 37 KB of LDS keeps the 4 workgroups per CU that the
// register budget allows anyway.
template <int MODE>
__global__ __launch_bounds__(SORT_THREADS, 4) void sort_scatter_staged_kernel(const uint64_t *__restrict__ keys_in,
                                                                           uint64_t *__restrict__ keys_out, int64_t n,
                                                                           int ntiles, int shift,
                                                                           const uint32_t *__restrict__ goff,
                                                                           const uint32_t *__restrict__ rtot,
                                                                           uint32_t fold, uint32_t dmask) {
  __shared__ uint32_t cnt[SORT_THREADS / WAVE][RADIX];
  __shared__ uint32_t dsum[SORT_THREADS / WAVE];
  __shared__ uint32_t lsum[SORT_THREADS / WAVE];
  __shared__ uint32_t gdelta[RADIX];
  __shared__ uint64_t skey[SORT_TILE];
  const int tile = xcd_tile(blockIdx.x, ntiles), batch = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < SORT_THREADS / WAVE; ++i) cnt[i][threadIdx.x] = 0;
  __syncthreads();
  const size_t boff = (size_t)batch * n;
  const int64_t tbase = (int64_t)tile * SORT_TILE;
  const int64_t wbase = tbase + (int64_t)w * (WAVE * SORT_IPT);
  uint64_t key[SORT_IPT];
  uint32_t dr[SORT_IPT];
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    key[k] = idx < n ? keys_in[boff + idx] : 0;
  }
#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    const bool valid = idx < n;
    const uint32_t d = digit_of<MODE>(key[k], shift, fold, dmask);
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const uint64_t bal = __ballot(one);
      m &= one ? bal : ~bal;
    }
    const uint32_t below = (uint32_t)__popcll(m & lt_mask);
    uint32_t prev = 0;
    if (valid) {
      prev = cnt[w][d];
      if (below == 0) cnt[w][d] = prev + (uint32_t)__popcll(m);
    }
    dr[k] = (d << 16) | (prev + below);
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    // digit base (global) = exclusive prefix of the 256 row totals; tile-local start = exclusive
    // prefix of this tile's 256 digit counts
    const uint32_t tot = rtot[(size_t)batch * RADIX + d];
    uint32_t tc = 0;
#pragma unroll
    for (int i = 0; i < SORT_THREADS / WAVE; ++i) tc += cnt[i][d];
    uint32_t inc = tot, linc = tc;
#pragma unroll
    for (int k = 1; k < WAVE; k <<= 1) {
      const uint32_t o = __shfl_up(inc, k, WAVE), lo = __shfl_up(linc, k, WAVE);
      if (lane >= k) {
        inc += o;
        linc += lo;
      }
    }
    if (lane == WAVE - 1) {
      dsum[w] = inc;
      lsum[w] = linc;
    }
    __syncthreads();
    uint32_t dbase = inc - tot, lstart = linc - tc;
#pragma unroll
    for (int k = 0; k < SORT_THREADS / WAVE; ++k)
      if (k < w) {
        dbase += dsum[k];
        lstart += lsum[k];
      }
    gdelta[d] = dbase + goff[((size_t)batch * RADIX + d) * ntiles + tile] - lstart;
    uint32_t run = lstart;
#pragma unroll
    for (int i = 0; i < SORT_THREADS / WAVE; ++i) {
      const uint32_t c = cnt[i][d];
      cnt[i][d] = run;  // tile-local position of wave i's first key with digit d
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    if (idx < n) skey[cnt[w][dr[k] >> 16] + (dr[k] & 0xFFFFu)] = key[k];
  }
  __syncthreads();
  const int ntile = (int)min((int64_t)SORT_TILE, n - tbase);
#pragma unroll
  for (int k = 0; k < SORT_IPT; ++k) {
    const int p = k * SORT_THREADS + threadIdx.x;
    if (p < ntile) {
      const uint64_t kk = skey[p];
      keys_out[boff + gdelta[digit_of<MODE>(kk, shift, fold, dmask)] + (uint32_t)p] = kk;
    }
  }
}

// workspace: the digit histograms of every (batch, tile), and a row of totals per batch
static uint32_t *sort_layout(QrCarve &c, int64_t n, int32_t nbatch) {
  return c.take<uint32_t>((size_t)nbatch * RADIX * (ceil_div64(n, SORT_TILE) + 1));
}
QRLSH_EXPORT size_t qrlsh_sort_workspace_bytes(int64_t n, int32_t nbatch) {
  if (n <= 0 || nbatch <= 0) return 16;
  return QR_LAYOUT_BYTES(sort_layout, n, nbatch);
}

template <int MIX>
static int sort_passes(uint64_t *ka, uint64_t *kb, uint32_t *va, uint32_t *vb, int64_t n, int nbatch, int bit_lo,
                       int bit_hi, bool iota, uint32_t fold, uint32_t *ghist, hipStream_t st) {
  const int ntiles = (int)ceil_div64(n, SORT_TILE);
  const dim3 grid(ntiles, nbatch), block(SORT_THREADS);
  const bool has_val = va != nullptr;
  uint32_t *rtot = ghist + (size_t)nbatch * RADIX * ntiles;
  int cur = 0;
  for (int shift = bit_lo; shift < bit_hi; shift += 8) {
    uint64_t *kin = cur ? kb : ka, *kout = cur ? ka : kb;
    uint32_t *vin = cur ? vb : va, *vout = cur ? va : vb;
    const uint32_t dmask = (1u << (bit_hi - shift < 8 ? bit_hi - shift : 8)) - 1u;   // the last pass may be narrower
    QR_LAUNCH("sort_hist", (sort_hist_kernel<MIX>), grid, block, 0, st, kin, n, ntiles, shift, ghist, fold, dmask);
    launch_rowscan(ghist, ntiles, rtot, nbatch, st);
    if (!has_val && (MIX == SM_PLAIN || MIX == SM_FOLD))
      QR_LAUNCH("sort_scatter_k", (sort_scatter_staged_kernel<MIX>), grid, block, 0, st, kin, kout, n, ntiles, shift,
                ghist, rtot, fold, dmask);
    else if (!has_val)
      QR_LAUNCH("sort_scatter_k", (sort_scatter_kernel<MIX, false, false>), grid, block, 0, st, kin, vin, kout, vout, n,
                         ntiles, shift, ghist, rtot, fold, dmask);
    else if (iota && shift == bit_lo)
      QR_LAUNCH("sort_scatter_kv", (sort_scatter_kernel<MIX, true, true>), grid, block, 0, st, kin, vin, kout, vout, n,
                         ntiles, shift, ghist, rtot, fold, dmask);
    else
      QR_LAUNCH("sort_scatter_kv", (sort_scatter_kernel<MIX, true, false>), grid, block, 0, st, kin, vin, kout, vout, n,
                         ntiles, shift, ghist, rtot, fold, dmask);
    cur ^= 1;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    qrlsh_set_error("qrlsh_sort_u64: launch failed: %s", hipGetErrorString(e));
    return QRLSH_EHIP;
  }
  return cur;
}

QRLSH_EXPORT int qrlsh_sort_u64(uint64_t *keys_a, uint64_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, int64_t n,
                                int32_t nbatch, int32_t bit_lo, int32_t bit_hi, uint32_t flags, uint64_t aux,
                                void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(n >= 0 && nbatch > 0, "qrlsh_sort_u64: bad sizes n=%lld nbatch=%d", (long long)n, nbatch);
  QR_CHECK_ARG(n < (1ll << 32), "qrlsh_sort_u64: n=%lld per batch exceeds 2^32-1", (long long)n);
  QR_CHECK_ARG(bit_lo >= 0 && bit_hi <= 64 && bit_lo <= bit_hi, "qrlsh_sort_u64: bad bit range [%d,%d)", bit_lo,
               bit_hi);
  QR_CHECK_ARG((vals_a == nullptr) == (vals_b == nullptr), "qrlsh_sort_u64: vals_a/vals_b must both be set or NULL");
  if (n == 0 || bit_lo == bit_hi) return 0;
  QR_CHECK_ARG(keys_a && keys_b && workspace, "qrlsh_sort_u64: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_sort_u64", workspace, workspace_bytes, qrlsh_sort_workspace_bytes(n, nbatch));
  QR_CHECK_ARG(ceil_div64(n, SORT_TILE) <= 2147483647ll && nbatch <= 65535, "qrlsh_sort_u64: grid too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  uint32_t *ghist = sort_layout(c, n, nbatch);
  const bool iota = (flags & QRLSH_SORT_IOTA) != 0;
  if (flags & QRLSH_SORT_MIX)
    return sort_passes<SM_MIX>(keys_a, keys_b, vals_a, vals_b, n, nbatch, bit_lo, bit_hi, iota, 0, ghist, st);
  if (flags & QRLSH_SORT_FOLD) {
    QR_CHECK_ARG(aux >= 1 && aux <= 32, "qrlsh_sort_u64: fold width %llu not in [1,32]", (unsigned long long)aux);
    return sort_passes<SM_FOLD>(keys_a, keys_b, vals_a, vals_b, n, nbatch, bit_lo, bit_hi, iota, (uint32_t)aux, ghist, st);
  }
  if (flags & QRLSH_SORT_OWNER) {
    QR_CHECK_ARG(aux >= 1 && aux < (1ull << 32), "qrlsh_sort_u64: owner shard size %llu not in [1, 2^32)",
                 (unsigned long long)aux);
    // one pass: the digit is the owner rank of the id field that starts at bit_lo
    return sort_passes<SM_OWNER>(keys_a, keys_b, vals_a, vals_b, n, nbatch, bit_lo, bit_lo + 1, iota, (uint32_t)aux, ghist,
                                 st);
  }
  if (flags & QRLSH_SORT_HOST) {
    QR_CHECK_ARG(aux >= 1 && aux < (1ull << 32), "qrlsh_sort_u64: host shard size %llu not in [1, 2^32)",
                 (unsigned long long)aux);
    return sort_passes<SM_HOST>(keys_a, keys_b, vals_a, vals_b, n, nbatch, 0, 1, iota, (uint32_t)aux, ghist, st);
  }
  return sort_passes<SM_PLAIN>(keys_a, keys_b, vals_a, vals_b, n, nbatch, bit_lo, bit_hi, iota, 0, ghist, st);
}

// bounds_out[g] = first position whose owner (word >> lo) / shard is >= g, g = 0 .. world, for
// words already grouped by owner (QRLSH_SORT_OWNER): the split points of the variable all-to-all.
// lo < 0: the words are pairs grouped with QRLSH_SORT_HOST, owner = qr_pair_host
__global__ void owner_bounds_kernel(const uint64_t *__restrict__ w, int64_t n, int lo, uint64_t shard, int world,
                                    int64_t *__restrict__ bounds_out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > world) return;
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    const uint64_t o = lo < 0 ? qr_pair_host(w[mid], (uint32_t)shard) : (w[mid] >> lo) / shard;
    if (o >= (uint64_t)g) b = mid;
    else a = mid + 1;
  }
  bounds_out[g] = a;
}

QRLSH_EXPORT int qrlsh_owner_bounds(const uint64_t *words, int64_t n, int32_t bit_lo, uint64_t shard, int32_t world,
                                    int64_t *bounds_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && bit_lo >= -1 && bit_lo < 64 && shard >= 1 && shard < (1ull << 32) && world >= 1 &&
                   world <= RADIX && bounds_out,
               "qrlsh_owner_bounds: bad arguments");
  QR_CHECK_ARG(n == 0 || words, "qrlsh_owner_bounds: null pointer");
  QR_LAUNCH("owner_bounds", owner_bounds_kernel, dim3((world + 1 + 63) / 64), dim3(64), 0,
            static_cast<hipStream_t>(stream), words, n, bit_lo, shard, world, bounds_out);
  QR_LAUNCH_CHECK("qrlsh_owner_bounds");
  return QRLSH_OK;
}
