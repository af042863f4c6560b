// sort.hip -- batched stable LSD radix sort of uint64 keys (+ optional uint32 payload), qrlsh_owner_bounds, and
// the histogram-free grouping of pair words by region (pair_group_scatter_kernel, qrlsh_pair_regions_*).
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
#include <type_traits>

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

// ---- pair words grouped by REGION without histogram passes (round 4) ------------------------------------------------------
// The region form of the de-duplication (pairs.hip) needs the emitted words grouped by their region id (i >> g, up to 16
// bits) and NOTHING about the order inside a group.  The stable LSD sort pays for an order nobody reads: per 8-bit pass a
// histogram pass over the words, a scan, and the scatter.  Here the words are dealt most-significant digit first the
// way bucket.hip deals its records, words only: every digit owns a fixed region of `cap` words, a tile counts its
// digits in LDS, reserves room with ONE atomic per (tile, digit) and writes its staged words in runs.  Level 1 deals by the
// high digit of the region id into tmp regions, level 2 deals every tmp region by the low digit into the final regions
// (region r at r * cap, counts[r] words).  One read + one write of the words per level -- 2.1 -> 1.4 ms for the 190 M words
// of the 10 M-query workload.  A region that outgrows its cap raises the flag (the caller groups by sorting instead).
#ifndef QR_PG_IPT
// (since the narrow form this constant governs the 8-byte forms and the single level of values only; the figures are round 4's,
// measured when both levels of the flagship's path were 8-byte forms)
#define QR_PG_IPT 32   // 8192-word tiles: runs of 32 - 54 words per (tile, digit); 16: 1.77 ms for the two levels at 10 M, 32: 1.46
#endif
#ifndef QR_PG_IPT_N1
#define QR_PG_IPT_N1 32   // level 1 of the narrow form (6 staged bytes per word, three workgroups per CU): 646 us per launch at 10 M; 40 (two per CU): 689
#endif
#ifndef QR_PG_IPT_N2
#define QR_PG_IPT_N2 40   // level 2 of the narrow form (5 staged bytes per word, 10 240-entry tiles, three per CU): 448 us; 32 (three): 458; 24 (four): 500
#endif
constexpr int PG_IPT = QR_PG_IPT;                 // words per thread of the pair-grouping partition: the 8-byte forms and the one level of values
constexpr int PG_IPT_N1 = QR_PG_IPT_N1, PG_IPT_N2 = QR_PG_IPT_N2;
static_assert(PG_IPT_N2 % 4 == 0, "level 2 of the narrow form reads four entries per load");
static_assert(SORT_THREADS * (PG_IPT > PG_IPT_N1 ? (PG_IPT > PG_IPT_N2 ? PG_IPT : PG_IPT_N2) : (PG_IPT_N1 > PG_IPT_N2 ? PG_IPT_N1 : PG_IPT_N2)) < 0xFFFF,
              "a word's place in its tile is kept in 16 bits");
constexpr int PG_LDS_FIXED = RADIX * 9 + 16;      // cnt, gdelta, gok, lsum
// workgroups per CU that the staged tile allows (160 KB of LDS per CU); at most 4 is asked of the compiler: small tiles
// fit more often, but a bound beyond 4 would only take registers from the kernel
constexpr int pg_wgs(int ipt, int staged_bytes) {
  const int w = 160 * 1024 / (SORT_THREADS * ipt * staged_bytes + PG_LDS_FIXED);
  return w > 4 ? 4 : w < 1 ? 1 : w;
}
// What a level reads -- IN_WORDS: n_in pair words i << 32 | j; IN_TMP_WORDS: the tmp regions of a first level, pair words;
// IN_TMP_NARROW: the tmp regions of a first level in the narrow form (below) -- and what it writes:
//   OUT_WORDS   the pair word as it came (8 bytes; the tile is staged as 8-byte words, the digit is read back from them);
//   OUT_VALUES  (the last level only) the 32-bit value (i & gmask) << jbits | j the region de-duplication reduces every word
//               to as its first step -- the region already says every bit of i above the low g.  Staged as the value and a
//               digit byte beside it: 5 bytes per word;
//   OUT_NARROW  (the first of two levels) that same value into a uint32 array and, at the same index of a byte array, the
//               LOW digit of the region id: the tmp region a word lies in says the high digit, the value the bits of i
//               below the region id and j, so the 5 bytes are all the second level needs (13 + 9 = 22 bytes per word
//               over the two levels instead of 16 + 12).  Staged as the value and (high digit << 8 | low digit): 6 bytes.
// The second level masks the tail with dmask: a tmp region that outgrew its capacity (the flag is up, nothing is usable)
// leaves holes of stale bytes below min(count, cap), and a stale tail must still index inside its batch's cursors.
enum { PG_IN_WORDS = 0, PG_IN_TMP_WORDS = 1, PG_IN_TMP_NARROW = 2 };
enum { PG_OUT_WORDS = 0, PG_OUT_VALUES = 1, PG_OUT_NARROW = 2 };
constexpr int pg_staged_bytes(int out) { return out == PG_OUT_WORDS ? 8 : out == PG_OUT_VALUES ? 5 : 6; }
template <int IN, int OUT, int IPT>
__global__ __launch_bounds__(SORT_THREADS, pg_wgs(IPT, pg_staged_bytes(OUT))) void pair_group_scatter_kernel(
    const void *__restrict__ in_, const uint8_t *__restrict__ in_tails, void *__restrict__ out_, uint8_t *__restrict__ out_tails,
    int64_t n_in, int ntiles, int shift, uint32_t dmask, uint32_t *__restrict__ cursors, uint32_t cap,
    uint32_t *__restrict__ overflow, const uint32_t *__restrict__ in_counts, uint32_t in_cap, int gbits, int jbits, uint32_t bmask) {
  constexpr bool LEVEL2 = IN != PG_IN_WORDS;
  constexpr int TILE = SORT_THREADS * IPT;
  using P = typename std::conditional<OUT == PG_OUT_WORDS, uint64_t, uint32_t>::type;   // what is staged and written
  using D = typename std::conditional<OUT == PG_OUT_NARROW, uint16_t, uint8_t>::type;   // the digit(s) staged beside a value
  static_assert(IN != PG_IN_TMP_NARROW || OUT == PG_OUT_VALUES, "narrow tmp regions hold values");
  static_assert(IN != PG_IN_TMP_WORDS || OUT == PG_OUT_WORDS, "tmp regions of pair words are dealt as pair words");
  __shared__ uint32_t cnt[RADIX];
  __shared__ uint32_t lsum[SORT_THREADS / WAVE];
  __shared__ uint32_t gdelta[RADIX];
  __shared__ uint8_t gok[RADIX];
  __shared__ __attribute__((aligned(16))) unsigned char stage[TILE * pg_staged_bytes(OUT)];
  P *const spay = reinterpret_cast<P *>(stage);
  D *const sdig = reinterpret_cast<D *>(stage + TILE * 4);   // (not used by OUT_WORDS)
  const int tile = LEVEL2 ? (int)blockIdx.x : xcd_tile(blockIdx.x, ntiles), batch = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  const int64_t n = LEVEL2 ? (int64_t)min(in_counts[batch], in_cap) : n_in;
  const int64_t tbase = (int64_t)tile * TILE;
  if (tbase >= n) return;  // LEVEL2: the grid covers a full region, this one holds fewer words (uniform)
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t boff = LEVEL2 ? (size_t)batch * in_cap : 0;
  const uint32_t nd = dmask + 1u;
  // pay[k]: what is staged; dr[k]: the word's place among its tile's words of the same digit in the low 16 bits, above
  // them the digit (OUT_NARROW: high digit << 8 | low digit); all ones: no word
  P pay[IPT];
  uint32_t dr[IPT];
  if constexpr (IN == PG_IN_TMP_NARROW) {
    // four consecutive entries per thread and load (the order inside a tile is free): 16 bytes of values, 4 of tails.
    // The region's last quad is read whole -- regions start and end at multiples of 64 entries -- and the entries at
    // or beyond n are dropped here
    const uint32_t *vals = static_cast<const uint32_t *>(in_) + boff;
    const uint8_t *tails = in_tails + boff;
    uint32_t tl[IPT / 4];
#pragma unroll
    for (int q = 0; q < IPT / 4; ++q) {
      const int64_t idx = tbase + ((int64_t)q * SORT_THREADS + threadIdx.x) * 4;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      tl[q] = 0u;
      if (idx < n) {
        v = *reinterpret_cast<const uint4 *>(vals + idx);
        tl[q] = *reinterpret_cast<const uint32_t *>(tails + idx);
      }
      pay[4 * q] = v.x, pay[4 * q + 1] = v.y, pay[4 * q + 2] = v.z, pay[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int64_t idx = tbase + ((int64_t)(k / 4) * SORT_THREADS + threadIdx.x) * 4 + (k & 3);
      const uint32_t d = (tl[k / 4] >> (8 * (k & 3))) & dmask;
      dr[k] = idx < n ? (d << 16) | atomicAdd(&cnt[d], 1u) : 0xFFFFFFFFu;
    }
  } else {
    const uint64_t *in = static_cast<const uint64_t *>(in_) + boff;
    const int64_t wbase = tbase + (int64_t)w * (WAVE * IPT);
    uint64_t key[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int64_t idx = wbase + (int64_t)k * WAVE + lane;
      key[k] = idx < n ? in[idx] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int64_t idx = wbase + (int64_t)k * WAVE + lane;
      const uint32_t d = (uint32_t)(key[k] >> shift) & dmask;
      uint32_t hi = d << 16;
      if constexpr (OUT == PG_OUT_NARROW) hi = (d << 24) | ((((uint32_t)(key[k] >> 32) >> gbits) & bmask) << 16);
      dr[k] = idx < n ? hi | atomicAdd(&cnt[d], 1u) : 0xFFFFFFFFu;
      if constexpr (OUT == PG_OUT_WORDS)
        pay[k] = key[k];
      else
        pay[k] = (((uint32_t)(key[k] >> 32) & ((1u << gbits) - 1u)) << jbits) | ((uint32_t)key[k] & ((1u << jbits) - 1u));   // jbits <= 31
    }
  }
  __syncthreads();
  const uint32_t tc = cnt[threadIdx.x];
  const uint32_t gb = tc ? atomicAdd(&cursors[(size_t)batch * nd + threadIdx.x], tc) : 0u;
  uint32_t lstart;
  {
    const uint32_t linc = wave_incl_scan(tc);
    if (lane == WAVE - 1) lsum[w] = linc;
    __syncthreads();
    lstart = linc - tc;
#pragma unroll
    for (int k = 0; k < SORT_THREADS / WAVE; ++k)
      if (k < w) lstart += lsum[k];
    cnt[threadIdx.x] = lstart;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < IPT; ++k)
    if (dr[k] != 0xFFFFFFFFu) {
      const uint32_t p = cnt[dr[k] >> (OUT == PG_OUT_NARROW ? 24 : 16)] + (dr[k] & 0xFFFFu);
      spay[p] = pay[k];
      if constexpr (OUT != PG_OUT_WORDS) sdig[p] = (D)(dr[k] >> 16);
    }
  {
    const int d = threadIdx.x;
    const bool ok = (uint64_t)gb + tc <= cap;
    if (!ok) atomicOr(overflow, 1u);
    gok[d] = ok;
    gdelta[d] = (uint32_t)d * cap + gb - lstart;
  }
  __syncthreads();
  uint32_t nstaged = 0;
#pragma unroll
  for (int k = 0; k < SORT_THREADS / WAVE; ++k) nstaged += lsum[k];
  const size_t obase = (size_t)batch * nd * cap;
  P *const out = static_cast<P *>(out_);
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const uint32_t p = k * SORT_THREADS + threadIdx.x;
    if (p < nstaged) {
      const P x = spay[p];
      uint32_t d, t = 0;
      if constexpr (OUT == PG_OUT_WORDS) {
        d = (uint32_t)(x >> shift) & dmask;
      } else {
        t = sdig[p];
        d = OUT == PG_OUT_NARROW ? t >> 8 : t;
      }
      if (gok[d]) {
        const size_t o = obase + (uint32_t)(gdelta[d] + p);
        out[o] = x;
        if constexpr (OUT == PG_OUT_NARROW) out_tails[o] = (uint8_t)t;
      }
    }
  }
}

// split of the region-id bits over the two levels, and the region capacities
struct PairRegions {
  int rbits, ra, rb;      // bits of the region id; high digit (level 1), low digit (level 2); ra == 0: one level
  int64_t nregions;       // region slots = na << rb
  int64_t na;             // level-1 digits that can occur
  uint32_t cap_a, cap_b;  // words per tmp region / per final region
};
static PairRegions pair_regions(int64_t n, int64_t nids, int group_bits, double words_per_query) {
  PairRegions r;
  const int64_t nr = (nids + (1ll << group_bits) - 1) >> group_bits;
  r.rbits = 1;
  while ((1ll << r.rbits) < nr) ++r.rbits;
  r.rb = r.rbits <= 8 ? r.rbits : (r.rbits + 1) / 2;
  r.ra = r.rbits - r.rb;
  r.na = (nr + (1ll << r.rb) - 1) >> r.rb;
  r.nregions = r.na << r.rb;
  // words a region holds on average: n / regions, or -- the words of a shard sit in a slice of the id space --
  // what the caller says a query emits
  double per = (double)n / (double)(nr > 0 ? nr : 1);
  const double hint = words_per_query * (double)(1ll << group_bits);
  if (hint > per) per = hint;
  // i is the SMALLER id of a pair: with partners anywhere in the id space the low ids carry up to twice the mean (the
  // density of the minimum of two ids falls linearly to zero at the top), popular queries come on top of that
  const double cb = 3.0 * per + 4096.0;
  const double ca = r.ra ? 2.5 * per * (double)(1ll << r.rb) + 65536.0 : 0.0;
  r.cap_b = (uint32_t)(cb > 4.0e9 ? 4.0e9 : cb);
  r.cap_b = (r.cap_b + 63u) / 64u * 64u;
  r.cap_a = (uint32_t)(ca > 4.0e9 ? 4.0e9 : ca);
  r.cap_a = (r.cap_a + 63u) / 64u * 64u;
  return r;
}

// pair_group_scatter_kernel places a word at (digit * cap + position) in 32 bits inside one batch: the regions a level
// deals into (na x cap_a at level 1, 2^rb x cap_b per tmp region at level 2) must stay below 2^32 words
static bool pair_regions_fit_u32(const PairRegions &r) {
  return (uint64_t)r.na * r.cap_a < (1ull << 32) && ((uint64_t)r.cap_b << r.rb) < (1ull << 32);
}

// words of the region buffer (and of the tmp buffer of level 1; 0 when one level is enough), the region capacity and count
QRLSH_EXPORT size_t qrlsh_pair_regions_words(int64_t n, int64_t nids, int32_t group_bits, double words_per_query) {
  if (n <= 0 || nids <= 0 || group_bits < 0 || group_bits > 8) return 0;
  const PairRegions r = pair_regions(n, nids, group_bits, words_per_query);
  if (r.rbits > 16) return 0;   // more than 65536 regions: not served (two levels of at most 256 digits)
  if (!pair_regions_fit_u32(r)) return 0;   // a level's regions reach 2^32 words: not served either
  return (size_t)r.nregions * r.cap_b;
}
QRLSH_EXPORT size_t qrlsh_pair_regions_tmp_words(int64_t n, int64_t nids, int32_t group_bits, double words_per_query) {
  if (n <= 0 || nids <= 0 || group_bits < 0 || group_bits > 8) return 0;
  const PairRegions r = pair_regions(n, nids, group_bits, words_per_query);
  return r.ra ? (size_t)r.na * r.cap_a : 0;
}
QRLSH_EXPORT int64_t qrlsh_pair_regions_cap(int64_t n, int64_t nids, int32_t group_bits, double words_per_query) {
  if (n <= 0 || nids <= 0 || group_bits < 0 || group_bits > 8) return 0;
  return (int64_t)pair_regions(n, nids, group_bits, words_per_query).cap_b;
}
QRLSH_EXPORT int64_t qrlsh_pair_regions_count(int64_t n, int64_t nids, int32_t group_bits, double words_per_query) {
  if (n <= 0 || nids <= 0 || group_bits < 0 || group_bits > 8) return 0;
  return pair_regions(n, nids, group_bits, words_per_query).nregions;
}

// words (n pair words i << 32 | j, any order) -> regions[r * cap + k], k < counts[r], r = i >> group_bits; counts:
// uint32 [qrlsh_pair_regions_count + 256] (the tail is level 1's cursors); overflow_out: uint32, != 0 when a region
// outgrew its capacity (nothing usable then).  tmp_regions may be NULL when qrlsh_pair_regions_tmp_words is 0.
template <typename W>
static int pair_regions_scatter_impl(const uint64_t *words, int64_t n, int32_t group_bits, int32_t id_bits, int64_t nids,
                                     double words_per_query, uint64_t *tmp_regions, W *regions, uint32_t *counts,
                                     uint32_t *overflow_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) && nids > 0 && group_bits >= 0 && group_bits <= 8 && counts && overflow_out,
               "qrlsh_pair_regions_scatter: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PairRegions r = pair_regions(n > 0 ? n : 1, nids, group_bits, words_per_query);
  QR_CHECK_ARG(r.rbits <= 16 && r.na <= RADIX, "qrlsh_pair_regions_scatter: %d region bits", r.rbits);
  QR_CHECK_ARG(pair_regions_fit_u32(r),
               "qrlsh_pair_regions_scatter: regions reach 2^32 words (na * cap_a = %llu, 2^rb * cap_b = %llu; need both < 2^32)",
               (unsigned long long)r.na * r.cap_a, (unsigned long long)r.cap_b << r.rb);
  if (hipMemsetAsync(counts, 0, ((size_t)r.nregions + RADIX) * sizeof(uint32_t), st) != hipSuccess ||
      hipMemsetAsync(overflow_out, 0, sizeof(uint32_t), st) != hipSuccess) {
    qrlsh_set_error("qrlsh_pair_regions_scatter: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(words && regions && (r.ra == 0 || tmp_regions), "qrlsh_pair_regions_scatter: null pointer");
  const int sh = 32 + group_bits;
  const uint32_t *none = nullptr;
  constexpr bool VALUES = sizeof(W) == 4;
  constexpr int LAST = VALUES ? PG_OUT_VALUES : PG_OUT_WORDS;
  if (r.ra == 0) {
    const int ntiles = (int)ceil_div64(n, SORT_THREADS * PG_IPT);
    QR_LAUNCH("pair_group", (pair_group_scatter_kernel<PG_IN_WORDS, LAST, PG_IPT>), dim3(ntiles, 1), dim3(SORT_THREADS), 0, st,
              (const void *)words, (const uint8_t *)nullptr, (void *)regions, (uint8_t *)nullptr, n, ntiles, sh,
              (1u << r.rb) - 1u, counts, r.cap_b, overflow_out, none, 0u, (int)group_bits, (int)id_bits, 0u);
  } else if constexpr (VALUES) {
    // the narrow form: tmp holds na * cap_a values, then as many tail bytes (5 of the 8 bytes per entry it was given)
    QR_CHECK_ARG((reinterpret_cast<uintptr_t>(tmp_regions) & 15u) == 0, "qrlsh_pair_regions_scatter32: tmp_regions not 16-byte aligned");
    uint32_t *cur_a = counts + r.nregions;
    uint32_t *tvals = reinterpret_cast<uint32_t *>(tmp_regions);
    uint8_t *ttails = reinterpret_cast<uint8_t *>(tvals + (size_t)r.na * r.cap_a);
    const int ntiles = (int)ceil_div64(n, SORT_THREADS * PG_IPT_N1);
    QR_LAUNCH("pair_group", (pair_group_scatter_kernel<PG_IN_WORDS, PG_OUT_NARROW, PG_IPT_N1>), dim3(ntiles, 1), dim3(SORT_THREADS),
              0, st, (const void *)words, (const uint8_t *)nullptr, (void *)tvals, ttails, n, ntiles, sh + r.rb, (1u << r.ra) - 1u,
              cur_a, r.cap_a, overflow_out, none, 0u, (int)group_bits, (int)id_bits, (1u << r.rb) - 1u);
    QR_LAUNCH("pair_group", (pair_group_scatter_kernel<PG_IN_TMP_NARROW, PG_OUT_VALUES, PG_IPT_N2>),
              dim3((unsigned)ceil_div64(r.cap_a, SORT_THREADS * PG_IPT_N2), (unsigned)r.na), dim3(SORT_THREADS), 0, st,
              (const void *)tvals, (const uint8_t *)ttails, (void *)regions, (uint8_t *)nullptr, (int64_t)0, 0, 0, (1u << r.rb) - 1u,
              counts, r.cap_b, overflow_out, (const uint32_t *)cur_a, r.cap_a, 0, 0, 0u);
  } else {
    uint32_t *cur_a = counts + r.nregions;
    const int ntiles = (int)ceil_div64(n, SORT_THREADS * PG_IPT);
    QR_LAUNCH("pair_group", (pair_group_scatter_kernel<PG_IN_WORDS, PG_OUT_WORDS, PG_IPT>), dim3(ntiles, 1), dim3(SORT_THREADS), 0, st,
              (const void *)words, (const uint8_t *)nullptr, (void *)tmp_regions, (uint8_t *)nullptr, n, ntiles, sh + r.rb,
              (1u << r.ra) - 1u, cur_a, r.cap_a, overflow_out, none, 0u, 0, 0, 0u);
    QR_LAUNCH("pair_group", (pair_group_scatter_kernel<PG_IN_TMP_WORDS, PG_OUT_WORDS, PG_IPT>),
              dim3((unsigned)ceil_div64(r.cap_a, SORT_THREADS * PG_IPT), (unsigned)r.na), dim3(SORT_THREADS), 0, st,
              (const void *)tmp_regions, (const uint8_t *)nullptr, (void *)regions, (uint8_t *)nullptr, (int64_t)0, 0, sh,
              (1u << r.rb) - 1u, counts, r.cap_b, overflow_out, (const uint32_t *)cur_a, r.cap_a, 0, 0, 0u);
  }
  QR_LAUNCH_CHECK("qrlsh_pair_regions_scatter");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_pair_regions_scatter(const uint64_t *words, int64_t n, int32_t group_bits, int64_t nids,
                                            double words_per_query, uint64_t *tmp_regions, uint64_t *regions,
                                            uint32_t *counts, uint32_t *overflow_out, void *stream) {
  return pair_regions_scatter_impl<uint64_t>(words, n, group_bits, 0, nids, words_per_query, tmp_regions, regions, counts,
                                             overflow_out, stream);
}

// The same into regions of 32-bit values (i & (2^group_bits - 1)) << id_bits | j: capacities and counts are those of the
// 8-byte form, in entries; only the bytes per entry of `regions` differ.  Needs group_bits + id_bits <= 32 and a value
// that is never 0xFFFFFFFF (qrlsh_region_unique_count_regions32, the only reader, marks empty slots with it).
QRLSH_EXPORT int qrlsh_pair_regions_scatter32(const uint64_t *words, int64_t n, int32_t group_bits, int32_t id_bits,
                                              int64_t nids, double words_per_query, uint64_t *tmp_regions, uint32_t *regions,
                                              uint32_t *counts, uint32_t *overflow_out, void *stream) {
  QR_CHECK_ARG(group_bits >= 0 && group_bits <= 8 && id_bits >= 1 && id_bits <= 31 && nids > 0 && nids <= (1ll << id_bits) &&
                   (group_bits + id_bits < 32 || (group_bits + id_bits == 32 && nids < (1ll << id_bits))),
               "qrlsh_pair_regions_scatter32: group_bits=%d / id_bits=%d / nids=%lld do not fit a 32-bit value", group_bits,
               id_bits, (long long)nids);
  return pair_regions_scatter_impl<uint32_t>(words, n, group_bits, id_bits, nids, words_per_query, tmp_regions, regions,
                                             counts, overflow_out, stream);
}

QRLSH_EXPORT size_t qrlsh_sort_workspace_bytes(int64_t n, int32_t nbatch) {
  if (n <= 0 || nbatch <= 0) return 16;
  const int64_t ntiles = ceil_div64(n, SORT_TILE);
  return (size_t)nbatch * RADIX * (ntiles + 1) * sizeof(uint32_t);
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
  if (workspace_bytes < qrlsh_sort_workspace_bytes(n, nbatch)) {
    qrlsh_set_error("qrlsh_sort_u64: workspace %zu < %zu bytes", workspace_bytes,
                    qrlsh_sort_workspace_bytes(n, nbatch));
    return QRLSH_EWORKSPACE;
  }
  QR_CHECK_ARG(ceil_div64(n, SORT_TILE) <= 2147483647ll && nbatch <= 65535, "qrlsh_sort_u64: grid too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t *ghist = static_cast<uint32_t *>(workspace);
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
