// dedup.hip -- a3 tail: the emitted pair words -> sorted unique pairs, in LDS.
//
// Reference: the Python set that removes cross-band duplicates, lsh.py:41, 53.
//
// Three parts, each with its entry points:
//   row form      (qrlsh_row_unique_*)      words sorted by i (or by a few i): rows found inside fixed chunks of the input;
//   region form   (qrlsh_region_unique_*)   one workgroup per region of 2^g consecutive i, from words sorted by region
//                                           or from the fixed regions of 32-bit values the grouping below fills;
//   pair grouping (qrlsh_pair_regions_*)    the emitted words dealt into those fixed regions without histogram passes.
// qrlsh_pair_regions_scatter32 and qrlsh_region_unique_count_regions32 are ONE step: same group_bits / id_bits / nids,
// same counts array, and the scatter's flag word is read by the finish on the same stream.
// The general path (full sort + qrlsh_unique_*) is in sort.hip / pairs.hip.
#include "common.h"
#include <type_traits>

// ---- a3 tail, fast form: sorted unique pairs from pairs GROUPED BY i ---------------------------
// The emitted pairs carry every candidate once per band it collides in (5.5x on the config-2
// workload), and a full (i, j) radix sort of all of them only to drop the repeats is the
// largest block of sort passes in the pipeline.  Here the pairs are sorted on i's bits only
// (ceil(id_bits / 8) passes instead of ceil(2 id_bits / 8)); a row (all pairs of one i) is then
// a short run -- tens of words -- that is de-duplicated and ordered by j inside LDS:
//   1. the row's own span of an LDS array serves as an open-addressing hash set of its j values
//      (as many slots as the row has words; ds_cmpst claims a slot or finds the value present);
//   2. a workgroup prefix sum over the occupied slots packs the distinct values, row by row;
//   3. the place of a distinct value is the number of smaller ones in its (now short) packed row.
//
// A workgroup owns the rows whose first word lies in its RD_C-word chunk; it loads RD_CAP words
// beyond the chunk so that the last owned row is complete (a longer overhang sets the overflow
// flag: the caller then uses the general sort + qrlsh_unique path).  The kept words of a
// workgroup are written, in order, into `tmp` starting at its first owned word (owned ranges
// tile the input, so these never overlap); per-workgroup counts are scanned and a second small
// kernel closes the gaps.
// A "row" may also be a GROUP of 2^gbits consecutive i (the words are then ordered by i >> gbits only,
// which can save the grouping sort its last pass): the value that is de-duplicated and ordered inside
// a row is then (i's low gbits, j) packed into 32 bits, j < 2^jbits.
struct RowSplit {
  int gbits, jbits;
  __device__ uint32_t row(uint64_t x) const { return (uint32_t)(x >> (32 + gbits)); }
  __device__ uint32_t val(uint64_t x) const {
    const uint32_t j = (uint32_t)x;
    return gbits ? ((uint32_t)(x >> 32) & ((1u << gbits) - 1u)) << jbits | j : j;
  }
  // the word of value v in the row that word x0 belongs to
  __device__ uint64_t word(uint64_t x0, uint32_t v) const {
    if (!gbits) return (x0 & 0xFFFFFFFF00000000ull) | v;
    const uint64_t i = ((x0 >> 32) & ~(uint64_t)((1u << gbits) - 1u)) | (v >> jbits);
    return i << 32 | (v & ((1u << jbits) - 1u));
  }
};

constexpr int RD_THREADS = 512;
constexpr int RD_C = 2048;
constexpr int RD_CAP = 1024;
constexpr int RD_IMG = RD_C + RD_CAP;
constexpr int RD_PER = RD_IMG / RD_THREADS;
constexpr uint32_t RD_EMPTY = 0xFFFFFFFFu;  // never a j (ids are non-negative int32)

__global__ __launch_bounds__(RD_THREADS) void row_unique_kernel(const uint64_t *__restrict__ in, int64_t n,
                                                                uint64_t *__restrict__ tmp,
                                                                uint64_t *__restrict__ counts,
                                                                uint64_t *__restrict__ starts,
                                                                uint64_t *__restrict__ longlist,
                                                                unsigned long long *__restrict__ nlong, int gbits,
                                                                int jbits) {
  __shared__ uint32_t lo[RD_IMG];    // j of every word; later: the packed distinct values
  __shared__ uint32_t tab[RD_IMG];   // hash sets, one per owned row, over the row's own span
  __shared__ uint16_t rs[RD_IMG];    // row start + 1 of the row a word belongs to, 0 = row began before the image
  __shared__ uint16_t re[RD_IMG];    // at a row's start: one past its last word
  __shared__ uint16_t pre[RD_IMG + 1];  // occupied slots before position p
  __shared__ uint16_t crow[RD_IMG];  // row start of every packed value
  __shared__ uint32_t wsum[RD_THREADS / WAVE];
  __shared__ uint32_t h0s, tail_open, long_s;
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const RowSplit rsp{gbits, jbits};
  const int64_t c0 = (int64_t)blockIdx.x * RD_C;
  const int m = (int)min((int64_t)RD_IMG, n - c0);
  const int mc = min(RD_C, m);
  if (t == 0) {
    h0s = 0xFFFFFFFFu;
    tail_open = 0;
    long_s = 0xFFFFFFFFu;
  }
  __syncthreads();
  // load; a word whose i differs from its predecessor's starts a row (i itself is not kept in LDS:
  // the output step re-reads it, the lines are still in L2)
  {
    uint64_t x[RD_PER], xp[RD_PER];  // all global loads of the workgroup are issued before the first use
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = k * RD_THREADS + t;
      x[k] = p < m ? in[c0 + p] : 0;
    }
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = k * RD_THREADS + t;
      xp[k] = (lane == 0 && p < m && c0 + p > 0) ? in[c0 + p - 1] : 0;
    }
    const bool more = t == 0 && c0 + m < n;   // does the last word's row go on past the image?
    const uint64_t xlast = more ? in[c0 + m - 1] : 0, xnext = more ? in[c0 + m] : 1ull << 32;
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = k * RD_THREADS + t;
      const uint32_t h = rsp.row(x[k]);
      const uint32_t ph = __shfl_up(h, 1, WAVE);
      if (p < m) {
        lo[p] = rsp.val(x[k]);
        tab[p] = RD_EMPTY;
        const bool head = lane == 0 ? (c0 + p == 0 || rsp.row(xp[k]) != h) : ph != h;
        rs[p] = head ? (uint16_t)(p + 1) : (uint16_t)0;
      }
    }
    if (more && rsp.row(xlast) == rsp.row(xnext)) tail_open = 1;
  }
  __syncthreads();

  // row starts: running maximum of (head position + 1), blocked layout (RD_PER consecutive words per thread)
  const int b0 = t * RD_PER;
  {
    uint32_t run = 0;
    uint16_t loc[RD_PER];
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = b0 + k;
      if (p < m) run = max(run, (uint32_t)rs[p]);
      loc[k] = (uint16_t)run;
    }
    uint32_t inc = run;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d, WAVE);
      if (lane >= d) inc = max(inc, o);
    }
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t excl = __shfl_up(inc, 1, WAVE);
    if (lane == 0) excl = 0;
    for (int k = 0; k < w; ++k) excl = max(excl, wsum[k]);
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = b0 + k;
      if (p < m) rs[p] = (uint16_t)max((uint32_t)loc[k], excl);
    }
  }
  __syncthreads();
  for (int p = t; p < m; p += RD_THREADS) {
    const uint32_t s1 = rs[p];
    if (!s1) continue;
    if (s1 == (uint32_t)p + 1u && p < mc) atomicMin(&h0s, (uint32_t)p);
    const bool last = p + 1 == m;
    if (last || rs[p + 1] == (uint16_t)(p + 2)) re[s1 - 1] = (uint16_t)(p + 1);
    // the last owned row runs past the image: it is left to row_unique_long_kernel (it is
    // necessarily the LAST row that starts in this chunk, so its output follows this workgroup's)
    if (last && (int)s1 - 1 < mc && tail_open) long_s = s1 - 1;
  }
  __syncthreads();
  const int own_end = (int)min((uint32_t)mc, long_s);  // rows starting before this position are finished here

  // 1. hash-set insert of every owned word into its row's span of tab
  for (int p = t; p < m; p += RD_THREADS) {
    const uint32_t s1 = rs[p];
    if (!s1 || (int)s1 - 1 >= own_end) continue;
    const uint32_t s = s1 - 1, e = re[s], len = e - s, v = lo[p];
    uint32_t slot = s + __umulhi(v * 0x9E3779B1u, len);
    for (;;) {  // at most len probes: the row has len slots and at most len distinct values
      const uint32_t old = atomicCAS(&tab[slot], RD_EMPTY, v);
      if (old == RD_EMPTY || old == v) break;
      slot = slot + 1 == e ? s : slot + 1;
    }
  }
  __syncthreads();
  // 2. exclusive prefix sum over the occupied slots; pack the distinct values (lo is free now)
  uint32_t total;
  {
    uint32_t sum = 0, val[RD_PER];
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = b0 + k;
      val[k] = p < m ? tab[p] : RD_EMPTY;
      sum += val[k] != RD_EMPTY;
    }
    // (the scan's first barrier: every wave is done with wsum (row starts) and with lo)
    uint32_t run = block_excl_scan<RD_THREADS>(sum, wsum, total);
#pragma unroll
    for (int k = 0; k < RD_PER; ++k) {
      const int p = b0 + k;
      if (p <= m) pre[p] = (uint16_t)run;   // p == m: the grand total (one thread reaches it)
      if (val[k] != RD_EMPTY) {
        lo[run] = val[k];
        crow[run] = (uint16_t)(rs[p] - 1);
        ++run;
      }
    }
    if (t == RD_THREADS - 1) pre[m] = (uint16_t)total;
  }
  __syncthreads();
  // 3. place of every distinct value inside its packed row; write out
  const uint32_t h0 = h0s == 0xFFFFFFFFu ? 0u : h0s;
  uint64_t *dst = tmp + c0 + h0;
  for (uint32_t k = t; k < total; k += RD_THREADS) {
    const uint32_t s = crow[k], cs = pre[s], ce = pre[re[s]], v = lo[k];
    uint32_t r = 0;
    for (uint32_t q = cs; q < ce; ++q) r += lo[q] < v;
    dst[cs + r] = rsp.word(in[c0 + s], v);
  }
  if (t == 0) {
    // two output segments per workgroup: its finished rows, then its long row (filled in later)
    counts[2 * (size_t)blockIdx.x] = total;
    starts[2 * (size_t)blockIdx.x] = (uint64_t)(c0 + h0);
    counts[2 * (size_t)blockIdx.x + 1] = 0;
    starts[2 * (size_t)blockIdx.x + 1] = (uint64_t)(c0 + (long_s == 0xFFFFFFFFu ? 0u : long_s));
    if (long_s != 0xFFFFFFFFu)
      longlist[__hip_atomic_fetch_add(nlong, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = blockIdx.x;
  }
}

// Rows too long for the chunk image (an i with thousands of emitted pairs; rare): one 1024-thread
// workgroup per row, same three steps with a table of RL_CAP slots.  The grid is fixed and walks the
// list the main kernel left, so nothing is read back to size the launch.  A row above RL_CAP words
// raises the overflow word (general path).
constexpr int RL_THREADS = 1024;
constexpr int RL_CAP = 12288;
constexpr int RL_PER = RL_CAP / RL_THREADS;
constexpr int RL_GRID = 512;

__global__ __launch_bounds__(RL_THREADS) void row_unique_long_kernel(const uint64_t *__restrict__ in, int64_t n,
                                                                     uint64_t *__restrict__ tmp,
                                                                     uint64_t *__restrict__ counts,
                                                                     const uint64_t *__restrict__ starts,
                                                                     const uint64_t *__restrict__ longlist,
                                                                     const unsigned long long *__restrict__ nlong,
                                                                     uint64_t *__restrict__ overflow, int gbits,
                                                                     int jbits) {
  __shared__ uint32_t tab[RL_CAP];
  __shared__ uint32_t pk[RL_CAP];
  __shared__ uint32_t wsum[RL_THREADS / WAVE];
  __shared__ long long s_end;
  const int t = threadIdx.x, lane = t & (WAVE - 1), w = t >> 6;
  const unsigned long long nl = *nlong;
  const RowSplit rsp{gbits, jbits};
  for (unsigned long long e = blockIdx.x; e < nl; e += gridDim.x) {
    const uint64_t b = longlist[e];
    const int64_t s0 = (int64_t)starts[2 * b + 1];
    const uint64_t x0 = in[s0];
    if (t == 0) {  // end of the row: first position whose row id is larger (the words are ordered by it)
      const uint32_t r0 = rsp.row(x0);
      int64_t a = s0 + 1, z = n;
      while (a < z) {
        const int64_t mid = (a + z) >> 1;
        if (rsp.row(in[mid]) > r0) z = mid;
        else a = mid + 1;
      }
      s_end = a;
    }
#pragma unroll
    for (int k = 0; k < RL_PER; ++k) tab[t + k * RL_THREADS] = RD_EMPTY;
    __syncthreads();
    const int64_t len = s_end - s0;
    if (len > RL_CAP) {  // uniform
      if (t == 0) atomicOr((unsigned long long *)overflow, 1ull);
      __syncthreads();
      continue;
    }
    for (int64_t p = t; p < len; p += RL_THREADS) {
      const uint32_t v = rsp.val(in[s0 + p]);
      uint32_t slot = __umulhi(v * 0x9E3779B1u, (uint32_t)RL_CAP);
      for (;;) {
        const uint32_t old = atomicCAS(&tab[slot], RD_EMPTY, v);
        if (old == RD_EMPTY || old == v) break;
        slot = slot + 1 == (uint32_t)RL_CAP ? 0u : slot + 1;
      }
    }
    __syncthreads();
    // pack the distinct values
    const int b0 = t * RL_PER;
    uint32_t val[RL_PER], sum = 0;
#pragma unroll
    for (int k = 0; k < RL_PER; ++k) {
      val[k] = tab[b0 + k];
      sum += val[k] != RD_EMPTY;
    }
    const uint32_t inc = wave_incl_scan(sum);
    if (lane == WAVE - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t run = inc - sum, u = 0;
    for (int k = 0; k < RL_THREADS / WAVE; ++k) {
      if (k < w) run += wsum[k];
      u += wsum[k];
    }
#pragma unroll
    for (int k = 0; k < RL_PER; ++k)
      if (val[k] != RD_EMPTY) pk[run++] = val[k];
    __syncthreads();
    for (uint32_t k = t; k < u; k += RL_THREADS) {
      const uint32_t v = pk[k];
      uint32_t r = 0;
#pragma unroll 8
      for (uint32_t q = 0; q < u; ++q) r += pk[q] < v;
      tmp[s0 + r] = rsp.word(x0, v);
    }
    if (t == 0) counts[2 * b + 1] = u;
    __syncthreads();  // tab / pk / wsum / s_end are reused by the next row
  }
}

// close the gaps: workgroup g copies its counts[g] kept words from tmp[starts[g]..] to out[offs[g]..]
__global__ __launch_bounds__(RD_THREADS) void row_unique_gather_kernel(const uint64_t *__restrict__ tmp,
                                                                       const uint64_t *__restrict__ offs,
                                                                       const uint64_t *__restrict__ starts,
                                                                       uint64_t *__restrict__ out) {
#pragma unroll
  for (int seg = 0; seg < 2; ++seg) {  // the workgroup's finished rows, then its long row (usually empty)
    const size_t g = 2 * (size_t)blockIdx.x + seg;
    const uint64_t o0 = offs[g], cnt = offs[g + 1] - o0;
    const uint64_t *src = tmp + starts[g];
    for (uint32_t k = threadIdx.x; k < cnt; k += RD_THREADS) out[o0 + k] = src[k];
  }
}

// workspace: counts[2 nblk + 1] | starts[2 nblk] | longlist[nblk] | nlong | chunk totals of the scan
struct RowUniqueWs {
  int64_t nblk;
  uint64_t *counts, *starts, *longlist, *nlong, *sums;
};
static RowUniqueWs row_unique_layout(QrCarve &c, int64_t n) {
  RowUniqueWs w;
  w.nblk = n > 0 ? ceil_div64(n, RD_C) : 0;
  w.counts = c.take<uint64_t>((size_t)(2 * w.nblk + 1), 8);
  w.starts = c.take<uint64_t>((size_t)(2 * w.nblk), 8);
  w.longlist = c.take<uint64_t>((size_t)w.nblk, 8);
  w.nlong = c.take<uint64_t>(1, 8);
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(2 * w.nblk + 1, SCANL_CHUNK) + 1), 8);
  return w;
}
QRLSH_EXPORT size_t qrlsh_row_unique_workspace_bytes(int64_t n) {
  return QR_LAYOUT_BYTES(row_unique_layout, n);
}

QRLSH_EXPORT int qrlsh_row_unique_count(const uint64_t *grouped, int64_t n, int32_t group_bits, int32_t id_bits,
                                        uint64_t *tmp, void *workspace, size_t workspace_bytes,
                                        uint64_t *total_overflow_out, void *stream) {
  QR_CHECK_ARG(n >= 0 && total_overflow_out, "qrlsh_row_unique_count: bad arguments");
  QR_CHECK_ARG(group_bits >= 0 && group_bits <= 8 && id_bits >= 1 && id_bits <= 32 &&
                   (group_bits == 0 || group_bits + id_bits <= 32),
               "qrlsh_row_unique_count: group_bits=%d / id_bits=%d (need group_bits + id_bits <= 32)", group_bits,
               id_bits);
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET("qrlsh_row_unique_count", total_overflow_out, 0, 2 * sizeof(uint64_t), st);
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(grouped && tmp && workspace, "qrlsh_row_unique_count: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_row_unique_count", workspace, workspace_bytes, qrlsh_row_unique_workspace_bytes(n));
  QrCarve c(workspace);
  const RowUniqueWs w = row_unique_layout(c, n);
  const int64_t nblk = w.nblk;
  uint64_t *counts = w.counts, *starts = w.starts, *longlist = w.longlist, *nlong = w.nlong;
  QR_MEMSET("qrlsh_row_unique_count", counts + 2 * nblk, 0, sizeof(uint64_t), st);
  QR_MEMSET("qrlsh_row_unique_count", nlong, 0, sizeof(uint64_t), st);
  QR_LAUNCH("row_unique", row_unique_kernel, dim3((unsigned)nblk), dim3(RD_THREADS), 0, st, grouped, n, tmp, counts,
            starts, longlist, reinterpret_cast<unsigned long long *>(nlong), group_bits, id_bits);
  QR_LAUNCH("row_unique_long", row_unique_long_kernel, dim3((unsigned)(nblk < RL_GRID ? nblk : RL_GRID)),
            dim3(RL_THREADS), 0, st, grouped, n, tmp, counts, (const uint64_t *)starts, (const uint64_t *)longlist,
            (const unsigned long long *)nlong, total_overflow_out + 1, group_bits, id_bits);
  qr_scan_u64(counts, 2 * nblk + 1, total_overflow_out, w.sums, st);
  QR_LAUNCH_CHECK("qrlsh_row_unique_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_row_unique_fill(const uint64_t *tmp, int64_t n, const void *workspace, uint64_t *out,
                                       void *stream) {
  QR_CHECK_ARG(n >= 0, "qrlsh_row_unique_fill: bad n");
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(tmp && workspace && out, "qrlsh_row_unique_fill: null pointer");
  QrCarve c(workspace);
  const RowUniqueWs w = row_unique_layout(c, n);
  const uint64_t *offs = w.counts, *starts = w.starts;   // (the counts, scanned)
  QR_LAUNCH("row_unique_gather", row_unique_gather_kernel, dim3((unsigned)w.nblk), dim3(RD_THREADS), 0,
            static_cast<hipStream_t>(stream), tmp, offs, starts, out);
  QR_LAUNCH_CHECK("qrlsh_row_unique_fill");
  return QRLSH_OK;
}

// ---- a3 tail, region form: sorted unique pairs from pairs grouped by i >> g, g up to 8 ---------------
// row_unique above finishes rows that a workgroup discovers inside a fixed chunk of the input; its cost is the
// bookkeeping of that discovery (row starts / ends / overhang, per-position arrays) and, at 2^24 ids, the three
// grouping passes that make single-i rows.  Here a REGION is the set of words whose i share their bits above
// g (2^g consecutive queries, a few thousand words): the grouping sort orders the words by i >> g only -- at
// 2^24 ids and g = 8 that is TWO radix passes -- and one workgroup finishes one region:
//   1. the words are streamed from global memory (never staged) into an open-addressing hash set in LDS keyed
//      by the 32-bit value (i's low g bits, j); a first insertion also counts the value for its i (256 counters);
//   2. the counters are scanned -> where each i's distinct values start in the output;
//   3. the occupied slots are dealt to their i's segment, then every value finds its place by counting the
//      smaller ones of its own i (a handful).
// Only the number of DISTINCT pairs of a region is bounded by LDS, not its word count, so an i with thousands
// of repeated emissions is no special case: about 5 K per region in the main kernel (two workgroups per CU),
// about 11 K in the big-image kernel that takes over the few regions beyond that; a region beyond THAT raises
// the overflow word and the caller takes the general path.  Region boundaries come from a binary search per region (the words are
// ordered by region), outputs are packed by the same count -> scan -> gather as above.
constexpr int RG_THREADS = 1024;
constexpr int RG_SEG = 6144;     // distinct pairs a region may hold
constexpr int RG_ROWS = 256;     // 2^g <= 256
constexpr int RG_LONGROW = 192;  // a query with more distinct neighbours than this is ranked through sub-buckets

__global__ __launch_bounds__(256) void region_bounds_kernel(const uint64_t *__restrict__ w, int64_t n, int shift,
                                                            int64_t nregions, uint64_t *__restrict__ starts) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f > nregions) return;
  int64_t a = 0, b = n;  // first position whose region is >= f
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if ((int64_t)(w[mid] >> shift) >= f) b = mid;
    else a = mid + 1;
  }
  starts[f] = (uint64_t)a;
}

// One region, finished by the calling workgroup (RG_THREADS threads).  TAB_LOG2 / SEG size the hash set and the
// segment array.  Returns false (uniform) when the region holds more than SEG distinct pairs.
// W = the word of `in`: the pair word, or the 32-bit value itself (regions of qrlsh_pair_regions_scatter32).
template <int TAB_LOG2, int SEG, typename W>
__device__ static inline bool region_finish(const W *__restrict__ in, int64_t s0, int64_t s1, int64_t region,
                                            uint64_t *__restrict__ tmp, uint64_t *__restrict__ counts, int gbits,
                                            int jbits) {
  constexpr int TAB = 1 << TAB_LOG2;
  __shared__ uint32_t tab[TAB];
  __shared__ uint32_t seg[SEG];
  __shared__ uint32_t rowcnt[RG_ROWS], rowstart[RG_ROWS + 1], rowfill[RG_ROWS];
  __shared__ uint32_t sub[RG_ROWS], substart[RG_ROWS + 1], subfill[RG_ROWS];
  __shared__ uint64_t longmask[RG_ROWS / WAVE];
  __shared__ uint32_t wsum[RG_ROWS / WAVE];
  __shared__ uint32_t full, ndist;
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
#pragma unroll
  for (int k = 0; k < TAB / RG_THREADS; ++k) tab[t + k * RG_THREADS] = RD_EMPTY;
  if (t < RG_ROWS) {
    rowcnt[t] = 0;
    rowfill[t] = 0;
  }
  if (t == 0) {
    full = 0;
    ndist = 0;
  }
  __syncthreads();
  const uint32_t gmask = (1u << gbits) - 1u, jmask = (1u << jbits) - 1u;  // jbits <= 31 (qrlsh_region_unique_count refuses 32)
  // 1. stream the words into the hash set, four independent loads in flight per thread
  for (int64_t p0 = s0 + t; p0 < s1; p0 += 4 * RG_THREADS) {
    W x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t p = p0 + (int64_t)k * RG_THREADS;
      x[k] = p < s1 ? in[p] : (W)~(W)0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (p0 + (int64_t)k * RG_THREADS >= s1) continue;
      uint32_t row, v;
      if constexpr (sizeof(W) == 4) {
        v = x[k];
        row = v >> jbits;
      } else {
        row = (uint32_t)(x[k] >> 32) & gmask;
        v = row << jbits | ((uint32_t)x[k] & jmask);
      }
      // Not a value of this region: a slot of a fixed region that was never written.  After a capacity overflow of
      // qrlsh_pair_regions_scatter32 the tiles that did not fit skip their runs, and what the buffer held before is read
      // here before the host sees the flag.  A row beyond 2^gbits would index past rowcnt / rowstart and send the
      // placement below to an arbitrary address; the empty marker would be counted without taking a slot.
      if (row > gmask || v == RD_EMPTY) continue;
      uint32_t slot = (v * 0x9E3779B1u) >> (32 - TAB_LOG2);
      // the set never takes more than SEG values (SEG < TAB: a free slot always turns up); once it would, the
      // region is given up and the remaining words are skipped
      while (!*(volatile uint32_t *)&full) {
        const uint32_t old = atomicCAS(&tab[slot], RD_EMPTY, v);
        if (old == RD_EMPTY) {
          atomicAdd(&rowcnt[row], 1u);
          if (atomicAdd(&ndist, 1u) >= (uint32_t)SEG - RG_THREADS) full = 1;  // (up to RG_THREADS inserts are in flight)
          break;
        }
        if (old == v) break;
        slot = (slot + 1) & (TAB - 1);
      }
    }
    if (*(volatile uint32_t *)&full) break;
  }
  __syncthreads();
  // 2. where each i's distinct values start: exclusive scan of the 256 counters
  uint32_t c = 0, inc = 0;
  if (t < RG_ROWS) {
    c = rowcnt[t];
    inc = wave_incl_scan(c);
    if (lane == WAVE - 1) wsum[wv] = inc;
  }
  __syncthreads();
  if (t < RG_ROWS) {
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < RG_ROWS / WAVE; ++k)
      if (k < wv) base += wsum[k];
    rowstart[t] = base + inc - c;
    if (t == RG_ROWS - 1) rowstart[RG_ROWS] = base + inc;
    const uint64_t lm = __ballot(c > (uint32_t)RG_LONGROW);  // which of this wave's 64 rows are popular queries
    if (lane == 0) longmask[wv] = lm;
  }
  __syncthreads();
  const uint32_t u = rowstart[RG_ROWS];
  const bool fits = !full;   // full: SEG - RG_THREADS distinct values were reached (u <= SEG either way)
  __syncthreads();  // every thread has read `full` / `u` before the arrays are touched again (or re-initialised)
  if (!fits) return false;
  // 3. deal the occupied slots to their i's segment ...
#pragma unroll
  for (int k = 0; k < TAB / RG_THREADS; ++k) {
    const uint32_t v = tab[t + k * RG_THREADS];
    if (v != RD_EMPTY) {
      const uint32_t row = v >> jbits;
      seg[rowstart[row] + atomicAdd(&rowfill[row], 1u)] = v;
    }
  }
  __syncthreads();
  // ... and place every value by the number of smaller ones of its own i
  const uint64_t ihigh = (uint64_t)region << gbits;
  uint64_t *dst = tmp + s0;
  for (uint32_t k = t; k < u; k += RG_THREADS) {
    const uint32_t v = seg[k], row = v >> jbits;
    const uint32_t rs = rowstart[row], re = rowstart[row + 1];
    if (re - rs > (uint32_t)RG_LONGROW) continue;  // a popular query: below
    uint32_t r = 0;
    for (uint32_t q = rs; q < re; ++q) r += seg[q] < v;
    dst[rs + r] = (ihigh | row) << 32 | (v & jmask);
  }
  // A popular query (hundreds to thousands of distinct neighbours) would cost its square that way.  Its values
  // are first dealt into 256 sub-buckets by the top bits of j (the same count -> scan -> deal as above, into the
  // hash table's space, which is dead by now) and then ranked inside their sub-bucket.
  const int sh = jbits > 8 ? jbits - 8 : 0;
  uint32_t *seg2 = tab;
  for (int part = 0; part < RG_ROWS / WAVE; ++part)
  for (uint64_t lm = longmask[part]; lm; lm &= lm - 1) {  // uniform: every thread reads the same masks
    const int row = part * WAVE + __ffsll((long long)lm) - 1;
    const uint32_t rs = rowstart[row], n = rowstart[row + 1] - rs;
    __syncthreads();  // the previous long row (or the short-row loop) is done with sub* / seg2
    if (t < RG_ROWS) {
      sub[t] = 0;
      subfill[t] = 0;
    }
    __syncthreads();
    for (uint32_t k = t; k < n; k += RG_THREADS) atomicAdd(&sub[(seg[rs + k] & jmask) >> sh], 1u);
    __syncthreads();
    uint32_t c2 = 0, inc2 = 0;
    if (t < RG_ROWS) {
      c2 = sub[t];
      inc2 = wave_incl_scan(c2);
      if (lane == WAVE - 1) wsum[wv] = inc2;
    }
    __syncthreads();
    if (t < RG_ROWS) {
      uint32_t base = 0;
#pragma unroll
      for (int k = 0; k < RG_ROWS / WAVE; ++k)
        if (k < wv) base += wsum[k];
      substart[t] = base + inc2 - c2;
      if (t == RG_ROWS - 1) substart[RG_ROWS] = base + inc2;
    }
    __syncthreads();
    for (uint32_t k = t; k < n; k += RG_THREADS) {
      const uint32_t v = seg[rs + k], b2 = (v & jmask) >> sh;
      seg2[substart[b2] + atomicAdd(&subfill[b2], 1u)] = v;
    }
    __syncthreads();
    for (uint32_t k = t; k < n; k += RG_THREADS) {
      const uint32_t v = seg2[k], b2 = (v & jmask) >> sh;
      const uint32_t bs = substart[b2], be = substart[b2 + 1];
      uint32_t r = 0;
      for (uint32_t q = bs; q < be; ++q) r += seg2[q] < v;
      dst[rs + bs + r] = (ihigh | (uint32_t)row) << 32 | (v & jmask);
    }
  }
  if (t == 0) counts[region] = u;
  __syncthreads();  // the big kernel re-uses the arrays for its next region
  return true;
}

template <typename W>
__global__ __launch_bounds__(RG_THREADS, 8) void region_unique_kernel(const W *__restrict__ in,
                                                                      const uint64_t *__restrict__ starts,
                                                                      const uint64_t *__restrict__ ends,
                                                                      uint64_t *__restrict__ tmp,
                                                                      uint64_t *__restrict__ counts,
                                                                      uint64_t *__restrict__ biglist,
                                                                      unsigned long long *__restrict__ nbig, int gbits,
                                                                      int jbits) {
  const int64_t region = blockIdx.x;
  // words of the region: [starts[r], ends[r]) -- ends = starts + 1 for words sorted by region, its own array for the
  // fixed regions of qrlsh_pair_regions_scatter32
  const int64_t s0 = (int64_t)starts[region], s1 = (int64_t)ends[region];
  if (s0 == s1) {  // uniform
    if (threadIdx.x == 0) counts[region] = 0;
    return;
  }
  if (!region_finish<13, RG_SEG, W>(in, s0, s1, region, tmp, counts, gbits, jbits) && threadIdx.x == 0) {
    // more distinct pairs than this image holds (a few very popular queries): left to the big-image kernel
    counts[region] = 0;
    biglist[__hip_atomic_fetch_add(nbig, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = (uint64_t)region;
  }
}

// Regions the kernel above could not hold: the same finish with a 16384-slot set and a 12288-value segment
// (one workgroup per CU), from a fixed grid that walks the device-side list -- nothing is read back to size
// the launch.  A region beyond THAT raises the overflow word (general path).
constexpr int RG_BIG_SEG = 12288;
constexpr int RG_BIG_GRID = 256;
template <typename W>
__global__ __launch_bounds__(RG_THREADS, 4) void region_unique_big_kernel(const W *__restrict__ in,
                                                                          const uint64_t *__restrict__ starts,
                                                                          const uint64_t *__restrict__ ends,
                                                                          uint64_t *__restrict__ tmp,
                                                                          uint64_t *__restrict__ counts,
                                                                          const uint64_t *__restrict__ biglist,
                                                                          const unsigned long long *__restrict__ nbig,
                                                                          uint64_t *__restrict__ overflow, int gbits,
                                                                          int jbits) {
  const unsigned long long nb = *nbig;
  for (unsigned long long e = blockIdx.x; e < nb; e += gridDim.x) {
    const int64_t region = (int64_t)biglist[e];
    const int64_t s0 = (int64_t)starts[region], s1 = (int64_t)ends[region];
    if (!region_finish<14, RG_BIG_SEG, W>(in, s0, s1, region, tmp, counts, gbits, jbits) && threadIdx.x == 0)
      atomicOr((unsigned long long *)overflow, 1ull);
  }
}

// close the gaps: workgroup r copies its counts[r] words from tmp[starts[r] ..) to out[offs[r] ..)
__global__ __launch_bounds__(256) void region_gather_kernel(const uint64_t *__restrict__ tmp,
                                                            const uint64_t *__restrict__ offs,
                                                            const uint64_t *__restrict__ starts,
                                                            uint64_t *__restrict__ out) {
  const size_t r = blockIdx.x;
  const uint64_t o0 = offs[r], cnt = offs[r + 1] - o0;
  const uint64_t *src = tmp + starts[r];
  for (uint32_t k = threadIdx.x; k < cnt; k += 256) out[o0 + k] = src[k];
}

// workspace: starts[nregions + 1] | counts[nregions + 1] | biglist[nregions] | nbig | chunk totals of the scan |
//            ends[nregions + 1] (fixed-region form only)
static int64_t region_count(int64_t nids, int gbits) { return (nids + (1ll << gbits) - 1) >> gbits; }

struct RegionWs {
  int64_t nr;
  uint64_t *starts, *counts, *biglist, *nbig, *sums, *ends;
};
static RegionWs region_layout(QrCarve &c, int64_t nids, int32_t group_bits) {
  RegionWs w;
  const int64_t nr = w.nr = region_count(nids, group_bits);
  w.starts = c.take<uint64_t>((size_t)(2 * (nr + 1)), 8);   // starts | counts: adjacent
  w.counts = qr_within(w.starts, (size_t)(nr + 1));
  w.biglist = c.take<uint64_t>((size_t)nr, 8);
  w.nbig = c.take<uint64_t>(1, 8);
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(nr + 1, SCANL_CHUNK) + 1), 8);
  w.ends = c.take<uint64_t>((size_t)(nr + 1), 8);
  c.take<uint64_t>(1, 8);   // (a spare word the size has always counted)
  return w;
}
QRLSH_EXPORT size_t qrlsh_region_unique_workspace_bytes(int64_t nids, int32_t group_bits) {
  if (nids <= 0 || group_bits < 0 || group_bits > 8) return 64;
  return QR_LAYOUT_BYTES(region_layout, nids, group_bits);
}

// spans of the fixed regions qrlsh_pair_regions_scatter32 fills: region r = words [r * cap, r * cap + counts[r])
__global__ __launch_bounds__(256) void region_spans_kernel(const uint32_t *__restrict__ counts, int64_t nr, uint32_t cap,
                                                           uint64_t *__restrict__ starts, uint64_t *__restrict__ ends,
                                                           const uint32_t *__restrict__ scatter_ovf,
                                                           uint64_t *__restrict__ ovf_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0 && ovf_out) *ovf_out = *scatter_ovf;   // the scatter's flag rides along: one read-back for both steps
  if (r > nr) return;
  starts[r] = (uint64_t)r * cap;
  ends[r] = (uint64_t)r * cap + (r < nr ? min(counts[r], cap) : 0u);
}

// The two count entry points -- words sorted by region (bounds by binary search, a two-word result) and the fixed regions
// of values qrlsh_pair_regions_scatter32 filled (region r at r * cap, counts[r] values; a three-word result whose last word
// is the scatter's capacity flag) -- share their checks and workspace layout (region_ws) and the launches of the finish.
// checks, clears the out_words result words and (n > 0) lays out the workspace
static int region_ws(const char *name, bool pointers, int64_t n, int32_t group_bits, int32_t id_bits, int64_t nids,
                     void *workspace, size_t workspace_bytes, uint64_t *out, int out_words, hipStream_t st, RegionWs *w) {
  QR_CHECK_ARG(n >= 0 && out && nids > 0 && nids <= (1ll << 32), "%s: bad arguments", name);
  // the 32-bit value (i's low bits, j) must never be the empty-slot marker 0xFFFFFFFF: either it has a spare
  // bit, or the largest j (nids - 1) is not all ones
  // (id_bits <= 31: the kernels build the j mask as (1u << id_bits) - 1)
  QR_CHECK_ARG(group_bits >= 0 && group_bits <= 8 && id_bits >= 1 && id_bits <= 31 && nids <= (1ll << id_bits) &&
                   (group_bits + id_bits < 32 || (group_bits + id_bits == 32 && nids < (1ll << id_bits))),
               "%s: group_bits=%d / id_bits=%d (need group_bits <= 8, id_bits <= 31, group_bits + id_bits <= 32)", name,
               group_bits, id_bits);
  QR_MEMSET(name, out, 0, out_words * sizeof(uint64_t), st);
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(pointers && workspace, "%s: null pointer", name);
  QR_CHECK_WORKSPACE(name, workspace, workspace_bytes, qrlsh_region_unique_workspace_bytes(nids, group_bits));
  QR_CHECK_ARG(region_count(nids, group_bits) <= 2147483647ll, "%s: too many regions", name);
  QrCarve c(workspace);
  *w = region_layout(c, nids, group_bits);
  QR_MEMSET(name, w->counts + w->nr, 0, sizeof(uint64_t), st);
  QR_MEMSET(name, w->nbig, 0, sizeof(uint64_t), st);
  return QRLSH_OK;
}

// the finish of regions [starts[r], ends[r]) of `in`: out2 = {total, distinct-overflow}
template <typename W>
static int region_unique_launch(const char *name, const W *in, const RegionWs &w, const uint64_t *ends, int32_t group_bits,
                                int32_t id_bits, uint64_t *tmp, uint64_t *out2, hipStream_t st) {
  QR_LAUNCH("region_unique", region_unique_kernel<W>, dim3((unsigned)w.nr), dim3(RG_THREADS), 0, st, in,
            (const uint64_t *)w.starts, ends, tmp, w.counts, w.biglist, reinterpret_cast<unsigned long long *>(w.nbig),
            group_bits, id_bits);
  QR_LAUNCH("region_unique_big", region_unique_big_kernel<W>, dim3((unsigned)(w.nr < RG_BIG_GRID ? w.nr : RG_BIG_GRID)),
            dim3(RG_THREADS), 0, st, in, (const uint64_t *)w.starts, ends, tmp, w.counts, (const uint64_t *)w.biglist,
            (const unsigned long long *)w.nbig, out2 + 1, group_bits, id_bits);
  qr_scan_u64(w.counts, w.nr + 1, out2, w.sums, st);
  QR_LAUNCH_CHECK(name);
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_region_unique_count(const uint64_t *grouped, int64_t n, int32_t group_bits, int32_t id_bits,
                                           int64_t nids, uint64_t *tmp, void *workspace, size_t workspace_bytes,
                                           uint64_t *total_overflow_out, void *stream) {
  const char *name = "qrlsh_region_unique_count";
  hipStream_t st = static_cast<hipStream_t>(stream);
  RegionWs w;
  const int rc = region_ws(name, grouped && tmp, n, group_bits, id_bits, nids, workspace, workspace_bytes, total_overflow_out,
                           2, st, &w);
  if (rc != QRLSH_OK || n == 0) return rc;
  QR_LAUNCH("region_bounds", region_bounds_kernel, dim3((unsigned)ceil_div64(w.nr + 1, 256)), dim3(256), 0, st, grouped, n,
            32 + group_bits, w.nr, w.starts);
  return region_unique_launch(name, grouped, w, w.starts + 1, group_bits, id_bits, tmp, total_overflow_out, st);
}

// The same from the fixed regions qrlsh_pair_regions_scatter32 filled with the same group_bits / id_bits / nids (region r =
// regions[r * cap ..), counts[r] values, any order): tmp takes 8-byte pair words, as many as the region buffer has entries;
// n = the number of words scattered (0: nothing to do).  ONE result buffer for the grouping and the finish: out3 = {total,
// distinct-overflow, capacity-overflow}, the last copied from the flag word the scatter wrote on the same stream (a device
// pointer).
QRLSH_EXPORT int qrlsh_region_unique_count_regions32(const uint32_t *regions, const uint32_t *counts, int64_t cap, int64_t n,
                                                     int32_t group_bits, int32_t id_bits, int64_t nids, uint64_t *tmp,
                                                     void *workspace, size_t workspace_bytes,
                                                     const uint32_t *scatter_overflow, uint64_t *out3, void *stream) {
  const char *name = "qrlsh_region_unique_count_regions32";
  QR_CHECK_ARG(counts && scatter_overflow && cap > 0 && cap < (1ll << 32), "%s: bad arguments", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  RegionWs w;
  const int rc = region_ws(name, regions && tmp, n, group_bits, id_bits, nids, workspace, workspace_bytes, out3, 3, st, &w);
  if (rc != QRLSH_OK || n == 0) return rc;
  QR_LAUNCH("region_bounds", region_spans_kernel, dim3((unsigned)ceil_div64(w.nr + 1, 256)), dim3(256), 0, st, counts, w.nr,
            (uint32_t)cap, w.starts, w.ends, scatter_overflow, out3 + 2);
  return region_unique_launch(name, regions, w, w.ends, group_bits, id_bits, tmp, out3, st);
}

QRLSH_EXPORT int qrlsh_region_unique_fill(const uint64_t *tmp, int64_t n, int32_t group_bits, int64_t nids,
                                          const void *workspace, uint64_t *out, void *stream) {
  QR_CHECK_ARG(n >= 0 && nids > 0 && group_bits >= 0 && group_bits <= 8, "qrlsh_region_unique_fill: bad arguments");
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(tmp && workspace && out, "qrlsh_region_unique_fill: null pointer");
  QrCarve c(workspace);
  const RegionWs w = region_layout(c, nids, group_bits);
  const uint64_t *starts = w.starts, *offs = w.counts;   // (the counts, scanned)
  QR_LAUNCH("region_gather", region_gather_kernel, dim3((unsigned)w.nr), dim3(256), 0, static_cast<hipStream_t>(stream), tmp,
            offs, starts, out);
  QR_LAUNCH_CHECK("qrlsh_region_unique_fill");
  return QRLSH_OK;
}

// ---- pair words grouped by REGION without histogram passes (round 4) ------------------------------------------------------
// The region form of the de-duplication (above) needs the emitted words grouped by their region id (i >> g, up to 16
// bits) and NOTHING about the order inside a group.  The stable LSD sort pays for an order nobody reads: per 8-bit pass a
// histogram pass over the words, a scan, and the scatter.  Here the words are dealt most-significant digit first the
// way bucket.hip deals its records, words only: every digit owns a fixed region of `cap` words, a tile counts its
// digits in LDS, reserves room with ONE atomic per (tile, digit) and writes its staged words in runs.  Level 1 deals by the
// high digit of the region id into tmp regions, level 2 deals every tmp region by the low digit into the final regions
// (region r at r * cap, counts[r] words).  One read + one write of the words per level -- 2.1 -> 1.4 ms for the 190 M words
// of the 10 M-query workload.  A region that outgrows its cap raises the flag (the caller groups by sorting instead).
#ifndef QR_PG_IPT
// (this constant governs the single level only -- at most 256 regions; the figures are round 4's, measured when it also
// governed both levels of the flagship's path, which then dealt 8-byte pair words)
#define QR_PG_IPT 32   // 8192-word tiles: runs of 32 - 54 words per (tile, digit); 16: 1.77 ms for the two levels at 10 M, 32: 1.46
#endif
#ifndef QR_PG_IPT_N1
#define QR_PG_IPT_N1 32   // level 1 of the narrow form (6 staged bytes per word, three workgroups per CU): 646 us per launch at 10 M; 40 (two per CU): 689
#endif
#ifndef QR_PG_IPT_N2
#define QR_PG_IPT_N2 40   // level 2 of the narrow form (5 staged bytes per word, 10 240-entry tiles, three per CU): 448 us; 32 (three): 458; 24 (four): 500
#endif
constexpr int PG_IPT = QR_PG_IPT;                 // words per thread of the pair-grouping partition when one level is enough
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
// What a level reads -- IN_WORDS: n_in pair words i << 32 | j; IN_TMP_NARROW: the tmp regions of a first level (OUT_NARROW
// below) -- and what it writes; what is staged is always a 32-bit value and its digit byte or bytes:
//   OUT_VALUES  (the last level only) the 32-bit value (i & gmask) << jbits | j the region de-duplication reduces every word
//               to as its first step -- the region already says every bit of i above the low g.  Staged as the value and a
//               digit byte beside it: 5 bytes per word;
//   OUT_NARROW  (the first of two levels) that same value into a uint32 array and, at the same index of a byte array, the
//               LOW digit of the region id: the tmp region a word lies in says the high digit, the value the bits of i
//               below the region id and j, so the 5 bytes are all the second level needs (13 + 9 = 22 bytes per word
//               over the two levels instead of 16 + 12).  Staged as the value and (high digit << 8 | low digit): 6 bytes.
// The second level masks the tail with dmask: a tmp region that outgrew its capacity (the flag is up, nothing is usable)
// leaves holes of stale bytes below min(count, cap), and a stale tail must still index inside its batch's cursors.
// (1 and 0 were the levels that dealt 8-byte pair words; the numbers are part of the kernels' symbol names, which
// profiles are keyed on, and stay)
enum { PG_IN_WORDS = 0, PG_IN_TMP_NARROW = 2 };
enum { PG_OUT_VALUES = 1, PG_OUT_NARROW = 2 };
constexpr int pg_staged_bytes(int out) { return out == PG_OUT_VALUES ? 5 : 6; }
template <int IN, int OUT, int IPT>
__global__ __launch_bounds__(SORT_THREADS, pg_wgs(IPT, pg_staged_bytes(OUT))) void pair_group_scatter_kernel(
    const void *__restrict__ in_, const uint8_t *__restrict__ in_tails, void *__restrict__ out_, uint8_t *__restrict__ out_tails,
    int64_t n_in, int ntiles, int shift, uint32_t dmask, uint32_t *__restrict__ cursors, uint32_t cap,
    uint32_t *__restrict__ overflow, const uint32_t *__restrict__ in_counts, uint32_t in_cap, int gbits, int jbits, uint32_t bmask) {
  constexpr bool LEVEL2 = IN != PG_IN_WORDS;
  constexpr int TILE = SORT_THREADS * IPT;
  using D = typename std::conditional<OUT == PG_OUT_NARROW, uint16_t, uint8_t>::type;   // the digit(s) staged beside a value
  static_assert(IN == PG_IN_WORDS || IN == PG_IN_TMP_NARROW, "pair words or the tmp regions of a first level");
  static_assert(OUT == PG_OUT_NARROW ? IN == PG_IN_WORDS : OUT == PG_OUT_VALUES, "tmp regions are dealt into the final regions");
  __shared__ uint32_t cnt[RADIX];
  __shared__ uint32_t lsum[SORT_THREADS / WAVE];
  __shared__ uint32_t gdelta[RADIX];
  __shared__ uint8_t gok[RADIX];
  __shared__ __attribute__((aligned(16))) unsigned char stage[TILE * pg_staged_bytes(OUT)];
  uint32_t *const spay = reinterpret_cast<uint32_t *>(stage);
  D *const sdig = reinterpret_cast<D *>(stage + TILE * 4);
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
  uint32_t pay[IPT];
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
      sdig[p] = (D)(dr[k] >> 16);
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
  uint32_t *const out = static_cast<uint32_t *>(out_);
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const uint32_t p = k * SORT_THREADS + threadIdx.x;
    if (p < nstaged) {
      const uint32_t x = spay[p], t = sdig[p];
      const uint32_t d = OUT == PG_OUT_NARROW ? t >> 8 : t;
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

// words (n pair words i << 32 | j, any order) -> regions[r * cap + k], k < counts[r], r = i >> group_bits, as the 32-bit
// values (i & (2^group_bits - 1)) << id_bits | j; counts: uint32 [qrlsh_pair_regions_count + 256] (the tail is level 1's
// cursors); overflow_out: uint32, != 0 when a region outgrew its capacity (nothing usable then).  tmp_regions may be NULL
// when qrlsh_pair_regions_tmp_words is 0.  Needs group_bits + id_bits <= 32 and a value that is never 0xFFFFFFFF
// (qrlsh_region_unique_count_regions32, the only reader, marks empty slots with it).
QRLSH_EXPORT int qrlsh_pair_regions_scatter32(const uint64_t *words, int64_t n, int32_t group_bits, int32_t id_bits,
                                              int64_t nids, double words_per_query, uint64_t *tmp_regions, uint32_t *regions,
                                              uint32_t *counts, uint32_t *overflow_out, void *stream) {
  QR_CHECK_ARG(group_bits >= 0 && group_bits <= 8 && id_bits >= 1 && id_bits <= 31 && nids > 0 && nids <= (1ll << id_bits) &&
                   (group_bits + id_bits < 32 || (group_bits + id_bits == 32 && nids < (1ll << id_bits))),
               "qrlsh_pair_regions_scatter32: group_bits=%d / id_bits=%d / nids=%lld do not fit a 32-bit value", group_bits,
               id_bits, (long long)nids);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) && counts && overflow_out, "qrlsh_pair_regions_scatter32: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PairRegions r = pair_regions(n > 0 ? n : 1, nids, group_bits, words_per_query);
  QR_CHECK_ARG(r.rbits <= 16 && r.na <= RADIX, "qrlsh_pair_regions_scatter32: %d region bits", r.rbits);
  QR_CHECK_ARG(pair_regions_fit_u32(r),
               "qrlsh_pair_regions_scatter32: regions reach 2^32 words (na * cap_a = %llu, 2^rb * cap_b = %llu; need both < 2^32)",
               (unsigned long long)r.na * r.cap_a, (unsigned long long)r.cap_b << r.rb);
  QR_MEMSET("qrlsh_pair_regions_scatter32", counts, 0, ((size_t)r.nregions + RADIX) * sizeof(uint32_t), st);
  QR_MEMSET("qrlsh_pair_regions_scatter32", overflow_out, 0, sizeof(uint32_t), st);
  if (n == 0) return QRLSH_OK;
  QR_CHECK_ARG(words && regions && (r.ra == 0 || tmp_regions), "qrlsh_pair_regions_scatter32: null pointer");
  const int sh = 32 + group_bits;
  const uint32_t *none = nullptr;
  if (r.ra == 0) {
    const int ntiles = (int)ceil_div64(n, SORT_THREADS * PG_IPT);
    QR_LAUNCH("pair_group", (pair_group_scatter_kernel<PG_IN_WORDS, PG_OUT_VALUES, PG_IPT>), dim3(ntiles, 1), dim3(SORT_THREADS), 0, st,
              (const void *)words, (const uint8_t *)nullptr, (void *)regions, (uint8_t *)nullptr, n, ntiles, sh,
              (1u << r.rb) - 1u, counts, r.cap_b, overflow_out, none, 0u, (int)group_bits, (int)id_bits, 0u);
  } else {
    // two levels: tmp holds na * cap_a values, then as many tail bytes (5 of the 8 bytes per entry it was given)
    QR_CHECK_ALIGNED("qrlsh_pair_regions_scatter32", "tmp_regions", qr_addr(tmp_regions), 16);
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
  }
  QR_LAUNCH_CHECK("qrlsh_pair_regions_scatter32");
  return QRLSH_OK;
}
