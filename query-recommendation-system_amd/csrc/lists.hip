// lists.hip -- keeping the per-query top-K neighbour lists current when queries are appended to the index.
//
// The lists of a run over queries 0 .. n-1 (COO src / dst / val, ordered by src, value descending, dst ascending, at
// most K per src) and a batch of m appended queries n .. n+m-1 that has been probed against the GROWN index with the
// indexed finish (qrlsh_index_probe_finish_indexed, first_id = n).  Every list is already a top-K, so
//   old row i < n:   the K best of (its stored row  U  its new neighbours (milli, n + x)) -- a merge of two sorted
//                    sequences, the new ids losing ties (they are larger than every old id);
//   new row n + x:   the finish's list of x (its K best candidates among all n + m queries, itself excluded)
// are element for element the lists of a full run over all n + m queries with the same K.
//
//   reverse edges:   one lane per raw word of the probe: a kept word (select key != ~0) with id < n becomes the record
//                    id << 11 | (1000 - milli) with payload x = its probe query, every other word ~0.  qrlsh_sort_u64
//                    over bits [0, 11 + id_bits) orders the records by (old id, value descending); the raw words are
//                    ordered by probe query and the sort is stable, so x ascends among equal records; the dropped
//                    words (no record has the value field 2047) end up last.
//   row bookkeeping: run heads / tails of src give every old row its stored entries [old_lo, old_hi), run heads / tails
//                    of the sorted records every touched row its reverse run [rev_lo, rev_hi) (both zeroed first:
//                    an absent row is [0, 0)); len_out[i] = min(K, stored + reverse), the new rows take theirs from
//                    the finish's offsets; one scan over the n + m rows gives the output offsets and the total.
//   fill:            every element ranks itself.  A stored entry's rank is its place in the row plus the records of
//                    the row's reverse run that order before it (a binary search in the run; none in the common row
//                    without a run: a shifted copy); a record's rank is its place in the run plus the stored entries
//                    that order before it (a binary search in at most K entries).  Ranks below K are written at
//                    out_off[row] + rank.  Nothing walks a row serially.
#include "common.h"

constexpr int LU_THREADS = 256;
constexpr int LU_PER = 4;                       // stored entries per lane of the fill, LU_THREADS apart
constexpr int LU_TILE = LU_THREADS * LU_PER;    // stored entries per workgroup step
constexpr int LU_MAXK = QRLSH_INDEX_MAX_K;
constexpr int LU_GRID = 2048;                   // workgroups of the grid-stride kernels (256 CUs x 8)

static inline size_t lu_al16(size_t x) { return (x + 15) / 16 * 16; }

static inline int lu_id_bits(int64_t n) {
  int bits = 1;
  while (bits < 32 && (1ll << bits) < n) ++bits;
  return bits;
}

struct LuWs {
  uint64_t *rec_a, *rec_b;                  // [n_raw] records, ping-pong
  uint32_t *pay_a, *pay_b;                  // [n_raw] their probe queries
  uint32_t *old_lo, *old_hi, *rev_lo, *rev_hi;   // [n] each, contiguous (one memset)
  uint64_t *off;                            // [n + m + 1] lengths, then output offsets; [n + m] = total
  uint64_t *sums;                           // scan scratch
  uint32_t *bad;                            // != 0: the stored lists break the contract
  void *sort_ws;
  size_t sort_bytes, total;
};

static LuWs lu_layout(void *workspace, int64_t n, int64_t m, int64_t n_raw) {
  LuWs w;
  char *p = static_cast<char *>(workspace);
  size_t o = 0;
  const size_t nr = (size_t)(n_raw > 0 ? n_raw : 0), nn = (size_t)(n > 0 ? n : 0), rows = (size_t)(n + m);
  w.rec_a = reinterpret_cast<uint64_t *>(p + o), o += lu_al16(nr * 8);
  w.rec_b = reinterpret_cast<uint64_t *>(p + o), o += lu_al16(nr * 8);
  w.pay_a = reinterpret_cast<uint32_t *>(p + o), o += lu_al16(nr * 4);
  w.pay_b = reinterpret_cast<uint32_t *>(p + o), o += lu_al16(nr * 4);
  w.old_lo = reinterpret_cast<uint32_t *>(p + o);
  w.old_hi = w.old_lo + nn;
  w.rev_lo = w.old_hi + nn;
  w.rev_hi = w.rev_lo + nn;
  o += lu_al16(nn * 16);
  w.off = reinterpret_cast<uint64_t *>(p + o), o += lu_al16((rows + 1) * 8);
  w.sums = reinterpret_cast<uint64_t *>(p + o), o += lu_al16((size_t)(ceil_div64((int64_t)rows, SCANL_CHUNK) + 1) * 8);
  w.bad = reinterpret_cast<uint32_t *>(p + o), o += 16;
  w.sort_ws = p + o;
  w.sort_bytes = qrlsh_sort_workspace_bytes(n_raw > 0 ? n_raw : 0, 1);
  o += lu_al16(w.sort_bytes);
  w.total = o;
  return w;
}

QRLSH_EXPORT size_t qrlsh_lists_update_workspace_bytes(int64_t n, int64_t m, int64_t n_edges, int64_t n_raw) {
  if (n < 0 || m < 0 || n_edges < 0 || n_raw < 0) return 0;
  (void)n_edges;  // the stored lists are read in place
  return lu_layout(nullptr, n, m, n_raw).total;
}

// one lane per raw word: the reverse-edge record of a kept word that names an old query
__global__ __launch_bounds__(LU_THREADS) void lists_records_kernel(const uint64_t *__restrict__ raw,
                                                                  const uint64_t *__restrict__ skeys, int64_t n_raw,
                                                                  int64_t n, int64_t m, int b,
                                                                  uint64_t *__restrict__ rec, uint32_t *__restrict__ pay) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_raw) return;
  const uint64_t k = skeys[i];
  const uint64_t x = (raw[i] >> 32) / (uint32_t)b;
  const uint64_t id = k & 0xFFFFFFFFull, inv = k >> 32;
  const bool keep = k != ~0ull && (int64_t)id < n && (int64_t)x < m && inv <= 2000;
  rec[i] = keep ? (id << 11 | inv) : ~0ull;
  pay[i] = (uint32_t)x;
}

// one lane per stored entry: run heads and tails of src -> [old_lo, old_hi) of the row; *bad when src is not
// ascending, or an id lies outside [0, n)
__global__ __launch_bounds__(LU_THREADS) void lists_old_rows_kernel(const int32_t *__restrict__ src,
                                                                   const int32_t *__restrict__ dst, int64_t n_edges,
                                                                   int64_t n, uint32_t *__restrict__ old_lo,
                                                                   uint32_t *__restrict__ old_hi,
                                                                   uint32_t *__restrict__ bad) {
  bool wrong = false;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = src[e], d = dst[e];
    const int64_t sp = e > 0 ? (int64_t)src[e - 1] : -1;
    const int64_t sn = e + 1 < n_edges ? (int64_t)src[e + 1] : n;
    if (s < 0 || s >= n || d < 0 || d >= n || sp > s) {
      wrong = true;
      continue;
    }
    if (sp != s) old_lo[s] = (uint32_t)e;
    if (sn != s) old_hi[s] = (uint32_t)(e + 1);
  }
  if (__ballot(wrong) && lane_id() == 0) atomicOr(bad, 1u);
}

// one lane per sorted record: run heads and tails of the old id -> [rev_lo, rev_hi) of the row
__global__ __launch_bounds__(LU_THREADS) void lists_rev_rows_kernel(const uint64_t *__restrict__ rec, int64_t n_raw,
                                                                   int64_t n, uint32_t *__restrict__ rev_lo,
                                                                   uint32_t *__restrict__ rev_hi) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_raw) return;
  const uint64_t r = rec[k];
  if (r == ~0ull) return;
  const uint64_t id = r >> 11;
  if ((int64_t)id >= n) return;  // never, for a record the records kernel wrote
  const uint64_t rp = k > 0 ? rec[k - 1] : ~0ull;
  const uint64_t rn = k + 1 < n_raw ? rec[k + 1] : ~0ull;
  if (rp == ~0ull || (rp >> 11) != id) rev_lo[id] = (uint32_t)k;
  if (rn == ~0ull || (rn >> 11) != id) rev_hi[id] = (uint32_t)(k + 1);
}

// one lane per row of the updated lists: its length
__global__ __launch_bounds__(LU_THREADS) void lists_len_kernel(const uint32_t *__restrict__ old_lo,
                                                              const uint32_t *__restrict__ old_hi,
                                                              const uint32_t *__restrict__ rev_lo,
                                                              const uint32_t *__restrict__ rev_hi,
                                                              const int64_t *__restrict__ new_off, int64_t n, int64_t m,
                                                              int K, uint64_t *__restrict__ len) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + m; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t l;
    if (i < n) {
      const uint32_t lo = old_lo[i], hi = old_hi[i];
      l = (uint64_t)(hi > lo ? hi - lo : 0) + (rev_hi[i] - rev_lo[i]);
    } else {
      const int64_t a = new_off[i - n], e = new_off[i - n + 1];
      l = e > a ? (uint64_t)(e - a) : 0;
    }
    len[i] = l < (uint64_t)K ? l : (uint64_t)K;
  }
}

// *total_out = the number of entries of the updated lists, or ~0 when the stored lists break the contract
__global__ void lists_total_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ bad,
                                   uint64_t *__restrict__ total_out) {
  if (threadIdx.x == 0) *total_out = *bad ? ~0ull : *total;
}

// stored entries, LU_PER per lane (consecutive lanes on consecutive entries): rank = place in the row + records of the
// row's reverse run with a larger value
__global__ __launch_bounds__(LU_THREADS) void lists_fill_old_kernel(
    const int32_t *__restrict__ src, const int32_t *__restrict__ dst, const int32_t *__restrict__ val, int64_t n_edges,
    int64_t n, int K, const uint32_t *__restrict__ old_lo, const uint32_t *__restrict__ rev_lo,
    const uint32_t *__restrict__ rev_hi, const uint64_t *__restrict__ rec, const uint64_t *__restrict__ out_off,
    int64_t total, int32_t *__restrict__ src_out, int32_t *__restrict__ dst_out, int32_t *__restrict__ val_out) {
  const int64_t ntiles = (n_edges + LU_TILE - 1) / LU_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t e0 = tile * LU_TILE + threadIdx.x;
    int32_t s[LU_PER], d[LU_PER], v[LU_PER];
#pragma unroll
    for (int k = 0; k < LU_PER; ++k) {  // every load of the step is issued before the first is used
      const int64_t e = e0 + (int64_t)k * LU_THREADS;
      const bool live = e < n_edges;
      s[k] = live ? src[e] : -1;
      d[k] = live ? dst[e] : 0;
      v[k] = live ? val[e] : 0;
    }
#pragma unroll
    for (int k = 0; k < LU_PER; ++k) {
      const int64_t e = e0 + (int64_t)k * LU_THREADS;
      const int64_t i = s[k];
      if (i < 0 || i >= n) continue;
      const uint32_t lo = old_lo[i];
      uint32_t L = rev_lo[i], R = rev_hi[i];
      const uint32_t base = L;
      const uint64_t inv = (uint64_t)(int64_t)(1000 - v[k]);  // a record orders before the entry iff its value is larger
      while (L < R) {
        const uint32_t mid = L + (R - L) / 2;
        if ((int64_t)(rec[mid] & 2047u) < (int64_t)inv) L = mid + 1;
        else R = mid;
      }
      const int64_t rank = (e - (int64_t)lo) + (int64_t)(L - base);
      if (rank < 0 || rank >= K) continue;
      const int64_t o = (int64_t)out_off[i] + rank;
      if (o >= total) continue;  // never, for offsets the count wrote
      src_out[o] = (int32_t)i;
      dst_out[o] = d[k];
      val_out[o] = v[k];
    }
  }
}

// sorted records, one lane each: rank = place in the run + stored entries of the row whose value is at least as large
__global__ __launch_bounds__(LU_THREADS) void lists_fill_rev_kernel(
    const uint64_t *__restrict__ rec, const uint32_t *__restrict__ pay, int64_t n_raw, int64_t n, int K,
    const int32_t *__restrict__ val, int64_t n_edges, const uint32_t *__restrict__ old_lo,
    const uint32_t *__restrict__ old_hi, const uint32_t *__restrict__ rev_lo, const uint64_t *__restrict__ out_off,
    int64_t total, int32_t *__restrict__ src_out, int32_t *__restrict__ dst_out, int32_t *__restrict__ val_out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_raw) return;
  const uint64_t r = rec[k];
  if (r == ~0ull) return;
  const int64_t id = (int64_t)(r >> 11);
  if (id >= n) return;
  const int32_t mi = 1000 - (int32_t)(r & 2047u);
  uint32_t L = old_lo[id], R = old_hi[id];
  if (R > (uint64_t)n_edges) R = (uint32_t)n_edges;
  if (L > R) L = R;
  const uint32_t lo = L;
  while (L < R) {  // stored values descend: the first entry with a smaller value
    const uint32_t mid = L + (R - L) / 2;
    if (val[mid] >= mi) L = mid + 1;
    else R = mid;
  }
  const int64_t rank = (k - (int64_t)rev_lo[id]) + (int64_t)(L - lo);
  if (rank < 0 || rank >= K) return;
  const int64_t o = (int64_t)out_off[id] + rank;
  if (o >= total) return;
  src_out[o] = (int32_t)id;
  dst_out[o] = (int32_t)(n + pay[k]);
  val_out[o] = mi;
}

// the new rows: the finish's lists with src = n + x
__global__ __launch_bounds__(LU_THREADS) void lists_fill_new_kernel(const int64_t *__restrict__ new_off,
                                                                   const int32_t *__restrict__ new_idx,
                                                                   const int32_t *__restrict__ new_milli, int64_t n,
                                                                   int64_t m, int K, const uint64_t *__restrict__ out_off,
                                                                   int64_t total, int32_t *__restrict__ src_out,
                                                                   int32_t *__restrict__ dst_out,
                                                                   int32_t *__restrict__ val_out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m * K) return;
  const int64_t x = g / K, k = g - x * K;
  const int64_t a = new_off[x];
  if (k >= new_off[x + 1] - a) return;
  const int64_t o = (int64_t)out_off[n + x] + k;
  if (o >= total) return;
  src_out[o] = (int32_t)(n + x);
  dst_out[o] = new_idx[a + k];
  val_out[o] = new_milli[a + k];
}

static int lu_args(const char *who, const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                   int64_t m, int32_t b, int32_t K, const uint64_t *raw, const uint64_t *skeys, int64_t n_raw,
                   const int64_t *new_off, const void *workspace, size_t workspace_bytes) {
  QR_CHECK_ARG(K >= 1 && K <= LU_MAXK, "%s: K=%d not in [1, %d]", who, K, LU_MAXK);
  QR_CHECK_ARG(n >= 0 && m >= 0 && n_edges >= 0 && n_raw >= 0 && b > 0 && b <= 65535,
               "%s: bad sizes n=%lld m=%lld n_edges=%lld n_raw=%lld b=%d", who, (long long)n, (long long)m,
               (long long)n_edges, (long long)n_raw, b);
  QR_CHECK_ARG(n + m < (1ll << 31) && n_edges < (1ll << 31) && n_raw < (1ll << 32) && m * (int64_t)b < (1ll << 32),
               "%s: n + m and n_edges must stay below 2^31, n_raw and m * b below 2^32", who);
  QR_CHECK_ARG(workspace && (n_edges == 0 || (src && dst && val)) && (n_raw == 0 || (raw && skeys)) && (m == 0 || new_off),
               "%s: null pointer", who);
  if (workspace_bytes < qrlsh_lists_update_workspace_bytes(n, m, n_edges, n_raw)) {
    qrlsh_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes,
                    qrlsh_lists_update_workspace_bytes(n, m, n_edges, n_raw));
    return QRLSH_EWORKSPACE;
  }
  return QRLSH_OK;
}

static inline unsigned lu_grid(int64_t work, int64_t per_block) {
  const int64_t g = ceil_div64(work, per_block);
  return (unsigned)(g < LU_GRID ? (g > 0 ? g : 1) : LU_GRID);
}

// the row bookkeeping of stored lists and of sorted reverse records, also for the replacement's lists (replace.hip)
void qr_lists_old_rows(const int32_t *src, const int32_t *dst, int64_t n_edges, int64_t n, uint32_t *old_lo,
                       uint32_t *old_hi, uint32_t *bad, hipStream_t st) {
  QR_LAUNCH("lists_old_rows", lists_old_rows_kernel, dim3(lu_grid(n_edges, LU_THREADS)), dim3(LU_THREADS), 0, st, src, dst,
            n_edges, n, old_lo, old_hi, bad);
}
void qr_lists_rev_rows(const uint64_t *rec, int64_t n_raw, int64_t n, uint32_t *rev_lo, uint32_t *rev_hi, hipStream_t st) {
  QR_LAUNCH("lists_rev_rows", lists_rev_rows_kernel, dim3((unsigned)ceil_div64(n_raw, LU_THREADS)), dim3(LU_THREADS), 0, st,
            rec, n_raw, n, rev_lo, rev_hi);
}

QRLSH_EXPORT int qrlsh_lists_update_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                          int64_t n, int64_t m, int32_t b, int32_t K, const uint64_t *raw,
                                          const uint64_t *select_keys, int64_t n_raw, const int64_t *new_off,
                                          void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(total_out, "qrlsh_lists_update_count: null total_out");
  const int rc = lu_args("qrlsh_lists_update_count", src, dst, val, n_edges, n, m, b, K, raw, select_keys, n_raw, new_off,
                         workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LuWs w = lu_layout(workspace, n, m, n_raw);
  if (hipMemsetAsync(w.bad, 0, 16, st) != hipSuccess ||
      (n + m == 0 && hipMemsetAsync(w.off, 0, sizeof(uint64_t), st) != hipSuccess) ||
      (n > 0 && hipMemsetAsync(w.old_lo, 0, (size_t)n * 16, st) != hipSuccess)) {
    qrlsh_set_error("qrlsh_lists_update_count: hipMemsetAsync failed");
    return QRLSH_EHIP;
  }
  if (n_raw > 0) {
    QR_LAUNCH("lists_records", lists_records_kernel, dim3((unsigned)ceil_div64(n_raw, LU_THREADS)), dim3(LU_THREADS), 0, st,
              raw, select_keys, n_raw, n, m, (int)b, w.rec_a, w.pay_a);
    const int where = qrlsh_sort_u64(w.rec_a, w.rec_b, w.pay_a, w.pay_b, n_raw, 1, 0, 11 + lu_id_bits(n), 0, 0, w.sort_ws,
                                     w.sort_bytes, stream);
    if (where < 0) return where;
    if (where == 1) {  // the sorted records are always left in rec_a / pay_a
      if (hipMemcpyAsync(w.rec_a, w.rec_b, (size_t)n_raw * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(w.pay_a, w.pay_b, (size_t)n_raw * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        qrlsh_set_error("qrlsh_lists_update_count: hipMemcpyAsync failed");
        return QRLSH_EHIP;
      }
    }
    if (n > 0) qr_lists_rev_rows(w.rec_a, n_raw, n, w.rev_lo, w.rev_hi, st);
  }
  if (n_edges > 0 && n > 0) qr_lists_old_rows(src, dst, n_edges, n, w.old_lo, w.old_hi, w.bad, st);
  else if (n_edges > 0) {  // entries without rows to belong to
    if (hipMemsetAsync(w.bad, 0xFF, 4, st) != hipSuccess) {
      qrlsh_set_error("qrlsh_lists_update_count: hipMemsetAsync failed");
      return QRLSH_EHIP;
    }
  }
  if (n + m > 0) {
    QR_LAUNCH("lists_len", lists_len_kernel, dim3(lu_grid(n + m, LU_THREADS)), dim3(LU_THREADS), 0, st,
              (const uint32_t *)w.old_lo, (const uint32_t *)w.old_hi, (const uint32_t *)w.rev_lo,
              (const uint32_t *)w.rev_hi, new_off, n, m, (int)K, w.off);
    qr_scan_u64(w.off, n + m, w.off + (n + m), w.sums, st);
  }
  QR_LAUNCH("lists_total", lists_total_kernel, dim3(1), dim3(64), 0, st, (const uint64_t *)(w.off + (n + m)),
            (const uint32_t *)w.bad, total_out);
  QR_LAUNCH_CHECK("qrlsh_lists_update_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_lists_update_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                         int64_t n, int64_t m, int32_t b, int32_t K, int64_t n_raw, const int64_t *new_off,
                                         const int32_t *new_idx, const int32_t *new_milli, const void *workspace,
                                         size_t workspace_bytes, int64_t total, int32_t *src_out, int32_t *dst_out,
                                         int32_t *val_out, void *stream) {
  const int rc = lu_args("qrlsh_lists_update_fill", src, dst, val, n_edges, n, m, b, K, (const uint64_t *)workspace,
                         (const uint64_t *)workspace, n_raw, new_off, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(total >= 0 && total <= (n + m) * (int64_t)K, "qrlsh_lists_update_fill: bad total %lld", (long long)total);
  if (total == 0) return QRLSH_OK;
  QR_CHECK_ARG(src_out && dst_out && val_out, "qrlsh_lists_update_fill: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LuWs w = lu_layout(const_cast<void *>(workspace), n, m, n_raw);
  if (n_edges > 0 && n > 0)
    QR_LAUNCH("lists_fill_old", lists_fill_old_kernel, dim3(lu_grid(n_edges, LU_TILE)), dim3(LU_THREADS), 0, st, src, dst, val,
              n_edges, n, (int)K, (const uint32_t *)w.old_lo, (const uint32_t *)w.rev_lo, (const uint32_t *)w.rev_hi,
              (const uint64_t *)w.rec_a, (const uint64_t *)w.off, total, src_out, dst_out, val_out);
  if (n_raw > 0 && n > 0)
    QR_LAUNCH("lists_fill_rev", lists_fill_rev_kernel, dim3((unsigned)ceil_div64(n_raw, LU_THREADS)), dim3(LU_THREADS), 0, st,
              (const uint64_t *)w.rec_a, (const uint32_t *)w.pay_a, n_raw, n, (int)K, val, n_edges,
              (const uint32_t *)w.old_lo, (const uint32_t *)w.old_hi, (const uint32_t *)w.rev_lo, (const uint64_t *)w.off,
              total, src_out, dst_out, val_out);
  if (m > 0 && new_idx && new_milli)  // (no new list has an entry when the finish wrote none: its arrays may be empty)
    QR_LAUNCH("lists_fill_new", lists_fill_new_kernel, dim3((unsigned)ceil_div64(m * K, LU_THREADS)), dim3(LU_THREADS), 0, st,
              new_off, new_idx, new_milli, n, m, (int)K, (const uint64_t *)w.off, total, src_out, dst_out, val_out);
  QR_LAUNCH_CHECK("qrlsh_lists_update_fill");
  return QRLSH_OK;
}
