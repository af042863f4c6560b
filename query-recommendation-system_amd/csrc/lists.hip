// lists.hip -- keeping the per-query top-K neighbour lists current when queries are appended to the index or replaced
// in place: ONE merge, described by its inputs (ListsMerge), behind qrlsh_lists_update_* and qrlsh_lists_replace_*.
//
// The lists of a run over queries 0 .. n-1 (COO src / dst / val, ordered by src, value descending, dst ascending, at
// most K per src) and a BATCH of m queries that has been probed against the index as it is afterwards.  Batch row x is
// query rids[x] when a table is given, else first_id + x.  Every list is already a top-K, so
//   a merged row:   the K best of (its surviving stored entries  U  the batch rows that now name it (milli, id of x)),
//                   a merge of two sequences in the one order "value descending, then neighbour id ascending"
//                   (lists_rec_first);
//   a probed row:   the finish's list, taken as it is -- the batch rows themselves, and the picked rows
// are element for element the lists of a full run with the same K.  What the inputs say:
//   rows:           n rows own stored entries, rows_out rows come out (n + m when the batch is appended, n when it
//                   replaces rows);
//   dropped ids:    an id map of ids whose stored entries and rows drop out (a replaced query's old row and every entry
//                   that names it).  The dropped rows are the batch rows coming back: row id is batch row rank(id), and
//                   the table rids names them.  Null: nothing drops, and then no kept array is allocated, written,
//                   scanned or read, and the batch rows are new rows first_id + x, first_id >= n (an id below n would
//                   be a row that is there already);
//   picked rows:    an id map of rows that are probed again instead of merged (rows of exactly K entries that lose one:
//                   they may need candidates the cut threw away), with their ids and lists.  A row is picked because
//                   an entry of it drops out: there is a pick map only with dropped ids;
//   record ids:     rids[x] with dropped ids, else first_id + x.  Ids without a table lie above every stored id, so a
//                   tie of values always goes to the stored entry and no id is loaded to settle it: "new ids lose ties"
//                   is the one order with ids that happen to be the largest.  The fills are templates on "ids drop out"
//                   (DROP): <false> reads per entry what the append always read.
//
//   reverse edges:   one lane per raw word of the probe: a kept word (select key != ~0) that names a row that is merged
//                    (id < n, not dropped, not picked) becomes the record id << 11 | (1000 - milli) with payload x, every
//                    other word ~0.  qrlsh_sort_u64 over bits [0, 11 + id_bits) orders the records by (row, value
//                    descending); the raw words are ordered by batch row and the sort is stable, so x -- and with it the
//                    record's id -- ascends among equal records; the dropped words (no record has the value field 2047)
//                    end up last.
//   row bookkeeping: run heads / tails of src give every row its stored entries [old_lo, old_hi), run heads / tails of
//                    the sorted records every touched row its reverse run [rev_lo, rev_hi) (both zeroed first: an absent
//                    row is [0, 0)).  With dropped ids, kept[e] = 1 for a stored entry whose dst stays, scanned over all
//                    entries: the surviving entries of a row before entry e are kept[e] - kept[row's first].  len =
//                    min(K, surviving + reverse) for a merged row, the finish's length for a probed one; one scan over
//                    the rows_out rows gives the output offsets and the total.
//   fill:            every element ranks itself.  A surviving stored entry's rank is its place among the row's surviving
//                    entries plus the records of the row's reverse run that order before it (a binary search in the run;
//                    none in the common row without a run: a shifted copy); a record's rank is its place in the run plus
//                    the surviving stored entries that order before it (a binary search in at most K entries).  Ranks
//                    below K are written at out_off[row] + rank.  Nothing walks a row serially.
#include <type_traits>

#include "idmap.h"

constexpr int LU_THREADS = 256;
constexpr int LU_PER = 4;                       // stored entries per lane of the fill, LU_THREADS apart
constexpr int LU_TILE = LU_THREADS * LU_PER;    // stored entries per workgroup step
constexpr int LU_MAXK = QRLSH_INDEX_MAX_K;
constexpr int32_t LU_ABOVE = INT32_MAX;       // above every id (rows_out < 2^31)

struct ListsMerge {
  const int32_t *src, *dst, *val;   // the stored lists
  int64_t n_edges, n, rows_out;
  int K, b;
  const uint2 *drop, *pick;         // id maps over [0, n), or null; pick only with drop
  const uint32_t *rids;             // [m] with drop: the ids of the batch rows (the dropped ids, ascending); else null: first_id + x
  int64_t first_id, m, n_raw;       // n_raw = raw words of the batch's probe
  const int64_t *b_off;             // the batch's lists
  const int32_t *b_idx, *b_milli;
  const uint32_t *pick_ids;         // [n_pick] the picked rows, ascending, and their lists
  int64_t n_pick;
  const int64_t *p_off;
  const int32_t *p_idx, *p_milli;
};

struct LuWs {
  uint64_t *rec_a, *rec_b;                  // [n_raw] records, ping-pong
  uint32_t *pay_a, *pay_b;                  // [n_raw] their batch rows
  uint32_t *old_lo, *old_hi, *rev_lo, *rev_hi;   // [n] each, contiguous (one memset)
  uint64_t *kept;                           // [n_edges + 1] stored entries whose dst stays, then their scan; null
                                            // without dropped ids
  uint64_t *off;                            // [rows_out + 1] lengths, then output offsets; [rows_out] = total
  uint64_t *sums;                           // scan scratch
  uint32_t *bad;                            // != 0: the stored lists break the contract
  void *sort_ws;
  size_t sort_bytes;
};

// n_kept: the stored entries when ids drop out, -1 when none do
static LuWs lu_layout(QrCarve &c, int64_t n, int64_t rows_out, int64_t n_raw, int64_t n_kept) {
  LuWs w;
  const size_t nr = (size_t)n_raw, nn = (size_t)n, rows = (size_t)rows_out;
  w.rec_a = c.take<uint64_t>(nr);
  w.rec_b = c.take<uint64_t>(nr);
  w.pay_a = c.take<uint32_t>(nr);
  w.pay_b = c.take<uint32_t>(nr);
  w.old_lo = c.take<uint32_t>(nn * 4);
  w.old_hi = qr_within(w.old_lo, nn);
  w.rev_lo = qr_within(w.old_lo, 2 * nn);
  w.rev_hi = qr_within(w.old_lo, 3 * nn);
  w.kept = n_kept >= 0 ? c.take<uint64_t>((size_t)(n_kept + 1)) : nullptr;
  w.off = c.take<uint64_t>(rows + 1);
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(n_kept > rows_out ? n_kept : rows_out, SCANL_CHUNK) + 1));
  w.bad = c.take<uint32_t>(4);
  w.sort_bytes = qrlsh_sort_workspace_bytes(n_raw, 1);
  w.sort_ws = c.take_bytes(w.sort_bytes);
  return w;
}
static LuWs lu_layout(const void *workspace, const ListsMerge &g) {
  QrCarve c(workspace);
  return lu_layout(c, g.n, g.rows_out, g.n_raw, g.drop ? g.n_edges : -1);
}

QRLSH_EXPORT size_t qrlsh_lists_update_workspace_bytes(int64_t n, int64_t m, int64_t n_edges, int64_t n_raw) {
  if (n < 0 || m < 0 || n_edges < 0 || n_raw < 0) return 0;
  return QR_LAYOUT_BYTES(lu_layout, n, n + m, n_raw, -1);  // the stored lists are read in place
}

QRLSH_EXPORT size_t qrlsh_lists_replace_workspace_bytes(int64_t n, int64_t n_edges, int64_t n_raw) {
  if (n < 0 || n_edges < 0 || n_raw < 0) return 0;
  return QR_LAYOUT_BYTES(lu_layout, n, n, n_raw, n_edges);
}

// The order of a merged row, between a reverse record and a stored entry: value descending (inv = 1000 - milli
// ascending), then neighbour id ascending.  True when the record goes first.  Both fills decide with it.  Ids without
// a table lie above every stored id: there the fills pass LU_ABOVE for a record and "-1" for an entry in place of loaded
// ids, and the tie goes to the stored entry.
// V: the width the caller compares values in.
template <typename V>
__device__ static inline bool lists_rec_first(V inv_rec, V inv_ent, int32_t rec_id, int32_t ent_id) {
  return inv_rec < inv_ent || (inv_rec == inv_ent && rec_id < ent_id);
}

// one lane per raw word: the reverse-edge record of a kept word that names a merged row
__global__ __launch_bounds__(LU_THREADS) void lists_records_kernel(const uint64_t *__restrict__ raw,
                                                                  const uint64_t *__restrict__ skeys, int64_t n_raw,
                                                                  int64_t n, int64_t m, int b,
                                                                  const uint2 *__restrict__ drop,
                                                                  const uint2 *__restrict__ pick,
                                                                  uint64_t *__restrict__ rec, uint32_t *__restrict__ pay) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_raw) return;
  const uint64_t k = skeys[i];
  const uint64_t x = (raw[i] >> 32) / (uint32_t)b;
  const uint64_t id = k & 0xFFFFFFFFull, inv = k >> 32;
  bool keep = k != ~0ull && (int64_t)id < n && (int64_t)x < m && inv <= 2000;
  if (keep && drop) keep = !idmap_has(drop[id >> 5], (uint32_t)id);
  if (keep && pick) keep = !idmap_has(pick[id >> 5], (uint32_t)id);
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

// one lane per sorted record: run heads and tails of the row id -> [rev_lo, rev_hi) of the row
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

// kept[e] = 1 for a stored entry whose dst does not drop out
__global__ __launch_bounds__(LU_THREADS) void lists_kept_kernel(const int32_t *__restrict__ dst, int64_t n_edges,
                                                               int64_t n, const uint2 *__restrict__ drop,
                                                               uint64_t *__restrict__ kept) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = dst[e];
    kept[e] = d >= 0 && d < n && !idmap_has(drop[d >> 5], (uint32_t)d) ? 1ull : 0ull;
  }
}

// one lane per output row: its length.  A row that is not a stored row any more (dropped) or never was (i >= n) is a
// batch row, a picked row takes its probed list, every other row is merged.
__global__ __launch_bounds__(LU_THREADS) void lists_len_kernel(
    const uint32_t *__restrict__ old_lo, const uint32_t *__restrict__ old_hi, const uint32_t *__restrict__ rev_lo,
    const uint32_t *__restrict__ rev_hi, const uint64_t *__restrict__ kept, int64_t n_edges, int64_t n, int64_t rows_out,
    const uint2 *__restrict__ drop, int64_t first_id, const int64_t *__restrict__ b_off, int64_t m,
    const uint2 *__restrict__ pick, const int64_t *__restrict__ p_off, int64_t n_pick, int K, uint64_t *__restrict__ len) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows_out; i += (int64_t)gridDim.x * blockDim.x) {
    const uint2 dw = drop && i < n ? drop[i >> 5] : make_uint2(0u, 0u);
    const uint2 pw = pick && i < n ? pick[i >> 5] : make_uint2(0u, 0u);
    uint64_t l = 0;
    if (i >= n || idmap_has(dw, (uint32_t)i)) {
      const int64_t j = i >= n ? i - first_id : (int64_t)idmap_rank(dw, (uint32_t)i);
      if (j >= 0 && j < m && b_off[j + 1] > b_off[j]) l = (uint64_t)(b_off[j + 1] - b_off[j]);
    } else if (idmap_has(pw, (uint32_t)i)) {
      const int64_t j = idmap_rank(pw, (uint32_t)i);
      if (j < n_pick && p_off[j + 1] > p_off[j]) l = (uint64_t)(p_off[j + 1] - p_off[j]);
    } else {  // (the four extents are loaded together, before the first is used)
      const uint32_t lo = old_lo[i], hi = old_hi[i], rev = rev_hi[i] - rev_lo[i];
      const bool any = hi > lo && hi <= n_edges;
      l = (kept ? (any ? kept[hi] - kept[lo] : 0ull) : (uint64_t)(any ? hi - lo : 0u)) + rev;
    }
    len[i] = l < (uint64_t)K ? l : (uint64_t)K;
  }
}

// *total_out = the number of entries of the new lists, or ~0 when the stored lists break the contract
__global__ void lists_total_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ bad,
                                   uint64_t *__restrict__ total_out) {
  if (threadIdx.x == 0) *total_out = *bad ? ~0ull : *total;
}

// stored entries, LU_PER per lane (consecutive lanes on consecutive entries): a surviving entry of a merged row ranks
// itself = its place among the row's surviving entries + records of the row's reverse run that order before it.
// DROP: ids drop out and come back as the batch rows (drop, kept and the id table are read)
template <bool DROP>
__global__ __launch_bounds__(LU_THREADS) void lists_fill_old_kernel(
    const int32_t *__restrict__ src, const int32_t *__restrict__ dst, const int32_t *__restrict__ val, int64_t n_edges,
    int64_t n, int K, const uint2 *__restrict__ drop, const uint2 *__restrict__ pick, const uint32_t *__restrict__ rids,
    int64_t m, const uint32_t *__restrict__ old_lo, const uint32_t *__restrict__ rev_lo,
    const uint32_t *__restrict__ rev_hi, const uint64_t *__restrict__ rec, const uint32_t *__restrict__ pay,
    const uint64_t *__restrict__ kept, const uint64_t *__restrict__ out_off, int64_t total, int32_t *__restrict__ src_out,
    int32_t *__restrict__ dst_out, int32_t *__restrict__ val_out) {
  const int64_t ntiles = (n_edges + LU_TILE - 1) / LU_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t e0 = tile * LU_TILE + threadIdx.x;
    int32_t s[LU_PER], d[LU_PER], v[LU_PER];
    uint64_t kp[LU_PER];
#pragma unroll
    for (int k = 0; k < LU_PER; ++k) {  // every load of the step is issued before the first is used
      const int64_t e = e0 + (int64_t)k * LU_THREADS;
      const bool live = e < n_edges;
      s[k] = live ? src[e] : -1;
      d[k] = live ? dst[e] : 0;
      v[k] = live ? val[e] : 0;
      kp[k] = DROP && live ? kept[e] : 0;
    }
#pragma unroll
    for (int k = 0; k < LU_PER; ++k) {
      const int64_t e = e0 + (int64_t)k * LU_THREADS;
      const int64_t i = s[k], dd = d[k];
      if (i < 0 || i >= n) continue;
      if (DROP && (dd < 0 || dd >= n || idmap_has(drop[i >> 5], (uint32_t)i) || idmap_has(drop[dd >> 5], (uint32_t)dd)))
        continue;
      if (DROP && pick && idmap_has(pick[i >> 5], (uint32_t)i)) continue;  // (a row is picked because it loses an entry)
      const uint32_t lo = old_lo[i];
      uint32_t L = rev_lo[i], R = rev_hi[i];
      const uint32_t base = L;
      // (64-bit values without dropped ids, as the append's kernel always compared them: with 32-bit ones the compiler
      // holds the third extent load of a step's first entry back behind a wait, 3 % of the kernel at one new query)
      typedef typename std::conditional<DROP, int32_t, int64_t>::type inv_t;
      const inv_t inv = 1000 - v[k];
      while (L < R) {
        const uint32_t mid = L + (R - L) / 2;
        const uint64_t r = rec[mid];
        int32_t rid = LU_ABOVE;
        if (DROP) {
          const uint32_t x = pay[mid];
          if ((int64_t)x < m) rid = (int32_t)rids[x];
        }
        if (lists_rec_first((inv_t)(r & 2047u), inv, rid, d[k])) L = mid + 1;
        else R = mid;
      }
      const int64_t place = DROP ? (int64_t)(kp[k] - kept[lo]) : e - (int64_t)lo;
      const int64_t rank = place + (int64_t)(L - base);
      if (rank < 0 || rank >= K) continue;
      const int64_t o = (int64_t)out_off[i] + rank;
      if (o >= total) continue;  // never, for offsets the count wrote
      src_out[o] = (int32_t)i;
      dst_out[o] = d[k];
      val_out[o] = v[k];
    }
  }
}

// sorted records, one lane each: rank = place in the run + surviving stored entries of the row that order before it
template <bool DROP>
__global__ __launch_bounds__(LU_THREADS) void lists_fill_rev_kernel(
    const uint64_t *__restrict__ rec, const uint32_t *__restrict__ pay, int64_t n_raw, int64_t n, int K,
    const uint32_t *__restrict__ rids, int64_t first_id, int64_t m, const int32_t *__restrict__ dst,
    const int32_t *__restrict__ val, int64_t n_edges, const uint32_t *__restrict__ old_lo,
    const uint32_t *__restrict__ old_hi, const uint32_t *__restrict__ rev_lo, const uint64_t *__restrict__ kept,
    const uint64_t *__restrict__ out_off, int64_t total, int32_t *__restrict__ src_out, int32_t *__restrict__ dst_out,
    int32_t *__restrict__ val_out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_raw) return;
  const uint64_t r = rec[k];
  if (r == ~0ull) return;
  const int64_t id = (int64_t)(r >> 11);
  if (id >= n) return;  // never, for a record the records kernel wrote
  const int32_t inv = (int32_t)(r & 2047u);
  int32_t rid = LU_ABOVE;
  if (DROP) {  // a table's id settles ties: read before the search
    const uint32_t x = pay[k];
    if ((int64_t)x >= m) return;
    rid = (int32_t)rids[x];
  }
  uint32_t L = old_lo[id], R = old_hi[id];
  if (R > (uint64_t)n_edges) R = (uint32_t)n_edges;
  if (L > R) L = R;
  const uint32_t lo = L;
  while (L < R) {  // the stored row is in the one order: the first entry that orders after the record
    const uint32_t mid = L + (R - L) / 2;
    const int32_t iv = 1000 - val[mid];
    if (!lists_rec_first(inv, iv, rid, DROP && iv == inv ? dst[mid] : -1)) L = mid + 1;  // (dst only at a tie)
    else R = mid;
  }
  const int64_t before = DROP ? (int64_t)(kept[L] - kept[lo]) : (int64_t)(L - lo);
  const int64_t rank = (k - (int64_t)rev_lo[id]) + before;
  if (rank < 0 || rank >= K) return;
  const int64_t o = (int64_t)out_off[id] + rank;
  if (o >= total) return;
  if (!DROP) rid = (int32_t)(first_id + pay[k]);  // only a record that is written needs its id
  src_out[o] = (int32_t)id;
  dst_out[o] = rid;
  val_out[o] = 1000 - inv;
}

// the probed lists: entry k of list j, which is row ids[j] or first_id + j
__global__ __launch_bounds__(LU_THREADS) void lists_fill_probed_kernel(
    const int64_t *__restrict__ off, const int32_t *__restrict__ idx, const int32_t *__restrict__ milli,
    const uint32_t *__restrict__ ids, int64_t first_id, int64_t count, int K, const uint64_t *__restrict__ base,
    int64_t base_rows, bool base_by_id, int64_t total, int32_t *__restrict__ src_out, int32_t *__restrict__ dst_out,
    int32_t *__restrict__ val_out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count * K) return;
  const int64_t j = g / K;
  const int k = (int)(g - j * K);
  const uint32_t id = ids ? ids[j] : (uint32_t)(first_id + j);
  const int64_t at = base_by_id ? (int64_t)id : j;
  if (at >= base_rows) return;
  // (loaded beside the offsets, not behind them: for a list without an entry k the base is read and not used -- the
  // removal's pick_base slot of a row whose head entry never wrote it is the zero its count put there)
  const uint64_t o = base[at] + (uint32_t)k;
  const int64_t a = off[j] + k;
  if (a >= off[j + 1] || o >= (uint64_t)total) return;
  src_out[o] = (int32_t)id;
  dst_out[o] = idx[a];
  val_out[o] = milli[a];
}

void qr_lists_old_rows(const int32_t *src, const int32_t *dst, int64_t n_edges, int64_t n, uint32_t *old_lo,
                       uint32_t *old_hi, uint32_t *bad, hipStream_t st) {
  QR_LAUNCH("lists_old_rows", lists_old_rows_kernel, dim3(rm_grid(n_edges, LU_THREADS)), dim3(LU_THREADS), 0, st, src, dst,
            n_edges, n, old_lo, old_hi, bad);
}
void qr_lists_rev_rows(const uint64_t *rec, int64_t n_raw, int64_t n, uint32_t *rev_lo, uint32_t *rev_hi, hipStream_t st) {
  QR_LAUNCH("lists_rev_rows", lists_rev_rows_kernel, dim3((unsigned)ceil_div64(n_raw, LU_THREADS)), dim3(LU_THREADS), 0, st,
            rec, n_raw, n, rev_lo, rev_hi);
}
void qr_lists_fill_probed(const int64_t *off, const int32_t *idx, const int32_t *milli, const uint32_t *ids,
                          int64_t first_id, int64_t count, int K, const uint64_t *base, int64_t base_rows, bool base_by_id,
                          int64_t total, int32_t *src_out, int32_t *dst_out, int32_t *val_out, hipStream_t st) {
  if (count <= 0 || !idx || !milli) return;  // (no probed list has an entry when the finish wrote none: its arrays may be empty)
  QR_LAUNCH("lists_fill_probed", lists_fill_probed_kernel, dim3((unsigned)ceil_div64(count * K, LU_THREADS)),
            dim3(LU_THREADS), 0, st, off, idx, milli, ids, first_id, count, K, base, base_rows, base_by_id, total, src_out,
            dst_out, val_out);
}

// the count of the merge: records, row bookkeeping, lengths, offsets; *total_out = the entries of the new lists (~0:
// the stored lists break the contract).  `who` names the entry point in an error
static int lists_merge_count(const char *who, const ListsMerge &g, const uint64_t *raw, const uint64_t *skeys,
                             void *workspace, uint64_t *total_out, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LuWs w = lu_layout(workspace, g);
  const bool rows = g.n_edges > 0 && g.n > 0;
  QR_MEMSET(who, w.bad, g.n_edges > 0 && !rows ? 0xFF : 0, 16, st);  // entries without rows to belong to
  if (g.rows_out == 0) QR_MEMSET(who, w.off, 0, sizeof(uint64_t), st);
  if (g.n > 0) QR_MEMSET(who, w.old_lo, 0, (size_t)g.n * 16, st);
  if (w.kept) QR_MEMSET(who, w.kept, 0, sizeof(uint64_t), st);
  const dim3 block(LU_THREADS);
  if (g.n_raw > 0) {
    QR_LAUNCH("lists_records", lists_records_kernel, dim3((unsigned)ceil_div64(g.n_raw, LU_THREADS)), block, 0, st, raw,
              skeys, g.n_raw, g.n, g.m, g.b, g.drop, g.pick, w.rec_a, w.pay_a);
    const int where = qrlsh_sort_u64(w.rec_a, w.rec_b, w.pay_a, w.pay_b, g.n_raw, 1, 0, 11 + qr_id_bits(g.n), 0, 0,
                                     w.sort_ws, w.sort_bytes, stream);
    if (where < 0) return where;
    if (where == 1) {  // the sorted records are always left in rec_a / pay_a
      QR_MEMCPY(who, w.rec_a, w.rec_b, (size_t)g.n_raw * 8, st);
      QR_MEMCPY(who, w.pay_a, w.pay_b, (size_t)g.n_raw * 4, st);
    }
    if (g.n > 0) qr_lists_rev_rows(w.rec_a, g.n_raw, g.n, w.rev_lo, w.rev_hi, st);
  }
  if (rows) {
    qr_lists_old_rows(g.src, g.dst, g.n_edges, g.n, w.old_lo, w.old_hi, w.bad, st);
    if (w.kept) {
      QR_LAUNCH("lists_kept", lists_kept_kernel, dim3(rm_grid(g.n_edges, LU_THREADS)), block, 0, st, g.dst, g.n_edges, g.n,
                g.drop, w.kept);
      qr_scan_u64(w.kept, g.n_edges, w.kept + g.n_edges, w.sums, st);
    }
  }
  if (g.rows_out > 0) {
    QR_LAUNCH("lists_len", lists_len_kernel, dim3(rm_grid(g.rows_out, LU_THREADS)), block, 0, st,
              (const uint32_t *)w.old_lo, (const uint32_t *)w.old_hi, (const uint32_t *)w.rev_lo,
              (const uint32_t *)w.rev_hi, (const uint64_t *)w.kept, g.n_edges, g.n, g.rows_out, g.drop, g.first_id, g.b_off,
              g.m, g.pick, g.p_off, g.n_pick, g.K, w.off);
    qr_scan_u64(w.off, g.rows_out, w.off + g.rows_out, w.sums, st);
  }
  QR_LAUNCH("lists_total", lists_total_kernel, dim3(1), dim3(64), 0, st, (const uint64_t *)(w.off + g.rows_out),
            (const uint32_t *)w.bad, total_out);
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}

// the fill of the merge, over the workspace its count left
static int lists_merge_fill(const char *who, const ListsMerge &g, const void *workspace, int64_t total, int32_t *src_out,
                            int32_t *dst_out, int32_t *val_out, void *stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LuWs w = lu_layout(workspace, g);
  const dim3 block(LU_THREADS);
  if (g.n_edges > 0 && g.n > 0)
    QR_LAUNCH("lists_fill_old", g.drop ? lists_fill_old_kernel<true> : lists_fill_old_kernel<false>,
              dim3(rm_grid(g.n_edges, LU_TILE)), block, 0, st, g.src, g.dst, g.val, g.n_edges, g.n, g.K, g.drop, g.pick,
              g.rids, g.m, (const uint32_t *)w.old_lo, (const uint32_t *)w.rev_lo, (const uint32_t *)w.rev_hi,
              (const uint64_t *)w.rec_a, (const uint32_t *)w.pay_a, (const uint64_t *)w.kept, (const uint64_t *)w.off,
              total, src_out, dst_out, val_out);
  if (g.n_raw > 0 && g.n > 0)
    QR_LAUNCH("lists_fill_rev", g.drop ? lists_fill_rev_kernel<true> : lists_fill_rev_kernel<false>,
              dim3((unsigned)ceil_div64(g.n_raw, LU_THREADS)), block, 0, st, (const uint64_t *)w.rec_a,
              (const uint32_t *)w.pay_a, g.n_raw, g.n, g.K, g.rids, g.first_id, g.m, g.dst, g.val, g.n_edges,
              (const uint32_t *)w.old_lo, (const uint32_t *)w.old_hi, (const uint32_t *)w.rev_lo, (const uint64_t *)w.kept,
              (const uint64_t *)w.off, total, src_out, dst_out, val_out);
  qr_lists_fill_probed(g.b_off, g.b_idx, g.b_milli, g.rids, g.first_id, g.m, g.K, w.off, g.rows_out, true, total, src_out,
                       dst_out, val_out, st);
  qr_lists_fill_probed(g.p_off, g.p_idx, g.p_milli, g.pick_ids, 0, g.n_pick, g.K, w.off, g.rows_out, true, total, src_out,
                       dst_out, val_out, st);
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}

// ---- appended queries: nothing drops, no row is picked, batch row x is the new query n + x -------------------------
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
  QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, qrlsh_lists_update_workspace_bytes(n, m, n_edges, n_raw));
  return QRLSH_OK;
}

static ListsMerge lu_merge(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                           int64_t m, int32_t b, int32_t K, int64_t n_raw, const int64_t *new_off, const int32_t *new_idx,
                           const int32_t *new_milli) {
  return ListsMerge{src, dst, val, n_edges, n, n + m, (int)K, (int)b, nullptr, nullptr, nullptr, n, m, n_raw, new_off,
                    new_idx, new_milli, nullptr, 0, nullptr, nullptr, nullptr};
}

QRLSH_EXPORT int qrlsh_lists_update_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                          int64_t n, int64_t m, int32_t b, int32_t K, const uint64_t *raw,
                                          const uint64_t *select_keys, int64_t n_raw, const int64_t *new_off,
                                          void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(total_out, "qrlsh_lists_update_count: null total_out");
  const int rc = lu_args("qrlsh_lists_update_count", src, dst, val, n_edges, n, m, b, K, raw, select_keys, n_raw, new_off,
                         workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  return lists_merge_count("qrlsh_lists_update_count",
                           lu_merge(src, dst, val, n_edges, n, m, b, K, n_raw, new_off, nullptr, nullptr), raw, select_keys,
                           workspace, total_out, stream);
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
  return lists_merge_fill("qrlsh_lists_update_fill",
                          lu_merge(src, dst, val, n_edges, n, m, b, K, n_raw, new_off, new_idx, new_milli), workspace,
                          total, src_out, dst_out, val_out, stream);
}

// ---- replaced queries: the ids of R drop out and come back as the batch rows, rows that lose an entry are picked ----
static int rl_args(const char *who, const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                   int64_t m, int32_t b, int32_t K, const void *replaced_map, const uint32_t *replaced_ids,
                   const void *pick_map, const uint32_t *pick_ids, int64_t n_pick, int64_t n_raw, const int64_t *r_off,
                   const int64_t *p_off, const void *workspace, size_t workspace_bytes) {
  QR_CHECK_ARG(K >= 1 && K <= LU_MAXK, "%s: K=%d not in [1, %d]", who, K, LU_MAXK);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31) && m >= 1 && m <= n && n_pick >= 0 &&
                   n_pick <= n - m && n_raw >= 0 && n_raw < (1ll << 32) && b > 0 && b <= 65535 &&
                   m * (int64_t)b < (1ll << 32),
               "%s: bad sizes n=%lld n_edges=%lld m=%lld n_pick=%lld n_raw=%lld b=%d", who, (long long)n,
               (long long)n_edges, (long long)m, (long long)n_pick, (long long)n_raw, b);
  QR_CHECK_ARG(replaced_map && replaced_ids && r_off && workspace && (n_edges == 0 || (src && dst && val)) &&
                   (n_pick == 0 || (pick_map && pick_ids && p_off)),
               "%s: null pointer", who);
  QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, qrlsh_lists_replace_workspace_bytes(n, n_edges, n_raw));
  return QRLSH_OK;
}

static ListsMerge rl_merge(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                           int64_t m, int32_t b, int32_t K, const void *replaced_map, const uint32_t *replaced_ids,
                           const void *pick_map, const uint32_t *pick_ids, int64_t n_pick, int64_t n_raw,
                           const int64_t *r_off, const int32_t *r_idx, const int32_t *r_milli, const int64_t *p_off,
                           const int32_t *p_idx, const int32_t *p_milli) {
  const uint2 *pk = n_pick > 0 ? idmap_layout(pick_map, n).w : nullptr;
  return ListsMerge{src, dst, val, n_edges, n, n, (int)K, (int)b, idmap_layout(replaced_map, n).w, pk,
                    replaced_ids, 0, m, n_raw, r_off, r_idx, r_milli, pick_ids, n_pick, p_off, p_idx, p_milli};
}

QRLSH_EXPORT int qrlsh_lists_replace_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                           int64_t n, int64_t m, int32_t b, int32_t K, const void *replaced_map,
                                           const uint32_t *replaced_ids, const void *pick_map, const uint32_t *pick_ids,
                                           int64_t n_pick, const uint64_t *raw, const uint64_t *select_keys, int64_t n_raw,
                                           const int64_t *r_off, const int64_t *p_off, void *workspace,
                                           size_t workspace_bytes, uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(total_out, "qrlsh_lists_replace_count: null total_out");
  const int rc = rl_args("qrlsh_lists_replace_count", src, dst, val, n_edges, n, m, b, K, replaced_map, replaced_ids,
                         pick_map, pick_ids, n_pick, n_raw, r_off, p_off, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(n_raw == 0 || (raw && select_keys), "qrlsh_lists_replace_count: null pointer");
  return lists_merge_count("qrlsh_lists_replace_count",
                           rl_merge(src, dst, val, n_edges, n, m, b, K, replaced_map, replaced_ids, pick_map, pick_ids,
                                    n_pick, n_raw, r_off, nullptr, nullptr, p_off, nullptr, nullptr),
                           raw, select_keys, workspace, total_out, stream);
}

QRLSH_EXPORT int qrlsh_lists_replace_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges,
                                          int64_t n, int64_t m, int32_t b, int32_t K, const void *replaced_map,
                                          const uint32_t *replaced_ids, const void *pick_map, const uint32_t *pick_ids,
                                          int64_t n_pick, int64_t n_raw, const int64_t *r_off, const int32_t *r_idx,
                                          const int32_t *r_milli, const int64_t *p_off, const int32_t *p_idx,
                                          const int32_t *p_milli, const void *workspace, size_t workspace_bytes,
                                          int64_t total, int32_t *src_out, int32_t *dst_out, int32_t *val_out,
                                          void *stream) {
  const int rc = rl_args("qrlsh_lists_replace_fill", src, dst, val, n_edges, n, m, b, K, replaced_map, replaced_ids,
                         pick_map, pick_ids, n_pick, n_raw, r_off, p_off, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  QR_CHECK_ARG(total >= 0 && total <= n * (int64_t)K, "qrlsh_lists_replace_fill: bad total %lld", (long long)total);
  if (total == 0) return QRLSH_OK;
  QR_CHECK_ARG(src_out && dst_out && val_out, "qrlsh_lists_replace_fill: null pointer");
  return lists_merge_fill("qrlsh_lists_replace_fill",
                          rl_merge(src, dst, val, n_edges, n, m, b, K, replaced_map, replaced_ids, pick_map, pick_ids,
                                   n_pick, n_raw, r_off, r_idx, r_milli, p_off, p_idx, p_milli),
                          workspace, total, src_out, dst_out, val_out, stream);
}
