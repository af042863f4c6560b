// index.hip -- serving new queries: a band-key index built once from a finished hot-path run, probed many times.
//
// Reference: LSH.get_candidates (lsh.py:40-55) and the neighbour lists of compute_querySimilarities
// (recommender.py:187-214) for a query x that was NOT in the indexed set: its candidates are the indexed ids that
// share with it a band whose r int16 values are equal and not all -1, its list the top K of them by rounded cosine.
//
//   build:  per band, (key, id) sorted by the top 32 bits of mix64(key) (qrlsh_sort_u64, QRLSH_SORT_MIX, 4 passes;
//           equal keys adjacent up to 32-bit mix collisions, ids ascending) and a directory over the top d bits of
//           mix64(key): dir[t][h] = first position of band t whose mix bits are >= h.
//   probe:  one lane per (new query, band): two directory words, a binary search for the run of equal top-32 mix
//           bits, then a full-key compare over that run (a run longer than IX_SERIAL records -- a popular key -- is
//           scanned by the whole wave).  count -> exclusive scan -> fill writes the raw candidate words
//           (q * b + band) << 32 | id, duplicates across bands included.
//   finish: one lane per raw word checks the candidate's row against the probe's row band by band and keeps the
//           word only if its band is the FIRST band with equal, non-empty int16 values.  That one test drops
//           duplicates (a candidate is kept once, at its first shared band), verifies hashed keys of wide bands and
//           drops caller keys that collide, with no sort.  The same pass computes the exact integer dot product
//           and score.hip's expression milli = rint(dot / (sqrt(na) * sqrt(nb)) * 1000).  A kept word becomes the
//           key (1000 - milli) << 32 | id.  Then one workgroup per new query streams its keys through an LDS
//           image of IX_CAP keys.  Keys below the current K-th are appended; a full image is sorted and cut to K.
//           Short lists take one pass and one sort, long lists (a popular key) several; the route is decided on
//           the device.  An exclusive scan of min(K, avail) gives the CSR offsets, and a compaction writes the
//           lists.
#include "common.h"

constexpr int IX_MAXK = 256;    // longest neighbour list a probe returns
constexpr int IX_CAP = 4096;    // keys in the LDS image of the per-query select (32 KB)
constexpr int IX_SERIAL = 32;   // runs of equal mix bits longer than this are scanned by the whole wave

// directory bits for n indexed queries: about 4 - 8 records per directory entry, so the directory is 1/2 - 1/4 of
// a word per record (<= 1/24 of the 12 bytes of key + id the band holds) and a probe's run is found in ~3 steps
QRLSH_EXPORT int32_t qrlsh_index_dir_bits(int64_t n) {
  int lg = 0;
  while (lg < 62 && (1ll << lg) < n) ++lg;
  int d = lg - 3;
  if (d < 1) d = 1;
  if (d > 26) d = 26;
  return d;
}

QRLSH_EXPORT size_t qrlsh_index_dir_words(int64_t n, int32_t b) {
  if (n < 0 || b <= 0) return 0;
  return (size_t)b * (((size_t)1 << qrlsh_index_dir_bits(n)) + 1);
}

QRLSH_EXPORT size_t qrlsh_index_build_workspace_bytes(int64_t n, int32_t b) { return qrlsh_sort_workspace_bytes(n, b); }

// dir[t][h] = first position of sorted band t whose top d mix bits are >= h, h = 0 .. 2^d (dir[t][2^d] = n)
__global__ __launch_bounds__(256) void index_dir_kernel(const uint64_t *__restrict__ keys, int64_t n, int d,
                                                        uint32_t *__restrict__ dir) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t t = blockIdx.y;
  const uint64_t *k = keys + t * n;
  uint32_t *dr = dir + t * ((1ll << d) + 1);
  const int64_t h = (int64_t)(qr_mix64(k[i]) >> (64 - d));
  const int64_t hp = i == 0 ? -1 : (int64_t)(qr_mix64(k[i - 1]) >> (64 - d));
  for (int64_t x = hp + 1; x <= h; ++x) dr[x] = (uint32_t)i;
  if (i == n - 1)
    for (int64_t x = h + 1; x <= (1ll << d); ++x) dr[x] = (uint32_t)n;
}

// the directory of b sorted bands of n > 0 records (also what qrlsh_index_remove runs over its output)
int qr_index_dir(const uint64_t *keys, int64_t n, int32_t b, uint32_t *dir_out, hipStream_t st, const char *who) {
  QR_LAUNCH("index_dir", index_dir_kernel, dim3((unsigned)ceil_div64(n, 256), (unsigned)b), dim3(256), 0, st, keys, n,
            (int)qrlsh_index_dir_bits(n), dir_out);
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_index_build(uint64_t *keys, uint64_t *keys_tmp, uint32_t *ids, uint32_t *ids_tmp, int64_t n,
                                   int32_t b, uint32_t *dir_out, void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && b > 0 && b <= 65535, "qrlsh_index_build: bad sizes n=%lld b=%d",
               (long long)n, b);
  QR_CHECK_ARG(dir_out, "qrlsh_index_build: null directory");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    QR_MEMSET("qrlsh_index_build", dir_out, 0, qrlsh_index_dir_words(n, b) * sizeof(uint32_t), st);
    return QRLSH_OK;
  }
  QR_CHECK_ARG(keys && keys_tmp && ids && ids_tmp, "qrlsh_index_build: null pointer");
  const int rc = qrlsh_sort_u64(keys, keys_tmp, ids, ids_tmp, n, b, 32, 64, QRLSH_SORT_MIX | QRLSH_SORT_IOTA, 0,
                                workspace, workspace_bytes, stream);
  if (rc < 0) return rc;
  if (rc == 1) {  // the result is always left in keys / ids
    QR_MEMCPY("qrlsh_index_build", keys, keys_tmp, (size_t)b * n * sizeof(uint64_t), st);
    QR_MEMCPY("qrlsh_index_build", ids, ids_tmp, (size_t)b * n * sizeof(uint32_t), st);
  }
  return qr_index_dir(keys, n, b, dir_out, st, "qrlsh_index_build");
}

// ---- probe: count / fill ------------------------------------------------------------------------------------------
__device__ static inline uint32_t ix_top32(uint64_t k) { return (uint32_t)(qr_mix64(k) >> 32); }

// [a, e): the records of band bk whose top 32 mix bits equal those of key
__device__ static inline void ix_run(const uint64_t *bk, const uint32_t *bdir, int d, uint64_t key, uint32_t &a,
                                     uint32_t &e) {
  const uint64_t h = qr_mix64(key);
  const uint64_t slot = h >> (64 - d);
  const uint32_t T = (uint32_t)(h >> 32);
  uint32_t L = bdir[slot], R = bdir[slot + 1];
  const uint32_t hi = R;
  while (L < R) {
    const uint32_t mid = L + (R - L) / 2;
    if (ix_top32(bk[mid]) < T) L = mid + 1;
    else R = mid;
  }
  a = L;
  R = hi;
  while (L < R) {
    const uint32_t mid = L + (R - L) / 2;
    if (ix_top32(bk[mid]) <= T) L = mid + 1;
    else R = mid;
  }
  e = L;
}

// one lane per g = q * b + t (new query q, band t).  count: cnt[g] = records of band t with key == probe key;
// fill: the same records, raw[cnt[g] + c] = g << 32 | id (cnt = exclusive scan)
template <bool FILL>
__global__ __launch_bounds__(256) void index_probe_kernel(const uint64_t *__restrict__ skeys,
                                                          const uint32_t *__restrict__ sids, int64_t n, int b, int r,
                                                          int d, const uint32_t *__restrict__ dir,
                                                          const uint64_t *__restrict__ pkeys, int64_t m,
                                                          uint64_t *__restrict__ cnt, uint64_t *__restrict__ raw) {
  const int lane = lane_id();
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = g < m * b;
  const int64_t q = live ? g / b : 0;
  const int t = live ? (int)(g - q * b) : 0;
  const uint64_t key = live ? pkeys[(int64_t)t * m + q] : 0;
  const bool act = live && key != qr_empty_key(r);
  const int64_t dw = (1ll << d) + 1;
  uint32_t a = 0, e = 0;
  if (act) ix_run(skeys + (int64_t)t * n, dir + (int64_t)t * dw, d, key, a, e);
  const uint64_t pos = (FILL && live) ? cnt[g] : 0;
  const uint64_t tag = (uint64_t)g << 32;
  uint64_t c = 0;
  const bool longrun = act && e - a > (uint32_t)IX_SERIAL;
  if (act && !longrun) {
    const uint64_t *bk = skeys + (int64_t)t * n;
    const uint32_t *bi = sids + (int64_t)t * n;
    for (uint32_t x = a; x < e; ++x)
      if (bk[x] == key) {
        if (FILL) raw[pos + c] = tag | bi[x];
        ++c;
      }
  }
  // popular keys: the wave takes the long runs of its lanes one after the other, 64 records per step
  uint64_t lm = __ballot(longrun);
  while (lm) {
    const int src = __ffsll((long long)lm) - 1;
    lm &= lm - 1;
    const uint32_t ra = __shfl(a, src, WAVE), re = __shfl(e, src, WAVE);
    const uint64_t rk = __shfl(key, src, WAVE);
    const int rt = __shfl(t, src, WAVE);
    const uint64_t rpos = __shfl(pos, src, WAVE), rtag = __shfl(tag, src, WAVE);
    const uint64_t *bk = skeys + (int64_t)rt * n;
    const uint32_t *bi = sids + (int64_t)rt * n;
    uint64_t rc = 0;
    for (uint32_t x0 = ra; x0 < re; x0 += WAVE) {
      const uint32_t x = x0 + lane;
      const bool hit = x < re && bk[x] == rk;
      const uint64_t hm = __ballot(hit);
      if (FILL && hit) raw[rpos + rc + __popcll(hm & ((1ull << lane) - 1))] = rtag | bi[x];
      rc += __popcll(hm);
    }
    if (lane == src) c = rc;
  }
  if (!FILL && live) cnt[g] = c;
}

// workspace: cnt / offsets u64 [m * b + 1] | scan sums
struct ProbeWs {
  uint64_t *cnt, *sums;
};
static ProbeWs probe_layout(QrCarve &c, int64_t m, int32_t b) {
  const int64_t mb = m * b;
  ProbeWs w;
  w.cnt = c.take<uint64_t>((size_t)(mb + 1), 8);
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(mb, SCANL_CHUNK) + 1), 8);
  return w;
}
QRLSH_EXPORT size_t qrlsh_index_probe_workspace_bytes(int64_t m, int32_t b) {
  if (m <= 0 || b <= 0) return 0;
  return QR_LAYOUT_BYTES(probe_layout, m, b);
}

static int probe_args(const char *who, const uint64_t *skeys, const uint32_t *dir, int64_t n, int32_t b, int32_t r,
                      const uint64_t *pkeys, int64_t m, const void *workspace, size_t workspace_bytes) {
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && b > 0 && b <= 65535 && r > 0 && m >= 0, "%s: bad sizes n=%lld b=%d r=%d m=%lld",
               who, (long long)n, b, r, (long long)m);
  QR_CHECK_ARG(m * (int64_t)b < (1ll << 32), "%s: m * b = %lld must stay below 2^32", who, (long long)(m * (int64_t)b));
  if (m == 0) return QRLSH_OK;
  QR_CHECK_ARG(pkeys && workspace && (n == 0 || (skeys && dir)), "%s: null pointer", who);
  QR_CHECK_WORKSPACE(who, workspace, workspace_bytes, qrlsh_index_probe_workspace_bytes(m, b));
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_index_probe_count(const uint64_t *sorted_keys, const uint32_t *dir, int64_t n, int32_t b, int32_t r,
                                         const uint64_t *probe_keys, int64_t m, void *workspace, size_t workspace_bytes,
                                         uint64_t *total_out, void *stream) {
  QR_CHECK_ARG(total_out, "qrlsh_index_probe_count: null total_out");
  const int rc = probe_args("qrlsh_index_probe_count", sorted_keys, dir, n, b, r, probe_keys, m, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m == 0) {
    QR_MEMSET("qrlsh_index_probe_count", total_out, 0, sizeof(uint64_t), st);
    return QRLSH_OK;
  }
  const int64_t mb = m * b;
  QrCarve c(workspace);
  const ProbeWs w = probe_layout(c, m, b);
  uint64_t *cnt = w.cnt, *sums = w.sums;
  if (n == 0) {
    QR_MEMSET("qrlsh_index_probe_count", cnt, 0, (size_t)(mb + 1) * sizeof(uint64_t), st);
  } else {
    QR_LAUNCH("index_probe_count", index_probe_kernel<false>, dim3((unsigned)ceil_div64(mb, 256)), dim3(256), 0, st,
              sorted_keys, nullptr, n, b, r, qrlsh_index_dir_bits(n), dir, probe_keys, m, cnt, nullptr);
    qr_scan_u64(cnt, mb, cnt + mb, sums, st);
  }
  QR_MEMCPY("qrlsh_index_probe_count", total_out, cnt + mb, sizeof(uint64_t), st);
  QR_LAUNCH_CHECK("qrlsh_index_probe_count");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_index_probe_fill(const uint64_t *sorted_keys, const uint32_t *sorted_ids, const uint32_t *dir,
                                        int64_t n, int32_t b, int32_t r, const uint64_t *probe_keys, int64_t m,
                                        const void *workspace, size_t workspace_bytes, uint64_t *raw_out, void *stream) {
  const int rc = probe_args("qrlsh_index_probe_fill", sorted_keys, dir, n, b, r, probe_keys, m, workspace, workspace_bytes);
  if (rc != QRLSH_OK) return rc;
  if (m == 0 || n == 0) return QRLSH_OK;
  QR_CHECK_ARG(sorted_ids && raw_out, "qrlsh_index_probe_fill: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t mb = m * b;
  QrCarve c(workspace);
  QR_LAUNCH("index_probe_fill", index_probe_kernel<true>, dim3((unsigned)ceil_div64(mb, 256)), dim3(256), 0, st,
            sorted_keys, sorted_ids, n, b, r, qrlsh_index_dir_bits(n), dir, probe_keys, m,
            probe_layout(c, m, b).cnt, raw_out);
  QR_LAUNCH_CHECK("qrlsh_index_probe_fill");
  return QRLSH_OK;
}

// ---- finish: dedupe + verify + score, select, cut ------------------------------------------------------------------
__device__ static inline int64_t ix_val(int32_t v) { return v; }
__device__ static inline int64_t ix_val(uint16_t v) { return v == 0xFFFFu ? -1 : (int64_t)v; }

// one lane per raw word g << 32 | id: key (1000 - milli) << 32 | id if band g % b is the first band the two rows
// share, else ~0 (a duplicate, or a key collision).  first_id >= 0: probe row q IS indexed query first_id + q, and the
// word that names it (the query finding itself) is dropped like a duplicate; self_ids: probe row q is indexed query
// self_ids[q] instead (scattered rows); first_id < 0 and no self_ids: the probe rows are strangers
template <typename SigT>
__global__ __launch_bounds__(256) void index_score_kernel(const SigT *__restrict__ sig, const int64_t *__restrict__ norm2,
                                                          int64_t n, const SigT *__restrict__ psig,
                                                          const int64_t *__restrict__ pnorm2, int P, int b, int64_t m,
                                                          const uint64_t *__restrict__ raw, int64_t n_raw,
                                                          int64_t first_id, const uint32_t *__restrict__ self_ids,
                                                          uint64_t *__restrict__ keys_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_raw) return;
  const uint64_t w = raw[i];
  const uint32_t id = (uint32_t)w;
  const int64_t g = (int64_t)(w >> 32);
  const int64_t q = g / b;
  const int t = (int)(g - q * b);
  if ((int64_t)id >= n || q >= m) {  // not a word the fill pass writes
    keys_out[i] = ~0ull;
    return;
  }
  const int64_t self = self_ids ? (int64_t)self_ids[q] : (first_id >= 0 ? first_id + q : -1);
  if ((int64_t)id == self) {  // q itself
    keys_out[i] = ~0ull;
    return;
  }
  const SigT *a = sig + (int64_t)id * P;
  const SigT *c = psig + q * P;
  const int r = P / b;
  int first = -1;
  int64_t dot = 0, na = 0, nb = 0;
  for (int band = 0; band < b; ++band) {
    bool eq = true, empty = true;
    for (int k = 0; k < r; ++k) {
      const SigT x = a[band * r + k], y = c[band * r + k];
      const uint32_t ux = (uint32_t)x & 0xFFFFu, uy = (uint32_t)y & 0xFFFFu;
      eq &= ux == uy;
      empty &= ux == 0xFFFFu;
      const int64_t vx = ix_val(x), vy = ix_val(y);
      dot += vx * vy;
      na += vx * vx;
      nb += vy * vy;
    }
    if (first < 0 && eq && !empty) {
      first = band;
      if (first != t) break;  // not this word's band: dropped, no score needed
    }
  }
  if (first != t) {
    keys_out[i] = ~0ull;
    return;
  }
  if (norm2) na = norm2[id];
  if (pnorm2) nb = pnorm2[q];
  double cs = 0.0;
  if (na != 0 && nb != 0) cs = (double)dot / (sqrt((double)na) * sqrt((double)nb));
  const int32_t mi = (int32_t)rint(cs * 1000.0);
  keys_out[i] = ((uint64_t)(uint32_t)(1000 - mi) << 32) | id;
}

// exclusive prefix of p over the 256-thread block; *total = number of p
__device__ static inline uint32_t ix_block_prefix(bool p, uint32_t *wc, uint32_t *total) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const uint64_t bal = __ballot(p);
  if (lane == 0) wc[w] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < w) base += wc[k];
    tot += wc[k];
  }
  __syncthreads();
  *total = tot;
  return base + (uint32_t)__popcll(bal & ((1ull << lane) - 1));
}

// ascending bitonic sort of buf[0 .. cnt) (padded to a power of two with ~0)
__device__ static inline void ix_sort(uint64_t *buf, uint32_t cnt) {
  uint32_t n2 = 2;
  while (n2 < cnt) n2 <<= 1;
  for (uint32_t x = cnt + threadIdx.x; x < n2; x += blockDim.x) buf[x] = ~0ull;
  __syncthreads();
  for (uint32_t k = 2; k <= n2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t x = threadIdx.x; x < n2; x += blockDim.x) {
        const uint32_t y = x ^ j;
        if (y > x) {
          const uint64_t u = buf[x], v = buf[y];
          if ((u > v) == ((x & k) == 0)) {
            buf[x] = v;
            buf[y] = u;
          }
        }
      }
      __syncthreads();
    }
}

// one workgroup per new query: the K smallest keys of its raw segment (and how many were kept) -> pidx / pmilli [m][K],
// avail[q], cut[q] = min(K, avail)
__global__ __launch_bounds__(256) void index_select_kernel(const uint64_t *__restrict__ keys,
                                                           const uint64_t *__restrict__ seg, int b, int K,
                                                           int32_t *__restrict__ pidx, int32_t *__restrict__ pmilli,
                                                           int32_t *__restrict__ avail, uint64_t *__restrict__ cut) {
  __shared__ uint64_t buf[IX_CAP];
  __shared__ uint32_t wc[4];
  const int64_t q = blockIdx.x;
  const uint64_t s0 = seg[q * b], s1 = seg[(q + 1) * b];
  uint32_t fill = 0;            // uniform
  uint64_t thresh = ~0ull;      // uniform: keys at or above it cannot make the cut
  uint32_t kept = 0;
  for (uint64_t base = s0; base < s1; base += blockDim.x) {
    const uint64_t x = base + threadIdx.x;
    const uint64_t v = x < s1 ? keys[x] : ~0ull;
    kept += v != ~0ull;
    bool take = v < thresh;
    uint32_t ns;
    uint32_t pos = ix_block_prefix(take, wc, &ns);
    if (fill + ns > (uint32_t)IX_CAP) {  // the image is full: keep its K best, raise the bar
      ix_sort(buf, fill);
      fill = fill < (uint32_t)K ? fill : (uint32_t)K;
      if (fill == (uint32_t)K) thresh = buf[K - 1];
      __syncthreads();
      take = v < thresh;
      pos = ix_block_prefix(take, wc, &ns);
    }
    if (take) buf[fill + pos] = v;
    fill += ns;
    __syncthreads();
  }
  ix_sort(buf, fill);
  const uint32_t nout = fill < (uint32_t)K ? fill : (uint32_t)K;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    const bool in = (uint32_t)k < nout;
    const uint64_t v = buf[in ? k : 0];
    pidx[q * K + k] = in ? (int32_t)(uint32_t)v : -1;
    pmilli[q * K + k] = in ? 1000 - (int32_t)(v >> 32) : 0;
  }
  // kept total: a wave sum, then the block's (ix_sort ended on a barrier: wc is free)
  uint32_t s = kept;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) s += __shfl_xor(s, o, WAVE);
  if (lane_id() == 0) wc[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t all = wc[0] + wc[1] + wc[2] + wc[3];
    avail[q] = (int32_t)all;
    cut[q] = nout;
  }
}

// lists of the padded [m][K] image -> CSR at off[q]
__global__ __launch_bounds__(256) void index_compact_kernel(const int32_t *__restrict__ pidx,
                                                            const int32_t *__restrict__ pmilli, int64_t m, int K,
                                                            const int64_t *__restrict__ off, int32_t *__restrict__ idx,
                                                            int32_t *__restrict__ milli) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m * K) return;
  const int64_t q = g / K, k = g - q * K;
  const int64_t lo = off[q];
  if (k < off[q + 1] - lo) {
    idx[lo + k] = pidx[g];
    milli[lo + k] = pmilli[g];
  }
}

// workspace: keys u64 [n_raw] | pidx i32 [m][K] | pmilli i32 [m][K] | scan sums
struct FinishWs {
  uint64_t *keys, *sums;
  int32_t *pidx, *pmilli;
};
static FinishWs finish_layout(QrCarve &c, int64_t m, int32_t K, int64_t n_raw) {
  FinishWs w;
  w.keys = c.take<uint64_t>((size_t)n_raw);
  w.pidx = c.take<int32_t>((size_t)m * K);
  w.pmilli = c.take<int32_t>((size_t)m * K);
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(m, SCANL_CHUNK) + 1), 8);
  return w;
}
QRLSH_EXPORT size_t qrlsh_index_finish_workspace_bytes(int64_t m, int32_t K, int64_t n_raw) {
  if (m <= 0 || K <= 0 || K > IX_MAXK || n_raw < 0) return 0;
  return QR_LAYOUT_BYTES(finish_layout, m, K, n_raw);
}

static int ix_finish(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig, const int64_t *probe_norm2,
                     int32_t sig_dtype, int32_t P, int32_t b, int64_t m, const void *probe_workspace, const uint64_t *raw,
                     int64_t n_raw, int32_t K, int64_t first_id, const uint32_t *self_ids, int64_t *off_out, int32_t *idx_out,
                     int32_t *milli_out,
                     int32_t *avail_out, void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(K >= 1 && K <= IX_MAXK, "qrlsh_index_probe_finish: K=%d not in [1, %d]", K, IX_MAXK);
  QR_CHECK_ARG(n >= 0 && n < (1ll << 32) - 1 && m >= 0 && n_raw >= 0 && P > 0 && b > 0 && b <= 65535 && P % b == 0,
               "qrlsh_index_probe_finish: bad sizes n=%lld m=%lld n_raw=%lld P=%d b=%d", (long long)n, (long long)m,
               (long long)n_raw, P, b);
  QR_CHECK_ARG(m * (int64_t)b < (1ll << 32), "qrlsh_index_probe_finish: m * b must stay below 2^32");
  QR_CHECK_ARG(sig_dtype == QRLSH_SIG_I32 || sig_dtype == QRLSH_SIG_U16, "qrlsh_index_probe_finish: bad sig_dtype %d",
               sig_dtype);
  QR_CHECK_ARG(off_out, "qrlsh_index_probe_finish: null off_out");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m == 0) {
    QR_MEMSET("qrlsh_index_probe_finish", off_out, 0, sizeof(int64_t), st);
    return QRLSH_OK;
  }
  QR_CHECK_ARG(probe_workspace && idx_out && milli_out && avail_out && workspace && (n_raw == 0 || (sig && probe_sig && raw)),
               "qrlsh_index_probe_finish: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_index_probe_finish", workspace, workspace_bytes, qrlsh_index_finish_workspace_bytes(m, K, n_raw));
  QrCarve c(workspace);
  const FinishWs w = finish_layout(c, m, K, n_raw);
  uint64_t *keys = w.keys, *sums = w.sums;
  int32_t *pidx = w.pidx, *pmilli = w.pmilli;
  if (n_raw > 0) {
    const dim3 grid((unsigned)ceil_div64(n_raw, 256)), block(256);
    if (sig_dtype == QRLSH_SIG_U16)
      QR_LAUNCH("index_score", index_score_kernel<uint16_t>, grid, block, 0, st, static_cast<const uint16_t *>(sig), norm2, n,
                static_cast<const uint16_t *>(probe_sig), probe_norm2, P, b, m, raw, n_raw, first_id, self_ids, keys);
    else
      QR_LAUNCH("index_score", index_score_kernel<int32_t>, grid, block, 0, st, static_cast<const int32_t *>(sig), norm2, n,
                static_cast<const int32_t *>(probe_sig), probe_norm2, P, b, m, raw, n_raw, first_id, self_ids, keys);
  }
  uint64_t *cut = reinterpret_cast<uint64_t *>(off_out);
  QR_LAUNCH("index_select", index_select_kernel, dim3((unsigned)m), dim3(256), 0, st, (const uint64_t *)keys,
            static_cast<const uint64_t *>(probe_workspace), b, K, pidx, pmilli, avail_out, cut);
  qr_scan_u64(cut, m, cut + m, sums, st);
  QR_LAUNCH("index_compact", index_compact_kernel, dim3((unsigned)ceil_div64(m * K, 256)), dim3(256), 0, st,
            (const int32_t *)pidx, (const int32_t *)pmilli, m, K, (const int64_t *)off_out, idx_out, milli_out);
  QR_LAUNCH_CHECK("qrlsh_index_probe_finish");
  return QRLSH_OK;
}

QRLSH_EXPORT int qrlsh_index_probe_finish(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig,
                                          const int64_t *probe_norm2, int32_t sig_dtype, int32_t P, int32_t b, int64_t m,
                                          const void *probe_workspace, const uint64_t *raw, int64_t n_raw, int32_t K,
                                          int64_t *off_out, int32_t *idx_out, int32_t *milli_out, int32_t *avail_out,
                                          void *workspace, size_t workspace_bytes, void *stream) {
  return ix_finish(sig, norm2, n, probe_sig, probe_norm2, sig_dtype, P, b, m, probe_workspace, raw, n_raw, K, -1, nullptr,
                   off_out, idx_out, milli_out, avail_out, workspace, workspace_bytes, stream);
}

// the finish for probe rows that are in the index themselves: row q is indexed query first_id + q and is kept out of
// its own list
QRLSH_EXPORT int qrlsh_index_probe_finish_indexed(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig,
                                                  const int64_t *probe_norm2, int32_t sig_dtype, int32_t P, int32_t b,
                                                  int64_t m, int64_t first_id, const void *probe_workspace,
                                                  const uint64_t *raw, int64_t n_raw, int32_t K, int64_t *off_out,
                                                  int32_t *idx_out, int32_t *milli_out, int32_t *avail_out,
                                                  void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(first_id >= 0 && m >= 0 && first_id + m <= n,
               "qrlsh_index_probe_finish_indexed: rows %lld .. %lld are not among the %lld indexed queries",
               (long long)first_id, (long long)(first_id + m), (long long)n);
  return ix_finish(sig, norm2, n, probe_sig, probe_norm2, sig_dtype, P, b, m, probe_workspace, raw, n_raw, K, first_id,
                   nullptr, off_out, idx_out, milli_out, avail_out, workspace, workspace_bytes, stream);
}

// the finish for probe rows scattered over the index: row q is indexed query self_ids[q] (device uint32 [m]) and is kept
// out of its own list
QRLSH_EXPORT int qrlsh_index_probe_finish_rows(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig,
                                               const int64_t *probe_norm2, int32_t sig_dtype, int32_t P, int32_t b, int64_t m,
                                               const uint32_t *self_ids, const void *probe_workspace, const uint64_t *raw,
                                               int64_t n_raw, int32_t K, int64_t *off_out, int32_t *idx_out,
                                               int32_t *milli_out, int32_t *avail_out, void *workspace,
                                               size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(m >= 0 && (m == 0 || self_ids), "qrlsh_index_probe_finish_rows: null self_ids");
  return ix_finish(sig, norm2, n, probe_sig, probe_norm2, sig_dtype, P, b, m, probe_workspace, raw, n_raw, K, -1, self_ids,
                   off_out, idx_out, milli_out, avail_out, workspace, workspace_bytes, stream);
}

// ---- append: new queries enter a built index ----------------------------------------------------------------------
// The build's order is "top 32 bits of mix64(key), then id ascending" and appended ids (n .. n + m - 1) are larger than
// every indexed id, so the grown index is the STABLE MERGE of the old band and the sorted batch, old records first
// among equal mix bits -- byte for byte what qrlsh_index_build makes of the concatenated [b][n + m] keys.
//   sort:   the batch, exactly as the build sorts it (qrlsh_sort_u64, QRLSH_SORT_MIX | QRLSH_SORT_IOTA, bits 32..64).
//   rank:   one lane per (band, sorted batch record j): p_j = old records of the band whose top-32 mix bits are <= the
//           record's (old directory + a binary search inside the slot); q_j = p_j + j, strictly increasing per band,
//           is the record's output position.
//   merge:  one workgroup per tile of IA_TILE consecutive output positions of one band.  Two binary searches in q
//           give the batch records [j0, j1) that land in the tile.  j0 == j1 (the common case): a copy of the old
//           records shifted by j0.  Otherwise a flag bitmap of the tile in LDS and a scan over its words tell every
//           position how many batch records lie before it in the tile: a flagged position takes batch record
//           j0 + before, any other old record x - j0 - before.  Old reads and all writes are consecutive per lane.
//           The same pass writes the directory at d = qrlsh_index_dir_bits(n + m) bits as index_dir_kernel does:
//           each record compares its top d mix bits with its predecessor's (the lane below; a wave's first lane
//           fetches it, the tile's first record reads one record before the tile).
constexpr int IA_TILE = 4096;          // output positions per merge workgroup
constexpr int IA_WORDS = IA_TILE / 32; // words of its flag bitmap

// q[t][j] = output position of sorted batch record j of band t
__global__ __launch_bounds__(256) void index_rank_kernel(const uint64_t *__restrict__ okeys,
                                                         const uint32_t *__restrict__ odir, int64_t n, int d,
                                                         const uint64_t *__restrict__ skeys, int64_t m,
                                                         uint32_t *__restrict__ q) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t t = blockIdx.y;
  uint32_t p = 0;
  if (n > 0) {
    const uint64_t *bk = okeys + t * n;
    const uint32_t *bd = odir + t * ((1ll << d) + 1);
    const uint64_t h = qr_mix64(skeys[t * m + j]);
    const uint32_t T = (uint32_t)(h >> 32);
    uint32_t L = bd[h >> (64 - d)], R = bd[(h >> (64 - d)) + 1];
    while (L < R) {
      const uint32_t mid = L + (R - L) / 2;
      if (ix_top32(bk[mid]) <= T) L = mid + 1;
      else R = mid;
    }
    p = L;
  }
  q[t * m + j] = p + (uint32_t)j;
}

// the source of tile position k: how many batch records of the tile lie before it, and whether it is one
__device__ static inline bool ia_source(bool mixed, const uint32_t *flags, const uint32_t *wpre, uint32_t k,
                                        uint32_t &before) {
  before = 0;
  if (!mixed) return false;
  const uint32_t f = flags[k >> 5], bit = k & 31u;
  before = wpre[k >> 5] + (uint32_t)__popc(f & ((1u << bit) - 1u));
  return (f >> bit) & 1u;
}

__global__ __launch_bounds__(256) void index_merge_kernel(const uint64_t *__restrict__ okeys,
                                                          const uint32_t *__restrict__ oids, int64_t n,
                                                          const uint64_t *__restrict__ skeys,
                                                          const uint32_t *__restrict__ sids,
                                                          const uint32_t *__restrict__ q, int64_t m, int d,
                                                          uint64_t *__restrict__ keys_out, uint32_t *__restrict__ ids_out,
                                                          uint32_t *__restrict__ dir_out) {
  __shared__ uint32_t flags[IA_WORDS];
  __shared__ uint32_t wpre[IA_WORDS];
  __shared__ uint64_t sc[4];
  const int64_t N = n + m, t = blockIdx.y;
  const int64_t o = (int64_t)blockIdx.x * IA_TILE;
  const int64_t oe = o + IA_TILE < N ? o + IA_TILE : N;
  const uint64_t *ok = okeys + t * n;
  const uint32_t *oi = oids + t * n;
  const uint64_t *sk = skeys + t * m;
  const uint32_t *si = sids + t * m;
  const uint32_t *bq = q + t * m;
  uint64_t *ko = keys_out + t * N;
  uint32_t *io = ids_out + t * N;
  uint32_t *dr = dir_out + t * ((1ll << d) + 1);
  const int lane = lane_id();
  // [j0, j1): the batch records with o <= q < oe (uniform; q is strictly increasing, so j1 <= j0 + oe - o)
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)bq[mid] < o) lo = mid + 1;
    else hi = mid;
  }
  const int64_t j0 = lo;
  hi = j0 + (oe - o) < m ? j0 + (oe - o) : m;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)bq[mid] < oe) lo = mid + 1;
    else hi = mid;
  }
  const int64_t j1 = lo;
  const bool mixed = j1 > j0;
  if (mixed) {
    if (threadIdx.x < IA_WORDS) flags[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
      const uint32_t k = (uint32_t)((int64_t)bq[j] - o);
      if (k < (uint32_t)IA_TILE) atomicOr(&flags[k >> 5], 1u << (k & 31u));
    }
    __syncthreads();
    uint64_t tot;
    const uint64_t c = threadIdx.x < IA_WORDS ? (uint64_t)__popc(flags[threadIdx.x]) : 0;
    const uint64_t pre = block_excl_scan_u64_256(c, sc, &tot);
    if (threadIdx.x < IA_WORDS) wpre[threadIdx.x] = (uint32_t)pre;
    __syncthreads();
  }
  // top d mix bits of the record before the tile (-1 before a band's first record)
  int64_t htile = -1;
  if (o > 0) {
    const bool isnew = j0 > 0 && (int64_t)bq[j0 - 1] == o - 1;
    const uint64_t kp = isnew ? sk[j0 - 1] : (o - 1 - j0 >= 0 && o - 1 - j0 < n ? ok[o - 1 - j0] : 0);
    htile = (int64_t)(qr_mix64(kp) >> (64 - d));
  }
  for (int k0 = 0; k0 < IA_TILE && o + k0 < oe; k0 += 256) {
    const uint32_t k = (uint32_t)k0 + threadIdx.x;
    const int64_t x = o + k;
    const bool live = x < oe;
    uint64_t key = 0;
    uint32_t id = 0;
    if (live) {
      uint32_t before;
      if (ia_source(mixed, flags, wpre, k, before)) {
        const int64_t j = j0 + before;
        if (j < m) {
          key = sk[j];
          id = (uint32_t)n + si[j];
        }
      } else {
        const int64_t i = x - j0 - before;
        if (i >= 0 && i < n) {  // always, for a q the rank kernel wrote
          key = ok[i];
          id = oi[i];
        }
      }
    }
    const int64_t h = (int64_t)(qr_mix64(key) >> (64 - d));
    int64_t hp = __shfl_up(h, 1, WAVE);
    if (lane == 0) {
      if (k == 0) hp = htile;
      else if (live) {
        uint32_t before;
        const bool isnew = ia_source(mixed, flags, wpre, k - 1, before);
        const int64_t i = isnew ? j0 + before : x - 1 - j0 - before;
        const uint64_t kp = i >= 0 && i < (isnew ? m : n) ? (isnew ? sk[i] : ok[i]) : 0;
        hp = (int64_t)(qr_mix64(kp) >> (64 - d));
      }
    }
    if (live) {
      ko[x] = key;
      io[x] = id;
      for (int64_t s = hp + 1; s <= h; ++s) dr[s] = (uint32_t)x;
      if (x == N - 1)
        for (int64_t s = h + 1; s <= (1ll << d); ++s) dr[s] = (uint32_t)N;
    }
  }
}

// workspace: batch keys_tmp u64 [b][m] | batch ids u32 [b][m] | ids_tmp u32 [b][m] | q u32 [b][m] | sort workspace
struct AppendWs {
  uint64_t *ktmp;
  uint32_t *bids, *itmp, *q;
  void *sort_ws;
  size_t sort_bytes;
};
static AppendWs append_layout(QrCarve &c, int64_t m, int32_t b) {
  const size_t bm = (size_t)b * (size_t)m;
  AppendWs w;
  w.ktmp = c.take<uint64_t>(bm);
  w.bids = c.take<uint32_t>(bm);
  w.itmp = c.take<uint32_t>(bm);
  w.q = c.take<uint32_t>(bm);
  w.sort_bytes = qrlsh_sort_workspace_bytes(m, b);
  w.sort_ws = c.take_bytes(w.sort_bytes, 1);
  return w;
}
QRLSH_EXPORT size_t qrlsh_index_append_workspace_bytes(int64_t m, int32_t b) {
  if (m <= 0 || b <= 0) return 0;
  return QR_LAYOUT_BYTES(append_layout, m, b);
}

QRLSH_EXPORT int qrlsh_index_append(const uint64_t *keys, const uint32_t *ids, const uint32_t *dir, int64_t n, int32_t b,
                                    uint64_t *new_keys, int64_t m, uint64_t *keys_out, uint32_t *ids_out,
                                    uint32_t *dir_out, void *workspace, size_t workspace_bytes, void *stream) {
  QR_CHECK_ARG(n >= 0 && m >= 0 && n < (1ll << 32) - 1 && m < (1ll << 32) - 1 && b > 0 && b <= 65535,
               "qrlsh_index_append: bad sizes n=%lld m=%lld b=%d", (long long)n, (long long)m, b);
  QR_CHECK_ARG(n + m < (1ll << 32) - 1, "qrlsh_index_append: n + m = %lld must stay below 2^32 - 1", (long long)(n + m));
  if (m == 0) return QRLSH_OK;  // nothing to add: the outputs are not written
  QR_CHECK_ARG(new_keys && keys_out && ids_out && dir_out && workspace && (n == 0 || (keys && ids && dir)),
               "qrlsh_index_append: null pointer");
  QR_CHECK_WORKSPACE("qrlsh_index_append", workspace, workspace_bytes, qrlsh_index_append_workspace_bytes(m, b));
  hipStream_t st = static_cast<hipStream_t>(stream);
  QrCarve c(workspace);
  const AppendWs w = append_layout(c, m, b);
  uint64_t *ktmp = w.ktmp;
  uint32_t *bids = w.bids, *itmp = w.itmp, *q = w.q;
  const int rc = qrlsh_sort_u64(new_keys, ktmp, bids, itmp, m, b, 32, 64, QRLSH_SORT_MIX | QRLSH_SORT_IOTA, 0, w.sort_ws,
                                w.sort_bytes, stream);
  if (rc < 0) return rc;
  const uint64_t *sk = rc == 1 ? ktmp : new_keys;
  const uint32_t *si = rc == 1 ? itmp : bids;
  QR_LAUNCH("index_rank", index_rank_kernel, dim3((unsigned)ceil_div64(m, 256), (unsigned)b), dim3(256), 0, st, keys, dir,
            n, (int)qrlsh_index_dir_bits(n), sk, m, q);
  QR_LAUNCH("index_merge", index_merge_kernel, dim3((unsigned)ceil_div64(n + m, IA_TILE), (unsigned)b), dim3(256), 0, st,
            keys, ids, n, sk, si, (const uint32_t *)q, m, (int)qrlsh_index_dir_bits(n + m), keys_out, ids_out, dir_out);
  QR_LAUNCH_CHECK("qrlsh_index_append");
  return QRLSH_OK;
}
