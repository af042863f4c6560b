// rankgrid.hip -- qrlsh_evaluate_ranking_grid: qrlsh_evaluate_ranking(candidates = QRLSH_RANK_HELDOUT)'s eight words per
// request and sixteen totals, for every setting of a grid (query-list cut, user-list cut, weight triple), from ONE sweep.
//
// The two sides of a test cell do not depend on the weights and depend on the cuts only through a list prefix, so the
// sweep computes them once per cut (at most 4 + 4 accumulations, identical prefixes shared) and writes one RECORD per
// test cell: column, truth value, one double per query cut, one per user cut.  What is per setting is the blend, the
// rounding and the SELECTION: which k of the request's test cells are listed, and in which order.  Four steps:
//   rank_grid_count_kernel  counts the test cells of every (request, column slice); an exclusive scan of the counts gives
//                           each slice its place in the record arrays, so a request's records lie together in column
//                           order and the arrays follow the number of test cells, never nq x settings;
//   rank_grid_sweep_kernel  rank_sweep_kernel<true>'s geometry (rankeval.hip: the user's row as bytes in LDS, the test
//                           cells of a slice queued in LDS and served 1024 at a time) writes the records;
//   rank_grid_rank_kernel   one workgroup per (request, setting): blends every record (ev_blend, rint), finds the list's
//                           boundary by a radix select over the whole int32 range (no value window, so no fallback),
//                           collects the <= k listed (prediction, column, relevant) keys in LDS in column order (a stable
//                           block scan: ties go to the lowest column) and gives every listed RELEVANT cell its exact
//                           position p = the number of listed keys below its own: gain[p], hits, first hit;
//   rank_grid_finish_kernel / rank_grid_totals_kernel add the lines into per-setting totals through the workspace: no
//                           global atomics on a result, nothing depends on the launch order.
// No list and no (nu, nq) matrix is written per setting.  Everything counted is an integer.
#include "common.h"
#include "evalsides.h"

constexpr int RG_THREADS = 1024;           // sweep
constexpr int RG_AUTO_GROUPS = 4096;       // column slices: about this many sweep workgroups
constexpr int RGC_THREADS = 256;           // count
constexpr int RGK_THREADS = 256;           // rank
constexpr int RGK_MAXK = 1024;             // QRLSH_RECOMMEND_MAX_K: the keys of one list fit 8 KB of LDS
constexpr int RGF_REQUESTS = 64;           // requests per workgroup of the finish kernel
constexpr int RG_LINE = 8, RG_TOTALS = 16;

static int64_t rg_slices(int64_t m, int64_t nq) {
  int64_t S = ceil_div64(RG_AUTO_GROUPS, m > 0 ? m : 1);
  const int64_t most = ceil_div64(nq, RG_THREADS);
  if (S > most) S = most;
  return S < 1 ? 1 : S;
}

// cnt[x * S + s] = the test cells (train == 0 && truth != 0) of request x in column slice s; 0 for a user id outside
// [0, nu) (flag bit 2 of the check kernel).  Scanned in place into the slices' record offsets.
__global__ __launch_bounds__(RGC_THREADS) void rank_grid_count_kernel(const int32_t *__restrict__ train,
                                                                      const int32_t *__restrict__ truth, int64_t nu,
                                                                      int64_t nq, const int32_t *__restrict__ users,
                                                                      int64_t m, int64_t slices,
                                                                      uint64_t *__restrict__ cnt) {
  __shared__ uint32_t wc[RGC_THREADS / WAVE];
  const int64_t s = blockIdx.x / m, x = blockIdx.x - s * m;
  const int t = threadIdx.x;
  const int64_t per = (nq + slices - 1) / slices;
  const int64_t j0 = s * per, j1 = min(nq, j0 + per);
  const int64_t i = users ? (int64_t)users[x] : x;
  uint32_t n = 0;
  if (i >= 0 && i < nu) {  // uniform
    const int32_t *row = train + i * nq;
    const int32_t *trow = truth + i * nq;
    for (int64_t j = j0 + t; j < j1; j += RGC_THREADS) n += (row[j] == 0 && trow[j] != 0) ? 1u : 0u;
  }
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) n += __shfl_xor(n, d, WAVE);
  if ((t & (WAVE - 1)) == 0) wc[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    uint64_t sum = 0;
#pragma unroll
    for (int q = 0; q < RGC_THREADS / WAVE; ++q) sum += wc[q];
    cnt[x * slices + s] = sum;
  }
}

// The sweep.  off[x * S + s] = where the records of (request x, slice s) start, off[m * S] = all records; nothing is
// written when they exceed `cap` (flag bit 4, raised by the rank kernel).  Record r: col[r], tru[r], sides[c][r] for c <
// ncq (query cuts) and sides[ncq + c][r] (user cuts), `cap` records per array.
__global__ __launch_bounds__(RG_THREADS) void rank_grid_sweep_kernel(
    const int32_t *__restrict__ train, const int32_t *__restrict__ truth, int64_t nu, int64_t nq,
    const int64_t *__restrict__ q_off, const int32_t *__restrict__ q_idx, const int32_t *__restrict__ q_milli,
    const int32_t *__restrict__ u_idx, const double *__restrict__ u_val, int ku, const int32_t *__restrict__ q_cuts,
    int ncq, const int32_t *__restrict__ u_cuts, int ncu, int sequential, const int32_t *__restrict__ users, int64_t m,
    int64_t slices, const uint64_t *__restrict__ off, int64_t cap, int32_t *__restrict__ col, int32_t *__restrict__ tru,
    double *__restrict__ sides) {
  __shared__ uint8_t lrow[PR_MAXQ];
  __shared__ int32_t queue_j[EV_QUEUE_SLOTS<RG_THREADS>];
  __shared__ int32_t queue_v[EV_QUEUE_SLOTS<RG_THREADS>];
  __shared__ uint32_t wsum[RG_THREADS / WAVE];
  __shared__ int wide;
  const int64_t s = blockIdx.x / m, x = blockIdx.x - s * m;
  const int64_t per = (nq + slices - 1) / slices;
  const int64_t j0 = s * per, j1 = min(nq, j0 + per);
  const int64_t i = users ? (int64_t)users[x] : x;
  if (i < 0 || i >= nu) return;                    // uniform; flagged (bit 2) by the check kernel; no records
  if (off[m * slices] > (uint64_t)cap) return;     // uniform; flagged (bit 4)
  const uint64_t base = off[x * slices + s];
  if (off[x * slices + s + 1] == base) return;     // uniform: no test cell in this slice (x * S + s + 1 <= m * S)
  const int32_t *row = train + i * nq;
  const int32_t *trow = truth + i * nq;
  bool in_lds = false;
  if (nq <= PR_MAXQ) in_lds = ev_stage_row<RG_THREADS>(row, nq, lrow, &wide);  // uniform
  const int32_t *ui = u_idx + i * ku;
  const double *uv = u_val + i * ku;
  int mu = 0;
  while (mu < ku && ui[mu] >= 0) ++mu;  // uniform: the user's own neighbour list (written out: see the queue below)
  // the cuts (uniform; a negative one is flagged and reads as 0) and the user list's length under each
  int qc[QRLSH_GRID_MAX_CUTS], um[QRLSH_GRID_MAX_CUTS];
#pragma unroll
  for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
    qc[c] = c < ncq ? max(q_cuts[c], 0) : 0;
    um[c] = c < ncu ? min(mu, max(u_cuts[c], 0)) : 0;
  }
  const bool seq = sequential != 0;
  // one test cell: its sides under every cut -> record base + slot (slot = its rank among the slice's test cells)
  // The queue is ev_cell_queue's (evalsides.h), written out with its ring and barriers, and so is the list-length loop
  // above: through both helpers this kernel measured up to 1.7 % slower than before with 16 requests, through the queue
  // helper alone still 1.1 to 1.3 % on thin samples.  As written it compiles to the instructions it had before
  // (profiles/predict_split_parent_vs_branch.json: rank_grid_probe and diagnostic_rank_grid_sweep).
  constexpr int RG_QUEUE = EV_QUEUE_SLOTS<RG_THREADS>;
  const int t = threadIdx.x;
  auto one = [&](uint32_t slot) {
    const int64_t j = queue_j[slot & (RG_QUEUE - 1)];
    const int32_t tv = queue_v[slot & (RG_QUEUE - 1)];
    double qp[QRLSH_GRID_MAX_CUTS] = {0.0, 0.0, 0.0, 0.0}, up[QRLSH_GRID_MAX_CUTS] = {0.0, 0.0, 0.0, 0.0};
    const int64_t lo = q_off[j], n64 = q_off[j + 1] - lo;
    if (n64 >= 0 && n64 <= PRED_MAXK) {  // else flagged (bit 0), never walked: every setting predicts 0
      bool outside = false;
      int last = -1;
#pragma unroll
      for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
        if (c < ncq) {
          const int n = min((int)n64, qc[c]);
          if (c > 0 && n == last) qp[c] = qp[c - 1];  // the list is no longer than either cut: the same prefix
          else
            qp[c] = ev_query_side<true>(
                nq, j, lo, n, q_idx, q_milli, seq, [&](int32_t q) { return in_lds ? (int32_t)lrow[q] : row[q]; }, outside);
          last = n;
        }
      }
#pragma unroll
      for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
        if (c < ncu) {
          if (c > 0 && um[c] == um[c - 1]) up[c] = up[c - 1];  // uniform
          else up[c] = ev_user_side<true>(train, nu, nq, i, j, ui, uv, um[c], seq);
        }
      }
      if (outside) {  // flagged (bit 1): every setting predicts 0
#pragma unroll
        for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) qp[c] = up[c] = 0.0;
      }
    }
    const uint64_t r = base + slot;   // < off[x * S + s + 1] <= cap
    col[r] = (int32_t)j;
    tru[r] = tv;
#pragma unroll
    for (int c = 0; c < QRLSH_GRID_MAX_CUTS; ++c) {
      if (c < ncq) sides[(uint64_t)c * cap + r] = qp[c];
      if (c < ncu) sides[(uint64_t)(ncq + c) * cap + r] = up[c];
    }
  };
  uint32_t head = 0, tail = 0;  // uniform
  for (int64_t b0 = j0; b0 < j1; b0 += RG_THREADS) {
    const int64_t j = b0 + t;
    bool take = false;
    int32_t tv = 0;
    if (j < j1) {
      const int32_t own = in_lds ? (int32_t)lrow[j] : row[j];
      tv = trow[j];
      take = own == 0 && tv != 0;
    }
    uint32_t total;
    const uint32_t pos = block_excl_scan<RG_THREADS>(take ? 1u : 0u, wsum, total);
    if (take) {
      queue_j[(tail + pos) & (RG_QUEUE - 1)] = (int32_t)j;
      queue_v[(tail + pos) & (RG_QUEUE - 1)] = tv;
    }
    tail += total;
    if (tail - head >= (uint32_t)RG_THREADS) {  // uniform
      __syncthreads();
      one(head + t);
      head += RG_THREADS;
    }
    // the next scan's first barrier stands between these reads of the queue and the writes that follow it
  }
  __syncthreads();
  if ((uint32_t)t < tail - head) one(head + t);
}

// The rank: one workgroup per (request, setting), the settings of a request together (its records stay in L2).
// key of a listed cell = (~biased prediction) << 32 | column << 1 | relevant: ascending keys = prediction descending,
// then column ascending; columns are distinct, so are the keys, and the position of a key in the list is the number of
// keys below it.  lines[x][s][8] = listed, hits, known (= listed: every candidate is a test cell), first hit, dcg,
// relevant test cells, test cells, avail; a request with a user id outside [0, nu): zeros and avail -1.
// Workgroup 0 also raises flag bit 3 (a negative gain or cut) and bit 4 (more records than the capacity: every request
// then reads as having none).
__global__ __launch_bounds__(RGK_THREADS) void rank_grid_rank_kernel(
    const int32_t *__restrict__ col, const int32_t *__restrict__ tru, const double *__restrict__ sides, int64_t cap,
    const uint64_t *__restrict__ off, int64_t slices, const int32_t *__restrict__ users, int64_t nu, int64_t m,
    const int32_t *__restrict__ q_cuts, int ncq, const int32_t *__restrict__ u_cuts, int ncu,
    const double *__restrict__ weights, int nw, int k, int32_t relevant, const long long *__restrict__ gain,
    long long *__restrict__ lines, uint32_t *__restrict__ flags) {
  __shared__ unsigned long long keys[RGK_MAXK];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wsum[RGK_THREADS / WAVE];
  __shared__ uint32_t sel[2];
  __shared__ long long red[RGK_THREADS / WAVE][4];
  const int settings = ncq * ncu * nw;
  const int64_t x = blockIdx.x / settings;
  const int s = (int)(blockIdx.x - x * settings);
  const int t = threadIdx.x, lane = t & (WAVE - 1);
  const bool over = off[m * slices] > (uint64_t)cap;  // uniform
  if (blockIdx.x == 0) {
    eg_check_cuts(t, q_cuts, ncq, u_cuts, ncu, flags);
    bool negative = false;
    for (int p = t; p < k; p += RGK_THREADS) negative |= gain[p] < 0;
    if (negative) atomicOr(flags, 8u);
    if (over && t == 0) atomicOr(flags, 16u);
  }
  long long *line = lines + (x * settings + s) * RG_LINE;
  const int64_t i = users ? (int64_t)users[x] : x;
  if (i < 0 || i >= nu) {  // uniform; flagged (bit 2) by the check kernel
    if (t < RG_LINE) line[t] = t == RG_LINE - 1 ? -1 : 0;
    return;
  }
  const int cq = s / (ncu * nw), cu = (s / nw) % ncu, w = s % nw;
  const double qw = weights[3 * w], uw = weights[3 * w + 1], dm = weights[3 * w + 2];
  const uint64_t base = off[x * slices];
  const int64_t n = over ? 0 : (int64_t)(off[(x + 1) * slices] - base);
  const int32_t *rc = col + base, *rt = tru + base;
  const double *sq = sides + (uint64_t)cq * cap + base, *su = sides + (uint64_t)(ncq + cu) * cap + base;
  auto biased = [&](int64_t c) {   // 0: no prediction; else the prediction with its sign bit turned (unsigned order)
    int branch;
    const int32_t p = (int32_t)rint(ev_blend(sq[c], su[c], qw, uw, dm, branch));
    return p == 0 ? 0u : (uint32_t)p ^ 0x80000000u;   // p != 0 -> never 0x80000000, so 0 is free to mean "none"
  };
  // the boundary: the k-th largest of the non-zero predictions, one byte of it per pass (the first pass also counts the
  // candidates and the relevant test cells)
  uint32_t prefix = 0, need = (uint32_t)k, avail = 0, nrel = 0;
  bool all = false;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[t] = 0;
    __syncthreads();
    for (int64_t b0 = 0; b0 < n; b0 += RGK_THREADS) {  // uniform trips: the ballots below need the whole wave
      const int64_t c = b0 + t;
      uint32_t u = 0;
      if (c < n) {
        u = biased(c);
        if (pass == 0) nrel += rt[c] >= relevant ? 1u : 0u;
      }
      const bool on = u != 0 && (pass == 0 || (u >> (shift + 8)) == prefix);
      const uint32_t digit = (u >> shift) & 255u;
      // ratings-sized predictions share their upper bytes: a wave whose lanes all hit one digit adds once
      const unsigned long long act = __ballot(on);
      if (act == 0) continue;  // wave-uniform
      const int lead = __ffsll((long long)act) - 1;
      const uint32_t d0 = (uint32_t)__shfl((int)digit, lead, WAVE);
      if (__ballot(on && digit != d0) == 0) {
        if (lane == lead) atomicAdd(&hist[d0], (uint32_t)__popcll(act));
      } else if (on) {
        atomicAdd(&hist[digit], 1u);
      }
    }
    __syncthreads();
    const uint32_t h = hist[255 - t];   // thread t looks at digit 255 - t: the scan runs from the largest digit down
    uint32_t total;
    const uint32_t above = block_excl_scan<RGK_THREADS>(h, wsum, total);
    if (pass == 0) {
      avail = total;
      if (avail <= (uint32_t)k) {  // uniform: everything is listed
        all = true;
        need = 0;
        break;
      }
    }
    if (above < need && need <= above + h) {  // one thread
      sel[0] = 255u - (uint32_t)t;
      sel[1] = need - above;
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    need = sel[1];
    // hist and sel are rewritten only behind the next pass's barriers
  }
  // listed: above the boundary, or on it and among its first `need` in column order
  const uint32_t listed = min(avail, (uint32_t)k);
  uint32_t gt_base = 0, eq_base = 0;  // uniform
  for (int64_t b0 = 0; b0 < n && gt_base + min(eq_base, need) < listed; b0 += RGK_THREADS) {
    const int64_t c = b0 + t;
    uint32_t u = 0;
    if (c < n) u = biased(c);
    const bool gt = u != 0 && (all || u > prefix), eq = u != 0 && !all && u == prefix;
    uint32_t total;
    const uint32_t pos = block_excl_scan<RGK_THREADS>((gt ? 1u : 0u) | (eq ? 1u << 16 : 0u), wsum, total);
    const uint32_t gb = gt_base + (pos & 0xffffu), eb = eq_base + (pos >> 16);
    if (gt || (eq && eb < need))   // slot = the listed cells in front of it < listed <= RGK_MAXK
      keys[gb + min(eb, need)] = (unsigned long long)(uint32_t)~u << 32 | (unsigned long long)(uint32_t)rc[c] << 1 |
                                 (rt[c] >= relevant ? 1ull : 0ull);
    gt_base += total & 0xffffu;
    eq_base += total >> 16;
  }
  __syncthreads();
  // the score: every listed relevant cell finds its position
  long long dcg = 0, hits = 0, first = 0x7fffffff, rel = nrel;
  for (uint32_t e = t; e < listed; e += RGK_THREADS) {
    const unsigned long long key = keys[e];
    if (key & 1ull) {
      uint32_t p = 0;
      for (uint32_t f = 0; f < listed; ++f) p += keys[f] < key ? 1u : 0u;
      ++hits;
      dcg += gain[p];
      first = min(first, (long long)p + 1);
    }
  }
#pragma unroll
  for (int d = WAVE / 2; d >= 1; d >>= 1) {
    dcg += __shfl_xor(dcg, d, WAVE);
    hits += __shfl_xor(hits, d, WAVE);
    rel += __shfl_xor(rel, d, WAVE);
    first = min(first, __shfl_xor(first, d, WAVE));
  }
  if (lane == 0) {
    red[t >> 6][0] = dcg;
    red[t >> 6][1] = hits;
    red[t >> 6][2] = rel;
    red[t >> 6][3] = first;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int q = 1; q < RGK_THREADS / WAVE; ++q) {
      dcg += red[q][0];
      hits += red[q][1];
      rel += red[q][2];
      first = min(first, red[q][3]);
    }
    line[0] = listed;
    line[1] = hits;
    line[2] = listed;
    line[3] = hits ? first : 0;
    line[4] = dcg;
    line[5] = rel;
    line[6] = n;
    line[7] = avail;
  }
}

// gpart[g][s][16] = the totals' words over the requests of group g (RGF_REQUESTS of them) under setting s: words 0-7 the
// column sums of the lines of the requests served, 8 requests served, 9 with >= 1 relevant test cell, 10 with >= 1 hit,
// 11 the ideal DCG gain_prefix[min(k, relevant test cells)], 12-15 = 0.  Thread = (setting, word).
__global__ __launch_bounds__(1024) void rank_grid_finish_kernel(const long long *__restrict__ lines, int64_t m,
                                                                int settings, int k,
                                                                const long long *__restrict__ gain_prefix,
                                                                long long *__restrict__ gpart) {
  const int64_t x0 = (int64_t)blockIdx.x * RGF_REQUESTS, x1 = min(m, x0 + RGF_REQUESTS);
  for (int e = threadIdx.x; e < settings * RG_TOTALS; e += 1024) {
    const int s = e >> 4, w = e & 15;
    long long sum = 0;
    for (int64_t x = x0; x < x1; ++x) {
      const long long *line = lines + (x * settings + s) * RG_LINE;
      if (line[7] < 0) continue;   // not served: nothing added
      if (w < 8) sum += line[w];
      else if (w == 8) sum += 1;
      else if (w == 9) sum += line[5] > 0 ? 1 : 0;
      else if (w == 10) sum += line[1] > 0 ? 1 : 0;
      else if (w == 11) sum += gain_prefix[line[5] < k ? line[5] : k];
    }
    gpart[(int64_t)blockIdx.x * settings * RG_TOTALS + e] = sum;
  }
}

// totals_out[s][16] = the sum of gpart[.][s][16] (one workgroup); *cells_out = the records of the call
__global__ __launch_bounds__(1024) void rank_grid_totals_kernel(const long long *__restrict__ gpart, int64_t groups,
                                                                int settings, long long *__restrict__ totals_out,
                                                                const uint64_t *__restrict__ all_cells,
                                                                long long *__restrict__ cells_out) {
  for (int e = threadIdx.x; e < settings * RG_TOTALS; e += 1024) {
    long long sum = 0;
    for (int64_t g = 0; g < groups; ++g) sum += gpart[g * settings * RG_TOTALS + e];
    totals_out[e] = sum;
  }
  if (threadIdx.x == 0 && cells_out) *cells_out = (long long)*all_cells;
}

// workspace: [off: m x S + 1 u64][the scan's chunk sums][lines: m x settings x 8 int64][gpart: ceil(m / 64) x settings x
// 16 int64][col: cells int32][tru: cells int32][sides: (ncq + ncu) x cells doubles], every part 16-byte aligned
struct RgWs {
  int64_t S, groups;
  uint64_t *off, *sums;
  long long *lines, *gpart;
  int32_t *col, *tru;
  double *sides;
};

static bool rg_sizes_ok(int64_t m, int64_t nq, int32_t ncq, int32_t ncu, int32_t settings, int64_t cells) {
  return m > 0 && nq >= 0 && ncq >= 1 && ncq <= QRLSH_GRID_MAX_CUTS && ncu >= 1 && ncu <= QRLSH_GRID_MAX_CUTS &&
         settings >= 1 && settings <= QRLSH_GRID_MAX_SETTINGS && cells >= 0 && m <= (1ll << 24);
}
static RgWs rg_layout(QrCarve &c, int64_t m, int64_t nq, int32_t ncq, int32_t ncu, int32_t settings, int64_t cells) {
  RgWs w;
  w.S = rg_slices(m, nq);
  w.groups = ceil_div64(m, RGF_REQUESTS);
  w.off = c.take<uint64_t>((size_t)(m * w.S + 1));
  w.sums = c.take<uint64_t>((size_t)(ceil_div64(m * w.S, SCANL_CHUNK) + 1));
  w.lines = c.take<long long>((size_t)m * settings * RG_LINE);
  w.gpart = c.take<long long>((size_t)w.groups * settings * RG_TOTALS);
  w.col = c.take<int32_t>((size_t)cells);
  w.tru = c.take<int32_t>((size_t)cells);
  w.sides = c.take<double>((size_t)(ncq + ncu) * (size_t)cells);
  return w;
}

QRLSH_EXPORT size_t qrlsh_evaluate_ranking_grid_workspace_bytes(int64_t m, int64_t nq, int32_t ncq, int32_t ncu,
                                                                int32_t settings, int64_t cells) {
  if (!rg_sizes_ok(m, nq, ncq, ncu, settings, cells)) return 0;
  return QR_LAYOUT_BYTES(rg_layout, m, nq, ncq, ncu, settings, cells);
}

QRLSH_EXPORT int qrlsh_evaluate_ranking_grid(const int32_t *train, const int32_t *truth, int64_t nu, int64_t nq,
                                             const int64_t *q_off, const int32_t *q_idx, const int32_t *q_milli,
                                             const int32_t *u_idx, const double *u_val, int32_t ku,
                                             const int32_t *q_cuts, int32_t ncq, const int32_t *u_cuts, int32_t ncu,
                                             const double *weights, int32_t nw, int32_t sum_order, const int32_t *users,
                                             int64_t m, int32_t k, int32_t relevant, const int64_t *gain,
                                             const int64_t *gain_prefix, int64_t cells, int64_t *per_request_out,
                                             int64_t *totals_out, int64_t *cells_out, uint32_t *flags_out,
                                             void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "qrlsh_evaluate_ranking_grid";
  QR_CHECK_ARG(nu >= 0 && nq >= 0 && nq <= 2147483647ll && m >= 0 && ku >= 0 && ku <= PRED_MAXK,
               "%s: bad sizes nu=%lld nq=%lld m=%lld ku=%d (<= %d)", who, (long long)nu, (long long)nq, (long long)m, ku,
               PRED_MAXK);
  QR_CHECK_ARG(k >= 1 && k <= RGK_MAXK, "%s: k=%d outside 1 .. %d", who, k, RGK_MAXK);
  QR_CHECK_ARG(relevant >= 1, "%s: relevant=%d below 1", who, relevant);
  QR_CHECK_ARG(sum_order == QRLSH_SUM_PAIRWISE || sum_order == QRLSH_SUM_SEQUENTIAL, "%s: bad sum_order %d", who,
               sum_order);
  QR_CHECK_ARG(ncq >= 1 && ncq <= QRLSH_GRID_MAX_CUTS && ncu >= 1 && ncu <= QRLSH_GRID_MAX_CUTS && nw >= 1 &&
                   (int64_t)ncq * ncu * nw <= QRLSH_GRID_MAX_SETTINGS,
               "%s: bad grid ncq=%d ncu=%d (1 .. %d each) nw=%d (settings 1 .. %d)", who, ncq, ncu, QRLSH_GRID_MAX_CUTS, nw,
               QRLSH_GRID_MAX_SETTINGS);
  QR_CHECK_ARG(cells >= 0, "%s: cells=%lld below 0", who, (long long)cells);
  QR_CHECK_ARG(users || m == nu, "%s: without a user list m (%lld) must equal nu (%lld)", who, (long long)m,
               (long long)nu);
  QR_CHECK_ARG(flags_out && totals_out && q_cuts && u_cuts && weights,
               "%s: flags_out, totals_out, q_cuts, u_cuts and weights are required", who);
  QR_CHECK_ARG(m == 0 || (gain && gain_prefix), "%s: gain and gain_prefix are required", who);
  QR_CHECK_ARG(m == 0 || nq == 0 || (q_off && (nu == 0 || (train && truth && (ku == 0 || (u_idx && u_val))))),
               "%s: null pointer", who);
  const int settings = ncq * ncu * nw;
  if (m > (1ll << 24) || m * settings > 2147483647ll) {
    qrlsh_set_error("%s: m=%lld above the %lld requests of a call, or m x settings above 2^31 - 1", who, (long long)m,
                    (long long)(1ll << 24));
    return QRLSH_EUNSUPPORTED;
  }
  if (m > 0) {   // (every limit of the size is checked above)
    QR_CHECK_ALIGNED(who, "the workspace", qr_addr(workspace), 16);
    QR_CHECK_WORKSPACE(who, workspace, workspace_bytes,
                       qrlsh_evaluate_ranking_grid_workspace_bytes(m, nq, ncq, ncu, settings, cells));
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  QR_MEMSET(who, flags_out, 0, sizeof(uint32_t), st);
  if (m == 0) QR_MEMSET(who, totals_out, 0, (size_t)settings * RG_TOTALS * sizeof(int64_t), st);
  if (m == 0 && cells_out) QR_MEMSET(who, cells_out, 0, sizeof(int64_t), st);
  if (m == 0) return QRLSH_OK;
  QrCarve c(workspace);
  const RgWs p = rg_layout(c, m, nq, ncq, ncu, settings, cells);
  uint64_t *off = p.off, *sums = p.sums;
  long long *lines = per_request_out ? reinterpret_cast<long long *>(per_request_out) : p.lines;
  long long *gpart = p.gpart;
  int32_t *col = p.col, *tru = p.tru;
  double *sides = p.sides;
  const int64_t S = p.S;
  const dim3 slices_grid((unsigned)(m * S));   // <= 2^24 + 4096
  qr_lists_check("rank_grid_check", q_off, q_idx, nq, users, m, nu, flags_out, st);
  QR_LAUNCH("rank_grid_count", rank_grid_count_kernel, slices_grid, dim3(RGC_THREADS), 0, st, train, truth, nu, nq, users, m,
            S, off);
  qr_scan_u64(off, m * S, off + m * S, sums, st);
  if (nq > 0)
    QR_LAUNCH("rank_grid_sweep", rank_grid_sweep_kernel, slices_grid, dim3(RG_THREADS), 0, st, train, truth, nu, nq, q_off,
              q_idx, q_milli, u_idx, u_val, (int)ku, q_cuts, (int)ncq, u_cuts, (int)ncu,
              (int)(sum_order == QRLSH_SUM_SEQUENTIAL), users, m, S, (const uint64_t *)off, cells, col, tru, sides);
  QR_LAUNCH("rank_grid_rank", rank_grid_rank_kernel, dim3((unsigned)(m * settings)), dim3(RGK_THREADS), 0, st,
            (const int32_t *)col, (const int32_t *)tru, (const double *)sides, cells, (const uint64_t *)off, S, users, nu, m,
            q_cuts, (int)ncq, u_cuts, (int)ncu, weights, (int)nw, (int)k, relevant,
            reinterpret_cast<const long long *>(gain), lines, flags_out);
  QR_LAUNCH("rank_grid_finish", rank_grid_finish_kernel, dim3((unsigned)p.groups), dim3(1024), 0, st,
            (const long long *)lines, m, settings, (int)k, reinterpret_cast<const long long *>(gain_prefix), gpart);
  QR_LAUNCH("rank_grid_totals", rank_grid_totals_kernel, dim3(1), dim3(1024), 0, st, (const long long *)gpart, p.groups,
            settings, reinterpret_cast<long long *>(totals_out), (const uint64_t *)(off + m * S),
            reinterpret_cast<long long *>(cells_out));
  QR_LAUNCH_CHECK(who);
  return QRLSH_OK;
}
