// bucket.hip -- the fast bucket path of the candidate-pair step: hash partition into fixed regions (+ overflow
// pool), the LDS finishes that turn a part into its pairs, and qrlsh_bucket_*.
#include "common.h"

// ==========================================================================================
// Fast bucket path (a2/a3): a T-bit hash PARTITION + an LDS finish, instead of a full sort.
//
//   partition : one or two steps of part_scatter_atomic_kernel on the top T bits of mix64(key)
//               (T = 8 .. 16, chosen by the host so that a part holds ~2-4 K records)
//               -> per band 2^T parts, each in a fixed region of its own, records in any order;
//               what a region cannot hold spills into a pool behind the regions;
//   finish    : one workgroup per (part, band) stages the part's records in LDS, groups equal
//               keys through an LDS hash table and pairs every record with the EARLIER arrivals
//               that have the same FULL key -- exactly the (i < j) pairs of that bucket
//               (lsh.py:47-49); parts beyond one LDS image are worked in blocks.
//
// Every workgroup reserves its output range on a device cursor.  What none of this can hold
// (heavily skewed data) raises the overflow word and the host falls back to the general sort path.
// ==========================================================================================

// One-kernel partition of the bucket path (256 parts): every part owns a fixed region of
// `cap` records, a tile reserves room in each part with one atomicAdd per (tile, part) on the part's
// cursor, and writes its records there through the same LDS staging as sort.hip's keys-only scatter.  No histogram pass, no
// row scan, no bounds search; the order of the records inside a part is whatever the atomics gave
// (the finish does not care).  A part that would exceed `cap` raises the overflow word and its
// records are dropped -- the caller then takes the general path.
// LEVEL2 = false: the input is the band-major key matrix ([batch][n], ids = positions), 256 parts per band.
// LEVEL2 = true : finer partitions (T > 8 bits) take a second step -- the input is the OUTPUT of a first
// step, one batch per (band, coarse part): its in_counts[batch] records sit at batch * in_cap and are
// dealt to nd = 2^(T-c1) fine parts by the next bits of the same hash; ids come with the records.
// OVERFLOW POOL (round 4).  A part's region holds ONE LDS image of the finish (reserved memory ~ 1.7 - 2 x the records
// instead of the 7.6 x of three-image regions), and a part swollen by a popular key -- at 100 M queries over 32768
// table rows the luckiest (row, band) makes one band key common to ~20 000 queries -- spills into a pool shared by all
// parts: a (tile, part) run that does not fit the part's region takes its room from a device bump cursor instead and
// leaves a descriptor {part slot, records, pool position}; the first such run also records how many records the
// region really holds (`fill`: reservations are handed out in cursor order, so the region holds a prefix of them).
// The finish lists such parts like every part beyond its image; bucket_big_gather_kernel then puts each one's records
// (region prefix + its runs) next to each other in the pool, where the block kernel works them.  No pool (keys ==
// nullptr: the coarse step of a two-step partition): an overflowing part raises the flag, as before.
// NARROW RECORDS (round 6).  A record is a 64-bit word and a 16-bit tail, 10 bytes instead of 12.  Where a record sits
// already says `used` top bits of x -- the part number: c1 bits after the first of two steps, T bits after the last
// step -- so those bits of the word carry the id's bits from 16 up instead, and the tail its low 16:
//     word = x's low (64 - used) bits | (id >> 16) << (64 - used),    tail = (uint16_t)id
// After the last step id >> 16 always fits (the path serves nq <= 2^(16+T) only).  After the first of two steps it need
// not (10 M queries: 24-bit ids, 16 + c1 = 22), so that step deals every SLAB of 2^(16+c1) consecutive queries to
// regions of its own -- (band, slab, part) -- and the id bits above 16 + c1 are the slab number, which the second step
// knows from its batch.  A tile of the first step is PS_TILE consecutive queries and PS_TILE divides 2^16: a tile lies
// in one slab, its records share id >> 16, and its runs per (tile, part) are as long as without slabs.
// xbits = 64 - used everywhere below.
__device__ static inline uint64_t rec_x(uint64_t word, int xbits) { return word & ((1ull << xbits) - 1ull); }
__device__ static inline uint64_t rec_word(uint64_t x, uint32_t id_hi, int xbits) {
  return rec_x(x, xbits) | (uint64_t)id_hi << xbits;
}
__device__ static inline uint32_t rec_id(uint64_t word, uint16_t tail, int xbits) {
  return (uint32_t)(word >> xbits) << 16 | tail;
}

struct PartPool {
  uint64_t *keys;               // pool records (the words) ...
  uint16_t *vals;               // ... and their tails
  unsigned long long *cursor;   // records handed out so far
  uint32_t cap;                 // records the pool holds (< 2^32)
  uint4 *runs;                  // {part slot, records, pool position, 0} per spilled run
  unsigned long long *nruns;
  uint32_t runs_max;
  uint32_t *fill;               // per part slot: records that sit in its region (0xFFFFFFFF: all of them)
  uint32_t slot_base;           // part slot of this launch's (batch 0, part 0)
};

#ifndef QR_PS_IPT
#define QR_PS_IPT 16
#endif
constexpr int PS_IPT = QR_PS_IPT;  // records per thread of the atomic partition (8, six workgroups per CU: 3.9 ms against 3.4)
constexpr int PS_TILE = SORT_THREADS * PS_IPT;
static_assert(65536 % PS_TILE == 0, "a tile of the first step lies in one slab and its records share id >> 16");
// workgroups per CU the LDS image (10 B per record + 2.3 KB of counters) allows: 42.3 KB at 16 records per thread --
// three; four would need 4 x 42.3 = 169 KB of the CU's 160
constexpr int PS_WGS = PS_IPT <= 16 ? 3 : 2;
// LEVEL2 = false: batch = band; its tiles go to the regions of (band, slab of the tile) -- nslabs = 1, slab_shift = 63
// for a one-step partition.  LEVEL2 = true: batch = ((band * nslabs + slab) << c1) + coarse part, dealt to the fine
// parts of (band, coarse part) whatever the slab.
template <bool LEVEL2>
__global__ __launch_bounds__(SORT_THREADS, PS_WGS) void part_scatter_atomic_kernel(
    const uint64_t *__restrict__ keys_in, const uint16_t *__restrict__ tails_in, uint64_t *__restrict__ keys_out,
    uint16_t *__restrict__ tails_out, int64_t n_in, int ntiles, int shift, uint32_t dmask,
    uint32_t *__restrict__ cursors, uint32_t cap, uint32_t *__restrict__ overflow, uint64_t ek,
    const uint32_t *__restrict__ in_counts, uint32_t in_cap, int64_t chunk_len, int64_t chunk_stride,
    int64_t band_stride, int c1, int nslabs, int slab_shift, PartPool pool) {
  // What travels through the partition is x = mix64(key), not the key: mix64 is a bijection, so equal x <=> equal
  // keys and the finish can pair on x; the part number of either step is then a shift of the staged word (no
  // second hash in the second step, none at the write-out).  Records of empty bands (key == ek) never pair
  // (lsh.py:47) and are dropped here.
  // The order of the records inside a part is free, so a record's place in its tile's share of a part is the old
  // value of an LDS counter (one returning ds_add per record), not the eight ballots + popcount a stable rank
  // costs: the kernel was VALU-bound on those (2200 vector instructions per wave, 66 % VALU-busy).
  __shared__ uint32_t cnt[RADIX];
  __shared__ uint32_t lsum[SORT_THREADS / WAVE];
  __shared__ uint32_t gdelta[RADIX];
  __shared__ uint8_t gok[RADIX];
  __shared__ uint64_t skey[PS_TILE];
  __shared__ uint16_t sval[PS_TILE];
  const int tile = LEVEL2 ? (int)blockIdx.x : xcd_tile(blockIdx.x, ntiles), batch = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
  const int64_t n = LEVEL2 ? (int64_t)min(in_counts[batch], in_cap) : n_in;
  const int64_t tbase = (int64_t)tile * PS_TILE;
  if (tbase >= n) return;  // LEVEL2: the grid covers a full region, this one holds fewer records (uniform)
  cnt[threadIdx.x] = 0;
  __syncthreads();
  // the batch the records go to, and the id bits from 16 up that the written word carries: the tile's own (first
  // step: ids are positions), or slab number : what the read word carries (second step)
  uint32_t obatch, id_hi;
  if (LEVEL2) {
    const uint32_t bs = (uint32_t)batch >> c1, band = bs / (uint32_t)nslabs, slab = bs - band * (uint32_t)nslabs;
    obatch = band << c1 | ((uint32_t)batch & ((1u << c1) - 1u));
    id_hi = slab << c1;
  } else {
    obatch = (uint32_t)batch * (uint32_t)nslabs + (uint32_t)(tbase >> slab_shift);
    id_hi = (uint32_t)(tbase >> 16) & dmask;
  }
  // first step: band `batch` of the key matrix, either plain ([b][n]: band_stride = n) or in chunks of
  // chunk_len queries chunk_stride words apart (what a band-partitioned all-to-all delivers: [rank][band][nql])
  const size_t boff = LEVEL2 ? (size_t)batch * in_cap : (size_t)batch * (size_t)(band_stride ? band_stride : n);
  const bool chunked = !LEVEL2 && chunk_len > 0 && chunk_len < n;
  const int64_t wbase = tbase + (int64_t)w * (WAVE * PS_IPT);
  const uint32_t nd = dmask + 1u;  // parts per batch
  uint64_t key[PS_IPT];
  uint16_t val[PS_IPT];
  uint32_t dr[PS_IPT];  // part << 16 | place among the tile's records of that part; 0xFFFFFFFF = no record
#pragma unroll
  for (int k = 0; k < PS_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    const size_t at = chunked ? boff + (size_t)(idx / chunk_len) * chunk_stride + (size_t)(idx % chunk_len) : boff + idx;
    key[k] = idx < n ? keys_in[at] : ek;
    val[k] = LEVEL2 ? (idx < n ? tails_in[boff + idx] : (uint16_t)0) : (uint16_t)idx;
  }
#pragma unroll
  for (int k = 0; k < PS_IPT; ++k) {
    const int64_t idx = wbase + (int64_t)k * WAVE + lane;
    const bool valid = idx < n && (LEVEL2 || key[k] != ek);
    if (!LEVEL2) key[k] = qr_mix64(key[k]);
    const uint32_t d = (uint32_t)(key[k] >> shift) & dmask;
    dr[k] = valid ? (d << 16) | atomicAdd(&cnt[d], 1u) : 0xFFFFFFFFu;
  }
  __syncthreads();
  // thread d speaks for part d.  The reservation goes out first and its result is not touched until the
  // tile has been laid out in LDS (which needs local positions only): the atomic's round trip to memory
  // runs beside the scan and the staging.
  const uint32_t tc = cnt[threadIdx.x];
  const uint32_t gb = tc ? atomicAdd(&cursors[(size_t)obatch * nd + threadIdx.x], tc) : 0u;
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
  for (int k = 0; k < PS_IPT; ++k) {
    if (dr[k] != 0xFFFFFFFFu) {
      const uint32_t lp = cnt[dr[k] >> 16] + (dr[k] & 0xFFFFu);
      skey[lp] = key[k];
      sval[lp] = val[k];
    }
  }
  {
    const int d = threadIdx.x;
    uint32_t where = gb + tc <= cap ? 1u : 0u;    // 1: the part's region, 2: the pool, 0: nowhere (overflow flag)
    uint32_t delta = (uint32_t)d * cap + gb - lstart;  // mod 2^32; + the staged position gives the place in the batch
    if (!where) {
      if (pool.keys) {  // the run spills: room from the pool's cursor, a descriptor, the region's fill mark
        const unsigned long long pb =
            __hip_atomic_fetch_add(pool.cursor, (unsigned long long)tc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pb + tc <= (unsigned long long)pool.cap) {
          const unsigned long long ri = __hip_atomic_fetch_add(pool.nruns, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (ri < (unsigned long long)pool.runs_max) {
            const uint32_t slot = pool.slot_base + obatch * nd + (uint32_t)d;
            pool.runs[ri] = make_uint4(slot, tc, (uint32_t)pb, 0u);
            atomicMin(&pool.fill[slot], gb);
            where = 2u;
            delta = (uint32_t)pb - lstart;
          }
        }
      }
      if (!where) atomicOr(overflow, 1u);
    }
    gok[d] = (uint8_t)where;
    gdelta[d] = delta;
  }
  __syncthreads();
  uint32_t nstaged = 0;  // records of the tile that are not of an empty band
#pragma unroll
  for (int k = 0; k < SORT_THREADS / WAVE; ++k) nstaged += lsum[k];
  const size_t obase = (size_t)obatch * nd * cap;
#pragma unroll
  for (int k = 0; k < PS_IPT; ++k) {
    const uint32_t p = k * SORT_THREADS + threadIdx.x;
    if (p < nstaged) {
      const uint64_t x = skey[p];  // (second step: the first step's word -- the digit's bits are x's in both)
      const uint32_t d = (uint32_t)(x >> shift) & dmask;
      const uint32_t where = gok[d];
      const uint64_t word = rec_word(x, LEVEL2 ? id_hi | (uint32_t)(x >> (64 - c1)) : id_hi, shift);
      if (where == 1u) {
        const size_t dst = obase + (uint32_t)(gdelta[d] + p);
        keys_out[dst] = word;
        tails_out[dst] = sval[p];
      } else if (where == 2u) {
        const uint32_t dst = gdelta[d] + p;
        pool.keys[dst] = word;
        pool.vals[dst] = sval[p];
      }
    }
  }
}

#ifndef QR_FIN_THREADS
#define QR_FIN_THREADS 1024
#endif
#ifndef QR_FIN_CAP
#define QR_FIN_CAP 6144
#endif
constexpr int FIN_THREADS = QR_FIN_THREADS;
constexpr int FIN_CAP = QR_FIN_CAP;   // records per part that fit the LDS image
constexpr int FIN_IPT = FIN_CAP / FIN_THREADS;
constexpr int FIN_SMALL_THREADS = 512, FIN_SMALL_CAP = 4096;  // the small-part form of the finish
constexpr int FIN_SMALL_MEAN = 2800;                          // mean records per part up to which it is used

// Finish of one (part, band): an open-addressing hash table in LDS keyed by the x bits of the record's word -- inside a
// part they tell the full 64-bit keys apart -- (ds_cmpst_b64 claims a slot or finds the key present; FIN_FREE, which
// has bits set above the x bits and so equals no key, is the "free slot" marker).  A record's arrival number o in its slot's counter
// says how many records of its bucket came before it, so
//     pairs of the part = sum of o
// and the ids of every bucket are laid out next to each other in LDS (run start = exclusive
// scan of the slot counters, place = o): a record pairs with the o ids in front of it in its
// run, ordered (smaller id, larger id).  No chains, no walks, no key re-compares.
// LDS: table 48 KB + counters 24 KB = 72 KB -> two 1024-thread workgroups per CU (which also
// needs <= 64 VGPRs: __launch_bounds__(1024, 8)).  Arrival order varies from run to run, so the
// pairs of a part come out in varying order -- as a set they are exact, and the next step sorts.
constexpr unsigned long long FIN_FREE = ~0ull;
// (key: the x bits only -- the id bits above them differ between the records of a bucket)
template <int CAP = FIN_CAP> __device__ static inline uint32_t fin_home(uint64_t key) {
  uint32_t h = (uint32_t)key * 0x9E3779B1u;
  h ^= h >> 15;
  h += (uint32_t)(key >> 32) * 0x85EBCA77u;
  h ^= h >> 13;
  h *= 0xC2B2AE3Du;
  return __umulhi(h, (uint32_t)CAP);
}

// The pairs of one record with the `c` ids at run[0 .. c) go to dst[pos .. pos + c).  A short run is written by the
// record's own lane; a long one (a popular key: hundreds to thousands of bucket-mates) by the whole wave, lane t
// writing pair t, t + 64, ... -- consecutive lanes write consecutive words instead of each lane walking thousands
// of words a long stride apart.  Called by every lane of the wave (c = 0 for lanes without a record).
// Threshold, 10 M queries x 32 bands (same box): never cooperative 2.88 ms for the finish, 48 -> 2.56, 12 -> 2.52.
#ifndef QR_FIN_COOP
#define QR_FIN_COOP 16
#endif
constexpr uint32_t FIN_COOP = QR_FIN_COOP;
__device__ static inline void emit_run(uint64_t *__restrict__ dst, uint32_t pos, uint32_t me, const uint32_t *run,
                                       uint32_t run_off, uint32_t c) {
  if (c <= FIN_COOP) {
    for (uint32_t t = 0; t < c; ++t) {
      const uint32_t other = run[run_off + t];
      dst[pos + t] = (uint64_t)min(me, other) << 32 | max(me, other);
    }
  }
  uint64_t big = __ballot(c > FIN_COOP);
  const int lane = threadIdx.x & (WAVE - 1);
  while (big) {  // uniform
    const int L = __ffsll((long long)big) - 1;
    big &= big - 1;
    const uint32_t me_b = __shfl(me, L, WAVE), c_b = __shfl(c, L, WAVE), off_b = __shfl(run_off, L, WAVE),
                   pos_b = __shfl(pos, L, WAVE);
    for (uint32_t t = lane; t < c_b; t += WAVE) {
      const uint32_t other = run[off_b + t];
      dst[pos_b + t] = (uint64_t)min(me_b, other) << 32 | max(me_b, other);
    }
  }
}

// ---- the phases all finishes share; how a record enters the LDS table is each kernel's own ----------------------------

// A part that holds more records than the kernel's LDS image (a popular key with thousands of copies, mostly), in its
// region or spilled into the pool, is left to bucket_finish_big_kernel, which works it in blocks: one thread of the
// workgroup lists its slot, or raises the overflow flag when the list is full.
__device__ static inline void fin_list_part(uint64_t slot, uint64_t *biglist, unsigned long long *nbig, uint32_t big_max,
                                            uint32_t *overflow) {
  const unsigned long long at = __hip_atomic_fetch_add(nbig, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (at < (unsigned long long)big_max) biglist[at] = slot;
  else atomicOr(overflow, 1u);
}

// The workgroup's output range: block exclusive scan of every thread's pair count `mine` (a part emits < 2^32 pairs:
// FIN_CAP^2 / 2), the total to `tot`, and -- if there are pairs -- one atomicAdd of the total on the device cursor by
// thread 0, whose result goes to *gbase (LDS: read it after the next barrier).  Returns the thread's first position in
// the range.  wsum is not in use yet when this runs, so nothing waits in front of the store of the wave totals; the
// one barrier behind it also ends the inserts.
template <int THREADS>
__device__ static inline uint32_t fin_reserve(uint32_t mine, uint32_t *wsum, uint64_t *blk, unsigned long long *gbase,
                                              uint32_t &tot) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid >> 6;
  const uint32_t inc = wave_incl_scan(mine);
  if (lane == WAVE - 1) wsum[w] = inc;
  __syncthreads();  // also: every insert is over
  uint32_t base = 0;
  tot = 0;
#pragma unroll
  for (int i = 0; i < THREADS / WAVE; ++i) {
    const uint32_t x = wsum[i];
    if (i < w) base += x;
    tot += x;
  }
  if (tid == 0 && tot)
    *gbase = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(blk), (unsigned long long)tot, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
  return base + inc - mine;
}

// Run starts: exclusive scan of the slot counters, blocked layout (IPT consecutive slots per thread).  count(s) reads
// slot s's counter, start[s] receives the place of its run's first id; returns the number of records.  Every counter
// is read before the scan's first barrier (which also waits for the readers of wsum) and every start is written after
// its second, so `start` may lie over what `count` reads.
template <int THREADS, int IPT, typename Count>
__device__ static inline uint32_t fin_run_starts(Count count, uint32_t *start, uint32_t *wsum) {
  const uint32_t b0 = threadIdx.x * IPT;
  uint32_t v[IPT], sum = 0;
#pragma unroll
  for (int q = 0; q < IPT; ++q) {
    v[q] = count(b0 + q);
    sum += v[q];
  }
  uint32_t all;
  uint32_t run = block_excl_scan<THREADS>(sum, wsum, all);
#pragma unroll
  for (int q = 0; q < IPT; ++q) {
    start[b0 + q] = run;
    run += v[q];
  }
  return all;
}

// so[j] of a thread's record j: arrival number << 16 | slot (both <= 65535), 0xFFFFFFFF = no record.
// The ids laid out bucket by bucket: record j goes to its slot's run start + its arrival number.
template <int IPT>
__device__ static inline void fin_layout(const uint32_t (&so)[IPT], const uint32_t (&ireg)[IPT], const uint32_t *start,
                                         uint32_t *grp) {
#pragma unroll
  for (int j = 0; j < IPT; ++j)
    if (so[j] != 0xFFFFFFFFu) grp[start[so[j] & 0xFFFFu] + (so[j] >> 16)] = ireg[j];
}

// A thread's records, each paired with the o earlier arrivals in front of it in its run, from dst[pos] on
template <int IPT>
__device__ static inline void fin_emit(uint64_t *__restrict__ dst, uint32_t pos, const uint32_t (&so)[IPT],
                                       const uint32_t (&ireg)[IPT], const uint32_t *start, const uint32_t *grp) {
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const bool rec = so[j] != 0xFFFFFFFFu;
    const uint32_t o = rec ? so[j] >> 16 : 0u;
    emit_run(dst, pos, ireg[j], grp, rec ? start[so[j] & 0xFFFFu] : 0u, o);
    pos += o;
  }
}

// The records of part `bslot` are the first counts[bslot] of its own region of `cap` records.  The workgroup reserves
// its output range with one atomicAdd on a global cursor (blk[0]) and writes only if the range fits `capacity`; the
// cursor ends up holding the exact total either way, so a caller whose guess was too small retries once.
// THREADS / CAP: the workgroup and its LDS image.  1024 / 6144 (72 KB: two workgroups per CU) is the general form; when
// the parts are small (mean <= FIN_SMALL_MEAN records: 10 M queries and beyond), 512 / 4096 (48 KB) puts THREE
// independent chains of phases on a CU instead of two (2.51 -> 2.12 ms at 10 M), and a part between 4096 and 6144
// records joins the ones the big kernel works in blocks.
template <int THREADS = FIN_THREADS, int CAP = FIN_CAP>
__global__ __launch_bounds__(THREADS, THREADS >= 1024 ? 8 : 6) void bucket_finish_kernel(
    const uint64_t *__restrict__ keys, const uint16_t *__restrict__ tails, int nparts, int xbits, uint64_t *__restrict__ blk,
    uint32_t *__restrict__ overflow, uint64_t *__restrict__ out, uint64_t capacity, const uint32_t *__restrict__ counts,
    uint32_t cap, uint64_t *__restrict__ biglist, unsigned long long *__restrict__ nbig, uint32_t big_max,
    uint32_t big_base) {
  constexpr int IPT = CAP / THREADS;
  constexpr uint64_t ek = FIN_FREE;
  static_assert(CAP % THREADS == 0 && CAP <= 65535, "image = whole records per thread, slots fit 16 bits");
  __shared__ unsigned long long gbase;
  __shared__ __attribute__((aligned(16))) unsigned long long tab[CAP];
  __shared__ uint32_t cnt[CAP];
  __shared__ uint32_t wsum[THREADS / WAVE];
  const int part = blockIdx.x, band = blockIdx.y;
  const int tid = threadIdx.x;
  const size_t bslot = (size_t)band * nparts + part;
  const uint32_t m = counts[bslot];
  const size_t first = bslot * cap;
  if (m > (uint32_t)CAP || m > cap) {  // uniform over the workgroup
    if (tid == 0) fin_list_part(big_base + bslot, biglist, nbig, big_max, overflow);
    return;
  }
  if (m == 0) return;
  const uint64_t *k = keys + first;
  const uint16_t *tl = tails + first;
  uint64_t kreg[IPT];
  uint32_t ireg[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const uint32_t i = tid + j * THREADS;
    kreg[j] = i < m ? k[i] : ek;
    ireg[j] = i < m ? tl[i] : 0u;  // coalesced, in flight together with the words
  }
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const uint32_t i = tid + j * THREADS;
    if (i < m) {
      ireg[j] = rec_id(kreg[j], (uint16_t)ireg[j], xbits);
      kreg[j] = rec_x(kreg[j], xbits);
    }
    tab[i] = ek;
    cnt[i] = 0;
  }
  __syncthreads();
  uint32_t so[IPT];  // arrival number << 16 | slot (both < FIN_CAP <= 65535); 0xFFFFFFFF = empty band
  uint32_t mine = 0;
  // first probes of all IPT records go out together (independent LDS atomics in flight), the
  // occasional second and later probes follow per record, then all the counter increments together
  uint32_t slot[IPT];
  unsigned long long seen[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    slot[j] = fin_home<CAP>(kreg[j]);
    seen[j] = kreg[j] != ek
                  ? atomicCAS(&tab[slot[j]], (unsigned long long)ek, (unsigned long long)kreg[j])
                  : (unsigned long long)ek;
  }
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    if (kreg[j] != ek) {
      unsigned long long old = seen[j];
      while (old != ek && old != kreg[j]) {  // FIN_CAP slots for at most FIN_CAP records: a free one always turns up
        slot[j] = slot[j] + 1 == (uint32_t)CAP ? 0u : slot[j] + 1;
        old = atomicCAS(&tab[slot[j]], (unsigned long long)ek, (unsigned long long)kreg[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    so[j] = 0xFFFFFFFFu;
    if (kreg[j] != ek) {
      const uint32_t o = atomicAdd(&cnt[slot[j]], 1u);
      so[j] = o << 16 | slot[j];
      mine += o;
    }
  }
  uint32_t tot;
  const uint32_t pos0 = fin_reserve<THREADS>(mine, wsum, blk, &gbase, tot);
  if (tot == 0) return;  // uniform
  fin_run_starts<THREADS, IPT>([&](uint32_t sl) { return cnt[sl]; }, cnt, wsum);
  __syncthreads();
  uint32_t *grp = reinterpret_cast<uint32_t *>(tab);  // the table is dead: ids, bucket by bucket
  fin_layout(so, ireg, cnt, grp);
  __syncthreads();
  const uint64_t obase = (uint64_t)gbase;
  if (obase + tot > capacity) return;  // uniform: counted, not written
  fin_emit(out + obase, pos0, so, ireg, cnt, grp);
}

// The small-part finish with the arrival counters INSIDE the table words (round 4; partitions of 12 bits and more: 10 M
// queries and up).  Inside a part the x bits of a word (64 - T <= 52 of them) tell keys apart, so a slot holds them
// in its low 52 bits, and the 12 bits above hold the number of records that found it: a slot is
// claimed with one CAS (0 -> key52 | 1 << 52: arrival number 0), joined with one returning 64-bit add of 1 << 52 (the old
// count is the arrival number).  No counter array: the image is 32 KB instead of 48 -- FOUR workgroups per CU instead of
// three (the kernel is a chain of barrier-separated phases; what hides one workgroup's latency is another workgroup).
// After the inserts the table is read once (counts -> run starts) and its space re-used: run starts in the lower half,
// the ids laid out by bucket in the upper half.  Parts of more than 4095 records (the 12-bit count) go to the block
// kernel like every part beyond the image.
constexpr int FIN_PK_THREADS = 512, FIN_PK_CAP = 4096, FIN_PK_MAX = 4095;
__global__ __launch_bounds__(FIN_PK_THREADS, 8) void bucket_finish_packed_kernel(
    const uint64_t *__restrict__ keys, const uint16_t *__restrict__ tails, int nparts, int xbits, uint64_t *__restrict__ blk,
    uint32_t *__restrict__ overflow, uint64_t *__restrict__ out, uint64_t capacity, const uint32_t *__restrict__ counts,
    uint32_t cap, uint64_t *__restrict__ biglist, unsigned long long *__restrict__ nbig, uint32_t big_max,
    uint32_t big_base) {
  constexpr int THREADS = FIN_PK_THREADS, CAP = FIN_PK_CAP, IPT = CAP / THREADS;
  constexpr unsigned long long KMASK = (1ull << 52) - 1ull, ONE = 1ull << 52;  // (xbits <= 52: the host's rule)
  __shared__ unsigned long long gbase;
  __shared__ __attribute__((aligned(16))) unsigned long long tab[CAP];
  __shared__ uint32_t wsum[THREADS / WAVE];
  const int part = blockIdx.x, band = blockIdx.y;
  const int tid = threadIdx.x;
  const size_t bslot = (size_t)band * nparts + part;
  const uint32_t m = counts[bslot];
  if (m > (uint32_t)FIN_PK_MAX) {  // uniform
    if (tid == 0) fin_list_part(big_base + bslot, biglist, nbig, big_max, overflow);
    return;
  }
  if (m == 0) return;
  const size_t first = bslot * cap;
  const uint64_t *k = keys + first;
  const uint16_t *tl = tails + first;
  uint64_t kreg[IPT];
  uint32_t ireg[IPT];
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    const uint32_t i = tid + j * THREADS;
    kreg[j] = i < m ? k[i] : 0ull;
    ireg[j] = i < m ? tl[i] : 0u;
  }
#pragma unroll
  for (int j = 0; j < IPT; ++j) tab[tid + j * THREADS] = 0ull;
  __syncthreads();
  uint32_t so[IPT];  // arrival number << 16 | slot; 0xFFFFFFFF = no record
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < IPT; ++j) {
    so[j] = 0xFFFFFFFFu;
    if (tid + j * THREADS < (int)m) {
      const unsigned long long k52 = rec_x(kreg[j], xbits);
      ireg[j] = rec_id(kreg[j], (uint16_t)ireg[j], xbits);  // (the tail was waiting there)
      uint32_t slot = fin_home<CAP>(k52);
      uint32_t o;
      for (;;) {  // at most 4095 records for 4096 slots: a free one always turns up
        const unsigned long long old = atomicCAS(&tab[slot], 0ull, k52 | ONE);
        if (old == 0ull) {
          o = 0;
          break;
        }
        if ((old & KMASK) == k52) {
          o = (uint32_t)(atomicAdd(&tab[slot], ONE) >> 52);
          break;
        }
        slot = slot + 1 == (uint32_t)CAP ? 0u : slot + 1;
      }
      so[j] = o << 16 | slot;
      mine += o;
    }
  }
  uint32_t tot;
  const uint32_t pos0 = fin_reserve<THREADS>(mine, wsum, blk, &gbase, tot);
  if (tot == 0) return;  // uniform
  uint32_t *rs = reinterpret_cast<uint32_t *>(tab);        // run starts: lower half of the table's space ...
  uint32_t *grp = rs + CAP;                                // ... ids by bucket: upper half
  fin_run_starts<THREADS, IPT>([&](uint32_t sl) { return (uint32_t)(tab[sl] >> 52); }, rs, wsum);
  __syncthreads();
  fin_layout(so, ireg, rs, grp);
  __syncthreads();
  const uint64_t obase = (uint64_t)gbase;
  if (obase + tot > capacity) return;  // uniform: counted, not written
  fin_emit(out + obase, pos0, so, ireg, rs, grp);
}

// Parts the kernel above listed (more records than its LDS image): worked in BLOCKS of
// FIN_CAP records by workgroups that walk the device-side list (fixed grid; nothing is read back to size the
// launch).  Block bi is finished exactly like a small part (hash table on the word's x bits, arrival numbers, bucket
// runs laid out in LDS -> its own pairs); then every EARLIER block's records are streamed past bi's table: a
// record whose word is in the table pairs with every id of that bucket's run.  Together: every pair of equal words
// of the part, once -- a key with any number of copies up to FIN_BIG_BLOCKS images is no special case any more.
// Output ranges are reserved on the same device cursor as the small parts'.
constexpr int FIN_BIG_GRID = 256;
constexpr int FIN_BIG_BLOCKS = 16;        // blocks of FIN_CAP records a listed part may hold (98 304); beyond: overflow flag
constexpr uint32_t FIN_BIG_LIST = 4096;   // listed parts per band group and call; beyond: overflow flag (general path)
constexpr int FIN_BIG_SLICES = 8;         // workgroups that share a block pair's pairs (a power of two)
// own-pair ranks of a block: runs up to here are walked by a lane per record; longer ones are sorted in LDS by the
// workgroup (~log2(c)^2 / 2 barrier steps against c^2 / 64 wave-wide LDS reads: by that count the two meet near
// 256 -- 36 steps of ~250 cycles against ~8 000 cycles of reads; the flagship has one run of ~1 700, where the sort wins 5x)
constexpr int FIN_RANK_SORT = 256;
constexpr uint32_t POOL_RUNS = 1u << 20;  // spilled-run descriptors per call; beyond: overflow flag

// where the records of a listed part sit: `pool` = 0: in the part buffers at `where` (its own region), 1: in the
// pool at `where` (gathered there by the kernel below); m = 0: nothing to do (the overflow flag is up)
struct BigDesc {
  uint64_t where;
  uint32_t m, pool;
};

// One workgroup per listed part: a part that spilled (fill mark set) gets m records of room at the pool's cursor and
// its records -- the prefix its region holds and every run of the descriptor list that names it -- are copied there,
// next to each other in any order (the finish does not care); a part that fits its region is described in place.
// Region and pool records have the same form (word, tail): they are copied as they are.
__global__ __launch_bounds__(256) void bucket_big_gather_kernel(const uint64_t *__restrict__ biglist,
                                                                const unsigned long long *__restrict__ nbig, uint32_t big_max,
                                                                BigDesc *__restrict__ desc, const uint64_t *__restrict__ part_keys,
                                                                const uint16_t *__restrict__ part_ids,
                                                                const uint32_t *__restrict__ counts, uint32_t cap, PartPool pool,
                                                                uint32_t max_records, uint32_t *__restrict__ overflow) {
  __shared__ unsigned long long base_s;
  __shared__ uint32_t match[256];
  __shared__ uint32_t nmatch;
  const int tid = threadIdx.x;
  unsigned long long nb = *nbig;
  if (nb > big_max) nb = big_max;
  for (unsigned long long e = blockIdx.x; e < nb; e += gridDim.x) {
    const uint32_t slot = (uint32_t)biglist[e];
    const uint32_t m = counts[slot];
    const uint32_t f = pool.fill ? pool.fill[slot] : 0xFFFFFFFFu;
    if (m > max_records || (f == 0xFFFFFFFFu && m > cap)) {  // (uniform) too large / records were dropped
      if (tid == 0) {
        atomicOr(overflow, 1u);
        desc[e] = BigDesc{0ull, 0u, 0u};
      }
      continue;
    }
    if (f == 0xFFFFFFFFu) {  // all in its region
      if (tid == 0) desc[e] = BigDesc{(uint64_t)slot * cap, m, 0u};
      continue;
    }
    __syncthreads();  // (the previous part's base_s has been read by everyone)
    if (tid == 0)
      base_s = __hip_atomic_fetch_add(pool.cursor, (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const unsigned long long base = base_s;
    if (base + m > (unsigned long long)pool.cap) {  // uniform
      if (tid == 0) {
        atomicOr(overflow, 1u);
        desc[e] = BigDesc{0ull, 0u, 0u};
      }
      continue;
    }
    for (uint32_t i = tid; i < f; i += blockDim.x) {
      pool.keys[base + i] = part_keys[(size_t)slot * cap + i];
      pool.vals[base + i] = part_ids[(size_t)slot * cap + i];
    }
    uint32_t at = f;
    unsigned long long nr = *pool.nruns;
    if (nr > pool.runs_max) nr = pool.runs_max;
    for (unsigned long long r0 = 0; r0 < nr; r0 += blockDim.x) {
      __syncthreads();
      if (tid == 0) nmatch = 0;
      __syncthreads();
      const unsigned long long r = r0 + tid;
      if (r < nr && pool.runs[r].x == slot) match[atomicAdd(&nmatch, 1u)] = (uint32_t)r;
      __syncthreads();
      const uint32_t nm = nmatch;
      for (uint32_t q = 0; q < nm; ++q) {
        const uint4 run = pool.runs[match[q]];
        if (at + run.y <= m)
          for (uint32_t i = tid; i < run.y; i += blockDim.x) {
            pool.keys[base + at + i] = pool.keys[(size_t)run.z + i];
            pool.vals[base + at + i] = pool.vals[(size_t)run.z + i];
          }
        at += run.y;
      }
    }
    if (tid == 0) {
      if (at != m) atomicOr(overflow, 1u);  // (cannot happen: every record of the part is in its region or in a run)
      desc[e] = BigDesc{(uint64_t)base, at == m ? m : 0u, 1u};
    }
  }
}

__global__ __launch_bounds__(FIN_THREADS) void bucket_finish_big_kernel(
    const uint64_t *__restrict__ keys, const uint16_t *__restrict__ ids, const uint64_t *pool_keys, const uint16_t *pool_ids,
    int xbits, const BigDesc *__restrict__ desc, const unsigned long long *__restrict__ nbig, uint32_t big_max,
    uint64_t *__restrict__ blk, uint64_t *__restrict__ out, uint64_t capacity) {
  __shared__ unsigned long long gbase;
  __shared__ __attribute__((aligned(16))) unsigned long long tab[FIN_CAP];
  __shared__ uint32_t cnt[FIN_CAP + 1];
  __shared__ uint32_t grp[FIN_CAP];
  __shared__ uint32_t srt[FIN_CAP];   // the runs in id order (own pairs of a block)
  __shared__ uint32_t wsum[FIN_THREADS / WAVE];
  __shared__ uint32_t lrun[FIN_CAP / (FIN_RANK_SORT + 1) + 1], nlrun;   // slots of the runs longer than FIN_RANK_SORT
  const int tid = threadIdx.x;
  constexpr uint64_t ek = FIN_FREE;
  unsigned long long nb = *nbig;
  if (nb > big_max) nb = big_max;
  // work items: (listed part, block bi, block bj <= bi, slice sl) -- the table of bi is built, then an eighth of bi's
  // own pairs (bj = bi) or of the pairs of bj's records with it is written; a part's items run on different
  // workgroups, so that a key with thousands of copies (1.4 M pairs for 1 700 copies: 0.35 ms when one workgroup
  // writes them all) is the work of eight.  Every workgroup builds the table itself and the arrival numbers differ
  // from build to build, so a slice is defined on something the builds share: bi's own pairs go by the RANK of a
  // record's query id among its bucket-mates (the runs are sorted by id; a record pairs with the mates of smaller
  // id, and belongs to slice rank mod 8), bj's records by their position in bj (mod 8).
  constexpr int COMBOS = FIN_BIG_BLOCKS * (FIN_BIG_BLOCKS + 1) / 2;
  static_assert(FIN_THREADS % FIN_BIG_SLICES == 0, "a thread's records share their position mod the slice count");
  for (unsigned long long item = blockIdx.x; item < nb * COMBOS * FIN_BIG_SLICES; item += gridDim.x) {
    const uint32_t sl = (uint32_t)(item % FIN_BIG_SLICES);
    const unsigned long long e = item / ((unsigned long long)COMBOS * FIN_BIG_SLICES);
    int combo = (int)((item / FIN_BIG_SLICES) % COMBOS);
    uint32_t bi = 0;
    while (combo > (int)bi) {  // combos in the order (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) ...
      combo -= (int)bi + 1;
      ++bi;
    }
    const uint32_t bj_only = (uint32_t)combo;
    const BigDesc de = desc[e];
    const uint32_t m = de.m;
    const uint64_t *k = (de.pool ? pool_keys : keys) + de.where;
    const uint16_t *id = (de.pool ? pool_ids : ids) + de.where;
    const uint32_t nblk = (m + FIN_CAP - 1) / FIN_CAP;
    if (bi >= nblk) continue;  // uniform
    {
      const uint32_t lo = bi * FIN_CAP, mb = min((uint32_t)FIN_CAP, m - lo);
      uint64_t kreg[FIN_IPT];
      uint32_t ireg[FIN_IPT], so[FIN_IPT];
      __syncthreads();  // the previous block / part is done with the arrays
#pragma unroll
      for (int j = 0; j < FIN_IPT; ++j) {
        const uint32_t i = tid + j * FIN_THREADS;
        kreg[j] = ek;
        ireg[j] = 0u;
        if (i < mb) {
          const uint64_t word = k[lo + i];
          kreg[j] = rec_x(word, xbits);
          ireg[j] = rec_id(word, id[lo + i], xbits);
        }
        tab[i] = ek;
        cnt[i] = 0;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < FIN_IPT; ++j) {
        so[j] = 0xFFFFFFFFu;
        if (kreg[j] != ek) {
          uint32_t slot = fin_home(kreg[j]);
          for (;;) {  // at most FIN_CAP records for FIN_CAP slots: a free one always turns up
            const unsigned long long old = atomicCAS(&tab[slot], (unsigned long long)ek, (unsigned long long)kreg[j]);
            if (old == ek || old == kreg[j]) break;
            slot = slot + 1 == (uint32_t)FIN_CAP ? 0u : slot + 1;
          }
          const uint32_t o = atomicAdd(&cnt[slot], 1u);
          so[j] = o << 16 | slot;
        }
      }
      __syncthreads();  // every insert is over
      {
        // cnt[FIN_CAP] = the block's record count: a run's length is cnt[slot + 1] - cnt[slot] for every slot
        const uint32_t all = fin_run_starts<FIN_THREADS, FIN_IPT>([&](uint32_t s) { return cnt[s]; }, cnt, wsum);
        if (tid == 0) cnt[FIN_CAP] = all;
      }
      __syncthreads();
      fin_layout(so, ireg, cnt, grp);
      __syncthreads();  // the runs are laid out (in this build's arrival order)
      if (bj_only == bi) {
        // this block's own pairs.  Rank of every record's id among its run (ids are distinct inside a bucket), the runs
        // re-laid in id order, then a record of rank r pairs with the r mates in front of it -- if r mod 8 is this slice
        // A run longer than FIN_RANK_SORT (the key shared by ~1 700 queries) is first sorted by the whole workgroup,
        // straight into its place in srt, and a record's rank is its id's position there: walking such a run once per
        // record was 1 700^2 LDS reads in every one of the eight slice workgroups, 0.2 of this kernel's 0.3 ms.
        if (tid == 0) nlrun = 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < FIN_IPT; ++q) {
          const uint32_t slot = tid * FIN_IPT + q;
          if (cnt[slot + 1] - cnt[slot] > (uint32_t)FIN_RANK_SORT) lrun[atomicAdd(&nlrun, 1u)] = slot;
        }
        __syncthreads();
        const uint32_t nl = nlrun;
        for (uint32_t r = 0; r < nl; ++r) {  // (uniform; the list's order differs from build to build, the sorted runs do not)
          const uint32_t s0 = cnt[lrun[r]], c = cnt[lrun[r] + 1] - s0;
          for (uint32_t i = tid; i < c; i += FIN_THREADS) srt[s0 + i] = grp[s0 + i];
          uint32_t nn = 2;
          while (nn < c) nn <<= 1;
          // bitonic network on nn >= c places, every exchange leaving the smaller id at the lower place (a merge opens
          // with the mirrored partner): the places from c on stand for +infinity, never move, and are never touched
          for (uint32_t k = 2; k <= nn; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
              __syncthreads();
              for (uint32_t t = tid; t < (nn >> 1); t += FIN_THREADS) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // bit j clear
                const uint32_t l = j == (k >> 1) ? i ^ (k - 1) : i | j;
                if (l < c) {
                  const uint32_t a = srt[s0 + i], b = srt[s0 + l];
                  if (a > b) {
                    srt[s0 + i] = b;
                    srt[s0 + l] = a;
                  }
                }
              }
            }
        }
        __syncthreads();
        uint32_t rk[FIN_IPT];
#pragma unroll
        for (int j = 0; j < FIN_IPT; ++j) {
          rk[j] = 0;
          if (so[j] != 0xFFFFFFFFu) {
            const uint32_t sl0 = so[j] & 0xFFFFu, s0 = cnt[sl0], c = cnt[sl0 + 1] - s0, me = ireg[j];
            uint32_t r = 0;
            if (c > (uint32_t)FIN_RANK_SORT) {
              uint32_t hi = c;   // first place of the sorted run whose id is >= me: the ids in front are the smaller ones
              while (r < hi) {
                const uint32_t mid = (r + hi) >> 1;
                if (srt[s0 + mid] < me) r = mid + 1;
                else hi = mid;
              }
            } else {
              // (a lane per record: the copies of a key fill whole waves, which then walk the run in step --
              // counting a run with the whole wave, one record after the other, was 2.5x slower)
              for (uint32_t u = 0; u < c; ++u) r += grp[s0 + u] < me;
            }
            rk[j] = r;
          }
        }
        __syncthreads();  // every rank is known: the runs may move
#pragma unroll
        for (int j = 0; j < FIN_IPT; ++j)
          if (so[j] != 0xFFFFFFFFu) srt[cnt[so[j] & 0xFFFFu] + rk[j]] = ireg[j];
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < FIN_IPT; ++j) {
          if (so[j] == 0xFFFFFFFFu || (rk[j] & (FIN_BIG_SLICES - 1)) != sl) rk[j] = 0;  // not this slice's: no pairs
          mine += rk[j];
        }
        uint32_t tot;
        const uint32_t pos0 = block_excl_scan<FIN_THREADS>(mine, wsum, tot);  // (its barriers also end the re-layout)
        if (tid == 0 && tot)
          gbase = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(blk), (unsigned long long)tot,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tot && gbase + tot <= capacity) {  // uniform; counted either way
          uint64_t *dst = out + gbase;
          uint32_t pos = pos0;
#pragma unroll
          for (int j = 0; j < FIN_IPT; ++j) {
            emit_run(dst, pos, ireg[j], srt, so[j] != 0xFFFFFFFFu ? cnt[so[j] & 0xFFFFu] : 0u, rk[j]);
            pos += rk[j];
          }
        }
      }
      // the records of an earlier block against this block's table
      if (bj_only < bi) {
        const uint32_t bj = bj_only;
        const uint32_t lo2 = bj * FIN_CAP;  // earlier blocks are full
        uint32_t hit[FIN_IPT];              // slot of the record's word in the table, 0xFFFFFFFF = absent
        uint32_t mine2 = 0;
#pragma unroll
        for (int j = 0; j < FIN_IPT; ++j) {
          const uint32_t i = tid + j * FIN_THREADS;
          const uint64_t word = k[lo2 + i], x = rec_x(word, xbits);
          ireg[j] = rec_id(word, id[lo2 + i], xbits);
          uint32_t slot = fin_home(x), found = 0xFFFFFFFFu;
          const bool my_slice = (uint32_t)(tid & (FIN_BIG_SLICES - 1)) == sl;
          for (int step = 0; my_slice && step < FIN_CAP; ++step) {  // (bounded: a full table has no free slot to stop at)
            const unsigned long long tv = tab[slot];
            if (tv == x) {
              found = slot;
              break;
            }
            if (tv == ek) break;
            slot = slot + 1 == (uint32_t)FIN_CAP ? 0u : slot + 1;
          }
          if ((uint32_t)(tid & (FIN_BIG_SLICES - 1)) != sl) found = 0xFFFFFFFFu;  // another slice's record of bj
          hit[j] = found;
          if (found != 0xFFFFFFFFu) mine2 += cnt[found + 1] - cnt[found];
        }
        uint32_t tot2;
        const uint32_t p0 = block_excl_scan<FIN_THREADS>(mine2, wsum, tot2);
        if (tid == 0 && tot2)
          gbase = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(blk), (unsigned long long)tot2,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (tot2 && gbase + tot2 <= capacity) {  // uniform
          uint64_t *dst = out + gbase;
          uint32_t pos = p0;
#pragma unroll
          for (int j = 0; j < FIN_IPT; ++j) {
            const bool h = hit[j] != 0xFFFFFFFFu;
            const uint32_t s0 = h ? cnt[hit[j]] : 0u, c = h ? cnt[hit[j] + 1] - s0 : 0u;
            emit_run(dst, pos, ireg[j], grp, s0, c);
            pos += c;
          }
        }
        __syncthreads();  // gbase is rewritten by the next reservation
      }
    }
  }
}

// records a listed part may hold (qrlsh_set_big_part_limit; default and maximum: FIN_BIG_BLOCKS images)
static uint32_t g_big_limit = (uint32_t)FIN_BIG_BLOCKS * FIN_CAP;
QRLSH_EXPORT int64_t qrlsh_set_big_part_limit(int64_t records) {
  const int64_t max = (int64_t)FIN_BIG_BLOCKS * FIN_CAP, old = g_big_limit;
  g_big_limit = (uint32_t)(records <= 0 || records > max ? max : records);
  return old;
}

// Slabs of the first step of a two-step partition (narrow records, above): 2^(16+c1) consecutive queries each
static int coarse_bits(int T);
static int slab_bits(int T) { return 16 + coarse_bits(T); }
static int n_slabs(int64_t nq, int T) { return T > 8 ? (int)((nq + (1ll << slab_bits(T)) - 1) >> slab_bits(T)) : 1; }

// workspace: [fill: b << T u32]
//            [step-1 cursors: b x slabs << c1 u32 (two-step partitions only)][step-2 cursors = records per part: b << T u32]
//            [big parts: one counter per band group][pool cursor, run count: 2 u64][runs: POOL_RUNS x 16 B]
//            [the big parts' lists: b << T u64 in all][desc: 2 x FIN_BIG_LIST x 16 B]
// Every area starts on a multiple of 16 bytes.
constexpr int EMIT_MAX_GROUPS = 2;  // band groups of one qrlsh_bucket_pairs_emit call
struct BucketWs {
  uint32_t *fill;
  uint32_t *cur1, *counts;  // (a one-step partition, T = 8, has one set of cursors: cur1 == counts)
  unsigned long long *nbig, *poolctl;
  uint4 *runs;
  uint64_t *biglist;
  BigDesc *desc;
};
static BucketWs bucket_layout(QrCarve &c, int64_t nq, int32_t b, int32_t T) {
  BucketWs w;
  const size_t slots = (size_t)b << T;
  w.fill = c.take<uint32_t>(slots);
  w.cur1 = c.take<uint32_t>(T > 8 ? ((size_t)b * n_slabs(nq, T)) << coarse_bits(T) : 0);
  w.counts = c.take<uint32_t>(slots);
  w.nbig = c.take<unsigned long long>(EMIT_MAX_GROUPS);
  w.poolctl = c.take<unsigned long long>(2);
  w.runs = c.take<uint4>((size_t)POOL_RUNS);
  w.biglist = c.take<uint64_t>(slots);
  w.desc = c.take<BigDesc>((size_t)EMIT_MAX_GROUPS * FIN_BIG_LIST);
  return w;
}
static_assert(sizeof(BigDesc) == 16, "the descriptors end the workspace on a multiple of 16 bytes");

QRLSH_EXPORT size_t qrlsh_bucket_workspace_bytes(int64_t nq, int32_t b, int32_t part_bits) {
  if (nq <= 0 || b <= 0 || part_bits < 8 || part_bits > 16) return 64;
  return QR_LAYOUT_BYTES(bucket_layout, nq, b, part_bits);
}

static int bucket_check(const char *name, const uint64_t *keys, uint64_t *part_keys, uint32_t *part_ids,
                        uint64_t *tmp_keys, uint32_t *tmp_ids, int64_t nq, int32_t b, int32_t r, int32_t part_bits,
                        void *workspace, size_t workspace_bytes, uint64_t *total_overflow_out, hipStream_t st) {
  QR_CHECK_ARG(nq >= 0 && b > 0 && b <= 65535 && r > 0, "%s: bad sizes nq=%lld b=%d r=%d", name, (long long)nq, b, r);
  QR_CHECK_ARG(part_bits >= 8 && part_bits <= 16, "%s: part_bits=%d not in [8,16]", name, part_bits);
  QR_CHECK_ARG(nq < (1ll << 32), "%s: nq too large", name);
  QR_CHECK_ARG(total_overflow_out && workspace, "%s: null pointer", name);
  QR_MEMSET(name, total_overflow_out, 0, 2 * sizeof(uint64_t), st);
  if (nq == 0) return QRLSH_OK;
  QR_CHECK_ARG(keys && part_keys && part_ids, "%s: null pointer", name);
  QR_CHECK_ARG(part_bits == 8 || (tmp_keys && tmp_ids), "%s: part_bits > 8 needs tmp buffers", name);
  QR_CHECK_WORKSPACE(name, workspace, workspace_bytes, qrlsh_bucket_workspace_bytes(nq, b, part_bits));
  return QRLSH_OK;
}

// records every part's region holds in a one-step partition (256 parts): the LDS image of the
// finish for full-size inputs, mean + 50 % + 512 for small ones
static uint32_t part_region(int64_t nq) {
  const int64_t c = ((nq / RADIX) * 3 / 2 + 512 + 63) / 64 * 64;
  // full-size inputs: ONE image of the finish; a part swollen by a popular key spills into the overflow pool and goes
  // to bucket_finish_big_kernel instead of sending the whole step to the general path
  return (uint32_t)(c < FIN_CAP ? c : FIN_CAP);
}

// finer partitions (T > 8) go through two such kernels: 2^c1 coarse regions per band, then 2^(T-c1) fine
// regions inside each (2 x mean + 128, at most the LDS image)
// the T bits of a fine partition are split evenly over the two steps (6 + 6 at T = 12: runs of 64 records per
// (tile, part) in both, 64 reservations per tile; 8 + 4 measured 3.71 ms against 3.45 at 10 M queries)
static int coarse_bits(int T) { return (T + 1) / 2; }
static uint32_t coarse_region(int64_t nq, int c1) {
  // equal keys share a region: beside the hash-uniform spread there must be room for popular keys (one
  // with more copies than the LDS image overflows the fine step anyway)
  const double a = (double)nq / (double)(1 << c1);
  const double slack = a >= 4096.0 ? 0.25 * a + 8192.0 : 6.0 * sqrt(a) + 2.0 * a + 64.0;
  return (uint32_t)(((int64_t)(a + slack) + 63) / 64 * 64);
}
// small parts: the 512-thread / 4096-slot form of the finish (three workgroups per CU)
static bool small_form(int64_t nq, int T) { return (nq >> T) >= 1024 && (nq >> T) <= FIN_SMALL_MEAN; }
static uint32_t fine_region(int64_t nq, int T) {
  // real sizes (mean >= 1024 records per part): the LDS image of the finish form that will run (4096 records for
  // means up to 2800 -- 10 M queries: 2441 --, else 6144): reserved = 1.4 - 2 x the records; a part swollen by a
  // popular key spills into the pool.  Tiny inputs: 2 x mean + 128
  if ((nq >> T) >= 1024) return small_form(nq, T) ? FIN_SMALL_CAP : FIN_CAP;
  const int64_t c = ((nq >> T) * 2 + 128 + 63) / 64 * 64;
  return (uint32_t)(c < FIN_CAP ? c : FIN_CAP);
}
// records of the overflow pool behind the regions: 1/16 of the records of the call (what popular keys spill, plus the
// gathered copies of the spilled parts), at least 1 M, below 2^32
static size_t pool_records(int64_t nq, int32_t b) {
  size_t n = (size_t)b * (size_t)nq / 16;
  if (n < ((size_t)1 << 20)) n = (size_t)1 << 20;
  if (n > 0xFFFFFF00ull) n = 0xFFFFFF00ull;
  return n;
}
static size_t region_words(int64_t nq, int32_t b, int32_t part_bits) {
  return part_bits == 8 ? (size_t)b * RADIX * part_region(nq) : ((size_t)b << part_bits) * fine_region(nq, part_bits);
}

// words part_keys / part_ids (and, for part_bits > 8, tmp_keys / tmp_ids) must hold for qrlsh_bucket_pairs_emit
// (the id buffers are sized in 32-bit words as before; the records' 16-bit tails use the first half of them)
QRLSH_EXPORT size_t qrlsh_bucket_part_words(int64_t nq, int32_t b, int32_t part_bits) {
  if (nq <= 0 || b <= 0) return 0;
  const size_t plain = (size_t)b * nq;
  const size_t regions = region_words(nq, b, part_bits) + pool_records(nq, b);   // [regions][overflow pool]
  return regions > plain ? regions : plain;
}
QRLSH_EXPORT size_t qrlsh_bucket_tmp_words(int64_t nq, int32_t b, int32_t part_bits) {
  if (nq <= 0 || b <= 0 || part_bits <= 8) return 0;
  const size_t plain = (size_t)b * nq;
  const int c1 = coarse_bits(part_bits);
  const int64_t slab = 1ll << slab_bits(part_bits);
  // a region of its own per (band, slab, coarse part), each with the room a whole slab asks for
  const size_t regions = (((size_t)b * n_slabs(nq, part_bits)) << c1) * coarse_region(nq < slab ? nq : slab, c1);
  return regions > plain ? regions : plain;
}

// Partition + finish with the output range of every part reserved on a device cursor.
// total_overflow_out[0] ends up holding the exact number of pairs whether or not they fitted
// `capacity` words of pairs_out (nothing is written past it); [1] != 0 flags an oversized part.
QRLSH_EXPORT int qrlsh_bucket_pairs_emit(const uint64_t *keys, uint64_t *part_keys, uint32_t *part_ids,
                                         uint64_t *tmp_keys, uint32_t *tmp_ids, int64_t nq, int32_t b, int32_t r,
                                         int32_t part_bits, void *workspace, size_t workspace_bytes,
                                         uint64_t *pairs_out, uint64_t capacity, uint64_t *total_overflow_out,
                                         void *stream) {
  return qrlsh_bucket_pairs_emit_chunked(keys, 0, 0, 0, part_keys, part_ids, tmp_keys, tmp_ids, nq, b, r, part_bits,
                                         workspace, workspace_bytes, pairs_out, capacity, total_overflow_out, stream);
}

// The same with the keys of band t, query q at keys[(q / key_chunk) * key_chunk_stride + t * key_band_stride +
// q % key_chunk] -- the layout a band-partitioned all-to-all delivers ([rank][band][queries of that rank]:
// key_chunk = queries per rank, key_band_stride = key_chunk, key_chunk_stride = bands * key_chunk) -- so the
// multi-GPU driver needs no transposing copy.  key_chunk = 0: plain [b][nq].
QRLSH_EXPORT int qrlsh_bucket_pairs_emit_chunked(const uint64_t *keys, int64_t key_chunk, int64_t key_chunk_stride,
                                                 int64_t key_band_stride, uint64_t *part_keys, uint32_t *part_ids,
                                                 uint64_t *tmp_keys, uint32_t *tmp_ids, int64_t nq, int32_t b,
                                                 int32_t r, int32_t part_bits, void *workspace,
                                                 size_t workspace_bytes, uint64_t *pairs_out, uint64_t capacity,
                                                 uint64_t *total_overflow_out, void *stream) {
  QR_CHECK_ARG(key_chunk >= 0 && key_chunk_stride >= 0 && key_band_stride >= 0,
               "qrlsh_bucket_pairs_emit_chunked: bad key layout");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = bucket_check("qrlsh_bucket_pairs_emit", keys, part_keys, part_ids, tmp_keys, tmp_ids, nq, b, r,
                              part_bits, workspace, workspace_bytes, total_overflow_out, st);
  if (rc != QRLSH_OK || nq == 0) return rc;
  QR_CHECK_ARG(pairs_out || capacity == 0, "qrlsh_bucket_pairs_emit: null output with capacity %llu",
               (unsigned long long)capacity);
  uint32_t *ovf = reinterpret_cast<uint32_t *>(total_overflow_out + 1);
  if (nq > (1ll << (16 + part_bits))) {  // ids beyond what a record of the last step carries: the general path
    QR_MEMSET("qrlsh_bucket_pairs_emit", ovf, 1, 1, st);
    return QRLSH_OK;
  }
  const int nparts = 1 << part_bits;
  QrCarve c(workspace);
  const BucketWs w = bucket_layout(c, nq, b, part_bits);
#define QR_PART_SCATTER(LEVEL2_, ...) QR_LAUNCH("part_scatter", (part_scatter_atomic_kernel<LEVEL2_>), __VA_ARGS__)
  // Partition(s) into fixed regions + the LDS finish.  The bands are independent of each other all the way to the
  // pair cursor, so they are worked in GROUPS that alternate between the caller's stream and an auxiliary one
  // (api.hip: qr_aux_fork): while one group sits in the finish -- a chain of LDS phases that leaves most of the
  // memory system idle -- the next group's partition, which is nothing but memory traffic, shares the device with
  // it.  Same kernels, same buffers (every group touches only its own bands' regions, cursors and counts), results
  // as unordered as before; QRLSH_OVERLAP=0 (or an active profiler) runs the groups one after the other on the
  // caller's stream.
  const int T = part_bits;
  const bool two = T > 8;
  const int c1 = two ? coarse_bits(T) : 8;
  const int nslabs = n_slabs(nq, T), slab_shift = two ? slab_bits(T) : 63;
  const int64_t slab_nq = two && nq > (1ll << slab_shift) ? 1ll << slab_shift : nq;
  const uint32_t cap1 = two ? coarse_region(slab_nq, c1) : part_region(nq), cap2 = two ? fine_region(nq, T) : cap1;
  const uint32_t lowmask = (1u << (T - c1)) - 1u;
  // step-2 cursors end up as the parts' record counts, which the finish reads (one step: they are step 1's)
  uint32_t *cur1 = w.cur1, *cur2 = w.counts;
  // the records' 16-bit tails live in the id buffers
  uint16_t *part_tails = reinterpret_cast<uint16_t *>(part_ids), *tmp_tails = reinterpret_cast<uint16_t *>(tmp_ids);
  // the overflow pool behind the regions of the part buffers (PartPool above); the step that fills the parts the
  // finish reads spills into it (the coarse step of a two-step partition does not: its regions have their own slack)
  const size_t reg_words = region_words(nq, b, T);
  PartPool pool;
  pool.keys = part_keys + reg_words;
  pool.vals = part_tails + reg_words;
  pool.cursor = w.poolctl;
  pool.nruns = w.poolctl + 1;
  pool.cap = (uint32_t)pool_records(nq, b);
  pool.runs = w.runs;
  pool.runs_max = POOL_RUNS;
  pool.fill = w.fill;
  pool.slot_base = 0;
  PartPool no_pool = pool;
  no_pool.keys = nullptr;
  no_pool.vals = nullptr;
  // lists of the parts that outgrow the LDS image (bucket_finish_big_kernel), one counter and one list per band group
  constexpr int MAX_GROUPS = EMIT_MAX_GROUPS;
  unsigned long long *nbig0 = w.nbig;
  uint64_t *biglist0 = w.biglist;
  const uint64_t slots = (uint64_t)b << T;  // >= 256 words in that area
  // small parts: the 512-thread / 4096-slot finish
  const bool small_parts = two && small_form(nq, T);
  const int ntiles = (int)ceil_div64(nq, PS_TILE);
  const int64_t band_words = key_band_stride ? key_band_stride : nq;  // words between two bands of the key matrix
  // two groups (10 M queries x 32 bands: 18.84 ms per step with 1 group, 18.42 with 2, 18.9 with 4, 19.2 with 8);
  // small inputs: one (the second stream's fork / join and the extra launches cost more than the overlap
  // gives: 1.71 against 1.67 ms per step at 1 M queries x 32 bands)
  const int GROUPS = (int64_t)b * nq >= (64ll << 20) ? MAX_GROUPS : 1;
  const int per = (b + GROUPS - 1) / GROUPS;
  const int ngroups = (b + per - 1) / per;
  const uint64_t list_room = (slots - MAX_GROUPS) / (uint64_t)ngroups;
  const uint32_t big_max = (uint32_t)(list_room < FIN_BIG_LIST ? list_room : FIN_BIG_LIST);
  // What the call counts in is cleared first: fill marks (0xFF), both steps' cursors, the big-part counters, the
  // pool's cursor and run count -- and, with two or more groups, the run descriptors.  A group's gather
  // (bucket_big_gather_kernel) scans the descriptors while the next group's partition, on the other stream, counts
  // new runs in before it writes their descriptors: a slot in between still holds what an earlier call left there,
  // and one that names a part of this group would be counted twice (the overflow flag, and the step on the general
  // path).  Cleared, such a slot reads {0, 0 records}: it matches at most slot 0 and adds nothing.
  // (One kernel that clears all of it in a single launch measured slower than these calls: DESIGN section 6, round 6.)
  QR_MEMSET("qrlsh_bucket_pairs_emit", cur1, 0, (((size_t)b * nslabs) << c1) * sizeof(uint32_t), st);
  if (two) QR_MEMSET("qrlsh_bucket_pairs_emit", cur2, 0, ((size_t)b << T) * sizeof(uint32_t), st);
  QR_MEMSET("qrlsh_bucket_pairs_emit", w.fill, 0xFF, ((size_t)b << T) * sizeof(uint32_t), st);
  QR_MEMSET("qrlsh_bucket_pairs_emit", w.poolctl, 0, 16, st);
  QR_MEMSET("qrlsh_bucket_pairs_emit", nbig0, 0, MAX_GROUPS * sizeof(unsigned long long), st);
  if (ngroups > 1) QR_MEMSET("qrlsh_bucket_pairs_emit", w.runs, 0, (size_t)POOL_RUNS * sizeof(uint4), st);
  hipStream_t aux = nullptr;
  int gi = 0;
  for (int g0 = 0; g0 < b; g0 += per, ++gi) {
    const int nb = (b - g0 < per) ? b - g0 : per;
    hipStream_t s = (aux && (gi & 1)) ? aux : st;
    uint64_t *biglist = biglist0 + (size_t)gi * big_max;
    unsigned long long *nbig = nbig0 + gi;
    uint64_t *k1 = two ? tmp_keys : part_keys;
    uint16_t *v1 = two ? tmp_tails : part_tails;
    pool.slot_base = (uint32_t)((size_t)g0 << T);
    BigDesc *desc = w.desc + (size_t)gi * FIN_BIG_LIST;
    const size_t in0 = ((size_t)g0 * nslabs) << c1;  // the group's first region / cursor of the first step
    QR_PART_SCATTER(false, dim3(ntiles, nb), dim3(SORT_THREADS), 0, s, keys + (size_t)g0 * band_words,
                    (const uint16_t *)nullptr, k1 + in0 * cap1, v1 + in0 * cap1, nq, ntiles, 64 - c1, (1u << c1) - 1u,
                    cur1 + in0, cap1, ovf, qr_empty_key(r), (const uint32_t *)nullptr, 0u, key_chunk, key_chunk_stride,
                    key_band_stride, c1, nslabs, slab_shift, two ? no_pool : pool);
    if (two)
      QR_PART_SCATTER(true, dim3((unsigned)ceil_div64(cap1, PS_TILE), (nb * nslabs) << c1), dim3(SORT_THREADS), 0, s,
                      (const uint64_t *)tmp_keys + in0 * cap1, (const uint16_t *)tmp_tails + in0 * cap1,
                      part_keys + ((size_t)g0 << T) * cap2, part_tails + ((size_t)g0 << T) * cap2, (int64_t)0, 0, 64 - T,
                      lowmask, cur2 + ((size_t)g0 << T), cap2, ovf, qr_empty_key(r), (const uint32_t *)cur1 + in0, cap1,
                      (int64_t)0, (int64_t)0, (int64_t)0, c1, nslabs, slab_shift, pool);
    // the auxiliary stream is forked once the first group's partition is queued and before its finish is: the
    // second group's partition then starts beside the first group's finish, and the two streams stay half a
    // group out of step
    if (gi == 0 && b > per) aux = qr_aux_fork(st);
    // the group's parts: regions, record counts (step 2's cursors) and first slot
    const uint32_t slot0 = (uint32_t)((size_t)g0 << T);
    const uint64_t *gkeys = part_keys + (size_t)slot0 * cap2;
    const uint16_t *gids = part_tails + (size_t)slot0 * cap2;
    const uint32_t *gcounts = cur2 + slot0;
    if (small_parts && T >= 12)
      QR_LAUNCH("bucket_emit", bucket_finish_packed_kernel, dim3(nparts, nb), dim3(FIN_PK_THREADS), 0, s, gkeys, gids, nparts,
                64 - T, total_overflow_out, ovf, pairs_out, capacity, gcounts, cap2, biglist, nbig, big_max, slot0);
    else if (small_parts)
      QR_LAUNCH("bucket_emit", (bucket_finish_kernel<FIN_SMALL_THREADS, FIN_SMALL_CAP>), dim3(nparts, nb),
                dim3(FIN_SMALL_THREADS), 0, s, gkeys, gids, nparts, 64 - T, total_overflow_out, ovf, pairs_out, capacity, gcounts,
                cap2, biglist, nbig, big_max, slot0);
    else
      QR_LAUNCH("bucket_emit", (bucket_finish_kernel<>), dim3(nparts, nb), dim3(FIN_THREADS), 0, s, gkeys, gids, nparts, 64 - T,
                total_overflow_out, ovf, pairs_out, capacity, gcounts, cap2, biglist, nbig, big_max, slot0);
    // the parts of this group the finish listed as larger than its LDS image (usually none: the kernel then finds
    // an empty list), on the group's own stream: they are worked beside the next group
    QR_LAUNCH("bucket_emit_big", bucket_big_gather_kernel, dim3(64), dim3(256), 0, s, (const uint64_t *)biglist,
              (const unsigned long long *)nbig, big_max, desc, (const uint64_t *)part_keys, (const uint16_t *)part_tails,
              (const uint32_t *)cur2, cap2, pool, g_big_limit, ovf);
    QR_LAUNCH("bucket_emit_big", bucket_finish_big_kernel, dim3(FIN_BIG_GRID), dim3(FIN_THREADS), 0, s,
              (const uint64_t *)part_keys, (const uint16_t *)part_tails, (const uint64_t *)pool.keys,
              (const uint16_t *)pool.vals, 64 - T, (const BigDesc *)desc, (const unsigned long long *)nbig, big_max,
              total_overflow_out, pairs_out, capacity);
  }
  if (aux && qr_aux_join(st) != QRLSH_OK) return QRLSH_EHIP;
  QR_LAUNCH_CHECK("qrlsh_bucket_pairs_emit");
  return QRLSH_OK;
#undef QR_PART_SCATTER
}
