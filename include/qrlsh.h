/*
 * qrlsh.h -- C ABI of libqrlsh.so, the MI355X (gfx950) implementation of the
 * MinHash-LSH candidate-generation + pair-scoring hot path of
 * wamuumu/query-recommendation-system (lsh.py, recommender.py:105-214), the steps around it (answer sets, the
 * prediction loop, user similarity, recommendations), and the serving of queries that were not in the indexed set
 * (qrlsh_index_*, qrlsh_predict_columns) and of chosen users straight from the live neighbour lists, without a
 * prediction matrix (qrlsh_predict_users, qrlsh_recommend_users).
 *
 * The reference is pure Python and has no FFI of its own; this header is the
 * boundary its Python call surface (lsh.LSH, Recommender.compute_signatures /
 * compute_querySimilarities) binds through ctypes.  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - the caller owns every buffer (torch tensors in the Python host layer); the
 *     library never allocates device memory;
 *   - variable-size outputs are count-then-fill: *_count leaves the size in a
 *     device word the caller reads back, *_fill writes into caller memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all calls
 *     are asynchronous on it and safe under hipGraph capture (no allocation, no sync);
 *   - return value: 0 (QRLSH_OK) or a negative QRLSH_E* code; qrlsh_last_error()
 *     gives a thread-local message for the last failure on this thread.
 */
#ifndef QRLSH_H
#define QRLSH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QRLSH_OK 0
#define QRLSH_EINVAL (-1)       /* bad argument (incl. P % b != 0: lsh.py:20 asserts) */
#define QRLSH_EHIP (-2)         /* a HIP runtime call failed */
#define QRLSH_EUNSUPPORTED (-3) /* shape outside what the kernels cover */
#define QRLSH_EWORKSPACE (-4)   /* workspace too small */

#define QRLSH_PERM_U16 0 /* permutation table element = uint16 (D <= 65536) */
#define QRLSH_PERM_I32 1 /* permutation table element = int32 */

#define QRLSH_SIG_I32 0 /* signature rows int32 [nq][P] (the reference's values) */
#define QRLSH_SIG_U16 1 /* compact rows uint16 [nq][P], 0xFFFF = -1; only valid when D <= 65535 */

#define QRLSH_SORT_MIX 1u  /* radix digits are taken from mix64(key) (grouping sort) */
#define QRLSH_SORT_IOTA 2u /* first pass synthesises vals = index within the batch */
#define QRLSH_SORT_FOLD 4u /* digits from (key >> 32) << w | (key & (2^w - 1)), w = aux:
                              sorts pairs i << 32 | j over [0, 2w) in ceil(2w / 8) passes */
#define QRLSH_SORT_OWNER 8u /* ONE pass whose digit is (key >> bit_lo) / aux: groups words by the rank
                               that owns the id starting at bit_lo (shards of aux ids, <= 256 ranks) */

#define QRLSH_SORT_HOST 16u /* ONE pass over pair words i << 32 | j whose digit is the rank that scores the pair
                               in the sharded driver: the owner (shards of aux ids) of i or of j, chosen by
                               the top bit of mix64(pair) -- an even split of the pairs for any id structure */

int qrlsh_version(void);
const char *qrlsh_last_error(void);

/* 64-bit bijective mixer used by QRLSH_SORT_MIX (host copy, for tests) */
uint64_t qrlsh_mix64_host(uint64_t x);

/* ---- a1: MinHash signatures ------------------------------------------------
 * Replaces Recommender.compute_signatures, recommender.py:105-143:
 *     sig[q][p] = min_{d in A(q)} perm_p[d],  -1 when A(q) is empty.
 * offsets[nq+1] / rows[nnz] : CSR answer sets (compute_shingles' output, :68-103)
 * perm_t : the P permutations TRANSPOSED, [D][P_stride] (row d = the P permuted
 *          indices of table row d), element type perm_dtype; P_stride >= P, and
 *          P_stride * sizeof(element) a multiple of 16.
 * sig_out   [nq][P] int32 (row-major; the reference returns the same matrix as int64), or NULL
 * sig16_out [nq][P] uint16 compact rows (0xFFFF = -1), or NULL; needs D <= 65535 and a uint16
 *           table.  At least one of sig_out / sig16_out.  Half the bytes for qrlsh_score_pairs.
 * norm2_out [nq] int64 = sum_p sig^2 (exact), or NULL          -- feeds qrlsh_score_pairs
 * keys_out  [b][nq] uint64 band keys (see qrlsh_band_keys), or NULL -- fused a2
 * PRECONDITION (not checked by qrlsh_minhash itself, which gathers table row rows[k] directly): offsets[0] = 0,
 * offsets non-decreasing, offsets[nq] = nnz and 0 <= rows[k] < D.  qrlsh_check_csr tests exactly that on the
 * device: *flags_out (device uint32) = 0 when it holds, else bit 0 = bad first / last offset, bit 1 = offsets
 * decrease, bit 2 = a row id out of range.
 */
int qrlsh_check_csr(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t nnz, int32_t D,
                    uint32_t *flags_out, void *stream);
int qrlsh_minhash(const int64_t *offsets, const int32_t *rows, int64_t nq, const void *perm_t,
                  int32_t perm_dtype, int32_t P, int32_t P_stride, int32_t D, int32_t *sig_out,
                  uint16_t *sig16_out, int64_t *norm2_out, uint64_t *keys_out, int32_t b, void *stream);

/* ---- a2: band keys -----------------------------------------------------------
 * Replaces LSH.make_subvecs / compute_buckets' key construction, lsh.py:17-38:
 * band i of a signature = its values [i*r, (i+1)*r) cast to int16 (:28) and joined
 * into a string (:33).  Equal strings <=> equal int16 tuples, so for r <= 4
 *     key = sum_k (sig[i*r + k] & 0xFFFF) << (16 * k)
 * is an exact bucket id.  For r > 4 ("wide bands") the key is a 64-bit hash of the tuple (the all
 * -1 tuple still maps to ~0): bucket ids are then exact only up to hash collisions, and the
 * caller must pass the unique pairs through qrlsh_verify_pairs (below) to stay exact.
 * keys_out is band-major [b][nq].  norm2_out optional.  Returns QRLSH_EINVAL if P % b != 0.
 */
int qrlsh_band_keys(const int32_t *sig, int64_t nq, int32_t P, int32_t b, uint64_t *keys_out,
                    int64_t *norm2_out, void *stream);

/* ---- radix sort (replaces the dict-of-lists buckets, lsh.py:9-15,31-38) -------
 * Stable LSD radix sort of nbatch independent arrays of n uint64 keys (+ optional
 * uint32 payload), 8 bits per pass over bits [bit_lo, bit_hi) of the key (or of
 * mix64(key) with QRLSH_SORT_MIX: equal keys still end up adjacent, in payload
 * order, after 32 bits instead of 64).  The range is exact: the order is that of ONE
 * stable sort by bits [bit_lo, bit_hi) alone, whatever the bits at and above bit_hi hold
 * (a last pass narrower than 8 bits masks its digit).  Buffers a/b ping-pong; the return
 * value (>= 0) says where the result is: 0 = a, 1 = b.  vals_a/vals_b may both be NULL.
 */
size_t qrlsh_sort_workspace_bytes(int64_t n, int32_t nbatch);
int qrlsh_sort_u64(uint64_t *keys_a, uint64_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, int64_t n,
                   int32_t nbatch, int32_t bit_lo, int32_t bit_hi, uint32_t flags, uint64_t aux,
                   void *workspace, size_t workspace_bytes, void *stream);

/* split points of words grouped with QRLSH_SORT_OWNER: bounds_out[g] (device int64 [world+1]) = first
 * position whose owner (word >> bit_lo) / shard is >= g.  bit_lo = -1: pair words grouped with
 * QRLSH_SORT_HOST (owner = the scoring rank of the pair). */
int qrlsh_owner_bounds(const uint64_t *words, int64_t n, int32_t bit_lo, uint64_t shard, int32_t world,
                       int64_t *bounds_out, void *stream);

/* ---- a3: candidate pairs -------------------------------------------------------
 * Replaces LSH.get_candidates, lsh.py:40-55.  Input: per band, keys sorted with
 * QRLSH_SORT_MIX over the top hash_bits (8..32) bits of mix64(key), i.e. bits
 * [64 - hash_bits, 64), and their query ids ([b][nq] each).  Every run of
 * equal keys that is not the all -1 tuple (:47) yields all its (i < j) pairs (:49).
 * pairs are i << 32 | j; duplicates across bands are still present (the Python
 * set's job, :41) -- sort them and call qrlsh_unique_*.
 *   count: *total_out (device uint64) = number of pairs; workspace keeps per-block offsets
 *   fill : writes exactly that many pairs (capacity checked by the caller)
 */
size_t qrlsh_pairs_workspace_bytes(int64_t nq, int32_t b);
int qrlsh_pairs_count(const uint64_t *sorted_keys, int64_t nq, int32_t b, int32_t r, int32_t hash_bits,
                      void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream);
int qrlsh_pairs_fill(const uint64_t *sorted_keys, const uint32_t *sorted_ids, int64_t nq, int32_t b,
                     int32_t r, int32_t hash_bits, const void *workspace, uint64_t *pairs_out,
                     void *stream);

/* Fast form of the same step for keys straight from qrlsh_minhash / qrlsh_band_keys (band-major
 * [b][nq], NOT sorted): a hash partition on the top part_bits (8..16) bits of mix64(key) into
 * part_keys / part_ids, then an LDS hash-group finish per (part, band).  Pick part_bits so that
 * nq / 2^part_bits is ~2-4 K.  Same pairs as the general path, in no particular (still
 * duplicate-carrying) order.
 * Output: every part reserves its output range on a device cursor, so there is no count pass -- at the price
 * of sizing pairs_out by a guess.  At most `capacity` words of pairs_out are written; total_overflow_out[2]
 * (device uint64 x2) receives {the exact number of pairs whether or not they fitted, overflow flag}.  A total
 * beyond capacity: allocate that many and call again.  Overflow flag != 0 (heavily skewed data): nothing of the
 * call is usable, take the general path (qrlsh_sort_u64 + qrlsh_pairs_count / _fill) instead.
 * Partition: ONE kernel per level (one level for part_bits = 8, two of about part_bits / 2 bits each beyond:
 * tmp_keys / tmp_ids are the buffers in between, may be NULL for 8) that gives every part a fixed region of ONE
 * LDS image of the finish and reserves room in it with an atomic per (tile, part) -- no histogram pass, no scan, no
 * bounds search.  part_keys / part_ids must hold qrlsh_bucket_part_words(nq, b, part_bits) words and, for
 * part_bits > 8, tmp_keys / tmp_ids qrlsh_bucket_tmp_words(...).
 * Pool: behind the regions the same buffers hold an OVERFLOW POOL (1/16 of the records, at least 1 M): a part
 * swollen by a popular key (lsh.py:42-49 makes a bucket of m queries m(m-1)/2 pairs whatever m is; at 100 M queries
 * over 32768 table rows m reaches ~20 000) spills there and is worked in blocks of one image; only a part beyond
 * qrlsh_set_big_part_limit records (default 16 images = 98 304), more than 4096 such parts per band group, or an
 * exhausted pool raise the overflow flag.  Reserved: ~1.4 - 2 x the b * nq records.  These buffers are scratch.
 * What they hold afterwards are 10-byte records, not keys and ids: part_keys a 64-bit word per record -- the low
 * 64 - part_bits bits of mix64(key) (a bijection of the keys; the top part_bits bits are the part number, which the
 * record's place says) with the query id's bits from 16 up above them -- and part_ids, used as uint16_t storage, the
 * id's low 16 bits at the record's index (the first half of the buffer; the sizes stay counted in 32-bit words).
 * tmp_keys / tmp_ids hold the same form after the first level, per slab of 2^(16 + first level's bits) consecutive
 * queries.  The records of empty bands are gone.  nq beyond 2^(16 + part_bits) raises the overflow flag. */
size_t qrlsh_bucket_workspace_bytes(int64_t nq, int32_t b, int32_t part_bits);
size_t qrlsh_bucket_part_words(int64_t nq, int32_t b, int32_t part_bits);
/* records a part beyond the LDS image may hold and stay on the partition path (<= 0 or beyond the maximum: the
 * default, 98 304); returns the previous limit.  Process-wide; a tuning / test knob. */
int64_t qrlsh_set_big_part_limit(int64_t records);
size_t qrlsh_bucket_tmp_words(int64_t nq, int32_t b, int32_t part_bits);
int qrlsh_bucket_pairs_emit(const uint64_t *keys, uint64_t *part_keys, uint32_t *part_ids,
                            uint64_t *tmp_keys, uint32_t *tmp_ids, int64_t nq, int32_t b, int32_t r,
                            int32_t part_bits, void *workspace, size_t workspace_bytes,
                            uint64_t *pairs_out, uint64_t capacity, uint64_t *total_overflow_out,
                            void *stream);

/* qrlsh_bucket_pairs_emit with the keys of band t, query q at
 *     keys[(q / key_chunk) * key_chunk_stride + t * key_band_stride + q % key_chunk]
 * -- what a band-partitioned all-to-all delivers ([rank][band][queries of that rank]: key_chunk = queries
 * per rank, key_band_stride = key_chunk, key_chunk_stride = bands * key_chunk), so the multi-GPU driver
 * needs no transposing copy; key_chunk_stride may exceed bands * key_chunk (a band range read out of a buffer
 * that holds more bands per rank).  key_chunk = 0: plain [b][nq].  Chunked keys need nq < 2^32. */
int qrlsh_bucket_pairs_emit_chunked(const uint64_t *keys, int64_t key_chunk, int64_t key_chunk_stride,
                                    int64_t key_band_stride, uint64_t *part_keys, uint32_t *part_ids,
                                    uint64_t *tmp_keys, uint32_t *tmp_ids, int64_t nq, int32_t b, int32_t r,
                                    int32_t part_bits, void *workspace, size_t workspace_bytes,
                                    uint64_t *pairs_out, uint64_t capacity, uint64_t *total_overflow_out,
                                    void *stream);

/* unique of a sorted uint64 array (count-then-fill) */
size_t qrlsh_compact_workspace_bytes(int64_t n);
int qrlsh_unique_count(const uint64_t *sorted, int64_t n, void *workspace, size_t workspace_bytes,
                       uint64_t *total_out, void *stream);
int qrlsh_unique_fill(const uint64_t *sorted, int64_t n, const void *workspace, uint64_t *out,
                      void *stream);

/* Sorted unique pairs from pairs that are only GROUPED BY i (qrlsh_sort_u64 over bits [32, 32 + id_bits)
 * of the emitted i << 32 | j words: about half the passes of the full (i, j) sort): every row -- the
 * pairs of one i, tens of words -- is de-duplicated (hash set) and ordered by j in LDS.  Replaces the Python set of
 * lsh.py:41,53 like qrlsh_unique_*, same result.  group_bits > 0: the words are ordered by
 * i >> group_bits only (a row is then 2^group_bits consecutive i; every id < 2^id_bits and group_bits +
 * id_bits <= 32) -- at 2^20 ids that is two radix passes instead of three.  count: tmp is scratch of n
 * words; leaves {number of
 * unique pairs, overflow flag} in total_overflow_out[2] (device uint64 x2); rows that do not fit a
 * workgroup's chunk image (more than ~1024 pairs past a 2048-word boundary) get a workgroup of their own;
 * overflow != 0 means one i has more than 12288 emitted pairs: ignore the total and use the general
 * path (full qrlsh_sort_u64 + qrlsh_unique_*) on the same words.  fill follows a count on the same
 * tmp / workspace and writes exactly `total` words, ascending.
 */
size_t qrlsh_row_unique_workspace_bytes(int64_t n);
int qrlsh_row_unique_count(const uint64_t *grouped, int64_t n, int32_t group_bits, int32_t id_bits,
                           uint64_t *tmp, void *workspace, size_t workspace_bytes, uint64_t *total_overflow_out,
                           void *stream);
int qrlsh_row_unique_fill(const uint64_t *tmp, int64_t n, const void *workspace, uint64_t *out, void *stream);

/* The same result from words grouped by i >> group_bits with group_bits up to 8 (REGIONS of 2^group_bits
 * consecutive queries, a few thousand words each: at 2^24 ids and group_bits = 8 the grouping sort needs two
 * radix passes, not three): one workgroup per region streams its words through an LDS hash set of the 32-bit
 * values (i's low bits, j), counts the distinct ones per i, and places each by the number of smaller ones of
 * its own i.  Only the DISTINCT pairs of a region are bounded, not its words: about 5 K in the main kernel,
 * about 11 K in the big-image kernel that takes over the regions beyond that (very popular queries).  nids = number of query
 * ids (regions = ceil(nids / 2^group_bits)); needs group_bits + id_bits <= 32, and nids < 2^id_bits when it is
 * exactly 32.  count / fill / overflow as qrlsh_row_unique_*.  This is the default de-duplication of the
 * pipeline; qrlsh_row_unique_* remains for id widths that leave no room for group bits. */
size_t qrlsh_region_unique_workspace_bytes(int64_t nids, int32_t group_bits);
int qrlsh_region_unique_count(const uint64_t *grouped, int64_t n, int32_t group_bits, int32_t id_bits, int64_t nids,
                              uint64_t *tmp, void *workspace, size_t workspace_bytes, uint64_t *total_overflow_out,
                              void *stream);
int qrlsh_region_unique_fill(const uint64_t *tmp, int64_t n, int32_t group_bits, int64_t nids, const void *workspace,
                             uint64_t *out, void *stream);

/* The same de-duplication WITHOUT the grouping sort: the region finish needs the words grouped by region (i >> group_bits)
 * and nothing about the order inside a group, so the stable radix passes (a histogram pass, a scan and a scatter per 8
 * bits) are replaced by a most-significant-digit-first partition into FIXED regions with one atomic reservation per
 * (tile, digit): one read and one write of the words per level, two levels for up to 65536 regions.
 * qrlsh_pair_regions_scatter32 deals the n emitted words into regions[r * cap ..) (counts[r] entries each; cap =
 * qrlsh_pair_regions_cap, buffers of qrlsh_pair_regions_words / _tmp_words entries, counts of _count + 256 uint32);
 * words_per_query: what a query of the populated id range emits on average (0: n / nids) -- sizes the regions (3 x the
 * mean + 4096: i is the smaller id of a pair, so low ids carry up to twice the mean).  *overflow_out != 0: a region
 * outgrew its capacity (group with qrlsh_sort_u64 instead).  qrlsh_pair_regions_words returns 0 when the id space has
 * more than 65536 regions, or when a level's regions reach 2^32 words -- the scatter places words with 32-bit offsets,
 * so it needs na * cap_a < 2^32 (level 1: na = tmp_words / cap_a coarse digits) and 2^rb * cap_b < 2^32 (the final
 * regions of one coarse digit) -- (not served; the scatter rejects such sizes with QRLSH_EINVAL before any device
 * work; a large words_per_query hint reaches them first).
 * An entry of a region is the 32-bit value (i & (2^group_bits - 1)) << id_bits | j, not the pair word: the region already
 * says every bit of i above the low group_bits, and the finish reduces each word to that value first thing.  So the form
 * needs group_bits + id_bits <= 32 and a value that is never 0xFFFFFFFF, the finish's empty-slot marker (group_bits +
 * id_bits < 32, or nids < 2^id_bits); both calls return QRLSH_EINVAL otherwise, before any device work.  `regions` holds
 * qrlsh_pair_regions_words uint32; tmp_regions qrlsh_pair_regions_tmp_words uint64 (16-byte aligned; NULL when that is 0),
 * of which the first of two levels uses 5 bytes per entry: the values as uint32, then as many bytes with the low digit
 * of each entry's region id.
 * qrlsh_region_unique_count_regions32 is qrlsh_region_unique_count on those regions (same group_bits / id_bits / nids,
 * counts and cap; tmp: as many uint64 as the region buffer has entries) with one result buffer for both steps, so that
 * the host reads back once: scatter_overflow is the DEVICE word the scatter wrote on the same stream; out3 (3 words) =
 * {total, distinct-overflow (a region holds more distinct pairs than the finish can), capacity-overflow
 * (*scatter_overflow)}.  qrlsh_region_unique_fill follows it as usual. */
size_t qrlsh_pair_regions_words(int64_t n, int64_t nids, int32_t group_bits, double words_per_query);
size_t qrlsh_pair_regions_tmp_words(int64_t n, int64_t nids, int32_t group_bits, double words_per_query);
int64_t qrlsh_pair_regions_cap(int64_t n, int64_t nids, int32_t group_bits, double words_per_query);
int64_t qrlsh_pair_regions_count(int64_t n, int64_t nids, int32_t group_bits, double words_per_query);
int qrlsh_pair_regions_scatter32(const uint64_t *words, int64_t n, int32_t group_bits, int32_t id_bits, int64_t nids,
                                 double words_per_query, uint64_t *tmp_regions, uint32_t *regions, uint32_t *counts,
                                 uint32_t *overflow_out, void *stream);
int qrlsh_region_unique_count_regions32(const uint32_t *regions, const uint32_t *counts, int64_t cap, int64_t n,
                                        int32_t group_bits, int32_t id_bits, int64_t nids, uint64_t *tmp, void *workspace,
                                        size_t workspace_bytes, const uint32_t *scatter_overflow, uint64_t *out3,
                                        void *stream);

/* ---- a5: pair scoring ------------------------------------------------------------
 * Replaces the cosine of recommender.py:203-204 for one candidate pair:
 *     np.around(cosine_similarity([sig_i, sig_j])[0][1], 3)
 * computed as exact integer dot / (sqrt(norm2_i) * sqrt(norm2_j)) in float64 (0 if a
 * norm is 0, as sklearn's normalize does), milli = rint(cos * 1000) so that
 * milli / 1000.0 == np.around(cos, 3).  sig is int32 [n][P] (QRLSH_SIG_I32) or the compact
 * uint16 rows written by qrlsh_minhash (QRLSH_SIG_U16).
 * norm2 may be NULL: the two squared norms are then summed from the rows inside the kernel (same exact integers;
 * slower on MI355X -- 5.1 vs 4.4 ms on 45 M pairs: the kernel is short of integer-multiply throughput, not of the
 * 64-byte sector a precomputed norm costs).
 * cos_out (double, unrounded) and edge_out are optional.  edge_out[2n] receives the two
 * directed top-K sort keys of each pair:
 *     src << (id_bits + 11) | (1000 - milli) << id_bits | dst        (needs id_bits <= 26)
 * or, when edge_dst_out[2n] is given (any id width, "wide ids"),
 *     edge_out = src << 11 | (1000 - milli),  edge_dst_out = dst   (a key + payload record).
 */
int qrlsh_row_norms(const int32_t *sig, int64_t nq, int32_t P, int64_t *norm2_out, void *stream);
/* exact candidate test (needed only for r = P / b > 4): flags_out[t] = 1 iff pair t shares a band
 * whose r int16 values are all equal and not all -1 (lsh.py:31-53) */
int qrlsh_verify_pairs(const void *sig, int32_t sig_dtype, int32_t P, int32_t b, const uint64_t *pairs,
                       int64_t n, uint8_t *flags_out, void *stream);
int qrlsh_score_pairs(const void *sig, int32_t sig_dtype, const int64_t *norm2, int32_t P,
                      const uint64_t *pairs, int64_t n, int32_t *milli_out, double *cos_out,
                      uint64_t *edge_out, int32_t id_bits, uint32_t *edge_dst_out, void *stream);

/* ---- a5: per-query top-K -----------------------------------------------------------
 * Replaces argsort(values)[::-1][:K] per query, recommender.py:206-210, on the edge keys
 * sorted ascending (so: src, value descending, dst ascending -- the documented
 * tie-break; the reference's own tie order is arbitrary).  count-then-fill; the output
 * is COO (src, dst, milli), at most K rows per src.  Wide-id edges: id_bits = 0 and sorted_dst =
 * the payload sorted along with the keys (NULL for the packed format).
 */
int qrlsh_topk_count(const uint64_t *sorted_edges, int64_t n_edges, int32_t K, int32_t id_bits,
                     void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream);
int qrlsh_topk_fill(const uint64_t *sorted_edges, const uint32_t *sorted_dst, int64_t n_edges, int32_t K,
                    int32_t id_bits, const void *workspace, int32_t *src_out, int32_t *dst_out,
                    int32_t *milli_out, void *stream);
/* the same with src_base added to every src written (edge keys whose src field is relative to a rank's
 * first query id: qrlsh_edges_localize) */
int qrlsh_topk_fill_based(const uint64_t *sorted_edges, const uint32_t *sorted_dst, int64_t n_edges, int32_t K,
                          int32_t id_bits, int64_t src_base, const void *workspace, int32_t *src_out,
                          int32_t *dst_out, int32_t *milli_out, void *stream);

/* Select form of the same cut, without sorting the directed edges: the forward edges of a query are its run of
 * the (sorted) scored pair list; only the n reverse words qrlsh_score_pairs_rev writes (rev_out[t] =
 * j << (id_bits + 11) | inv << id_bits | i, or key + payload j << 11 | inv, i for ids beyond 26 bits) are
 * sorted, stably, on j's bits alone -- ceil(id_bits / 8) passes over n words instead of ceil((id_bits + 11) / 8)
 * over 2n.  Every directed edge then counts the edges of its query's two runs that order before it (value
 * descending, neighbour id ascending; at most K of them are looked for) and, if fewer than K do, lands at that
 * rank of its query's output row.  count: *total_out = number of edges kept; fill writes the same (src, dst,
 * milli) COO qrlsh_topk_fill does.  nq = number of query ids; n < 2^31 pairs.
  * pairs == NULL (and milli == NULL in _fill): the lists are made of the n reverse words alone, whatever scored them
 * (the sharded driver: every directed edge a rank receives, re-based to its id range by qrlsh_edges_localize, IS
 * such a word with src = one of its own queries; sorted on the src bits only); packed words then need
 * src < 2^(53 - id_bits) instead of id_bits <= 26.
 */
int qrlsh_score_pairs_rev(const void *sig, int32_t sig_dtype, const int64_t *norm2, int32_t P,
                          const uint64_t *pairs, int64_t n, int32_t *milli_out, uint64_t *rev_out, int32_t id_bits,
                          uint32_t *rev_dst_out, void *stream);
/* 1 (default): compact rows of 128 / 256 values with precomputed norms are scored by the run form (16 consecutive pairs
 * per 16-lane group, first row kept while it does not change); 0: by the generic form.  Same results bit for bit; an
 * A/B and test knob.  Returns the previous setting (-1: not yet decided, i.e. the default). */
int qrlsh_set_score_runs(int on);
size_t qrlsh_topk_select_workspace_bytes(int64_t nq);
int qrlsh_topk_select_count(const uint64_t *pairs, int64_t n, const uint64_t *rev_sorted, const uint32_t *rev_dst,
                            int64_t nq, int32_t K, int32_t id_bits, void *workspace, size_t workspace_bytes,
                            uint64_t *total_out, void *stream);
int qrlsh_topk_select_fill(const uint64_t *pairs, const int32_t *milli, int64_t n, const uint64_t *rev_sorted,
                           const uint32_t *rev_dst, int64_t nq, int32_t K, int32_t id_bits, const void *workspace,
                           int32_t *src_out, int32_t *dst_out, int32_t *milli_out, void *stream);

/* ---- multi-GPU glue (one process per GPU; qrlsh/dist.py) ----------------------------------------------
 * remap_pairs: an owner scores pairs (i local, j anywhere) against a row table [its nql local rows | the
 * fetched remote rows]; out[t] = (i - q0) << 32 | slot(j), slot(j) = j - q0 for a local j, else nql + the
 * position of j in `need` (the ascending global ids of the fetched rows).
 * pair_edges: the directed edge keys of scored pairs, forward (src = i) and reverse (src = j) in separate
 * arrays: packed (id_bits > 0, as qrlsh_score_pairs writes them) or key + payload (id_bits == 0).
 */
int qrlsh_remap_pairs(const uint64_t *pairs, int64_t n, int64_t q0, int64_t nql, const uint64_t *need,
                      int64_t n_need, uint64_t *out, void *stream);
int qrlsh_pair_edges(const uint64_t *pairs, const int32_t *milli, int64_t n, int32_t id_bits,
                     uint64_t *fwd_out, uint64_t *rev_out, uint32_t *fwd_dst_out, uint32_t *rev_dst_out,
                     void *stream);
/* (rev_out == NULL: both edges of pair t go to fwd_out[2t], fwd_out[2t+1] -- and fwd_dst_out likewise --
 * exactly the layout qrlsh_score_pairs' edge_out has.)
 *
 * Sharded scoring.  A pair is scored on the rank qr_pair_host names (QRLSH_SORT_HOST): the owner of one of
 * its two queries, so at most one of its signature rows is remote.
 *   idset_*: the set of remote ids a rank's pairs touch, as a bitmap over the nids global ids plus its rank
 *     structure, kept in `workspace` (qrlsh_idset_workspace_bytes).  build marks both endpoints of every
 *     pair outside [q0, q0 + nql) and leaves in bounds_out[g] (device int64 [world + 1]) the number of marked
 *     ids below g * shard -- the per-owner request sizes, bounds_out[world] = the total; list writes the ids
 *     ascending (the row-fetch request); remap rewrites each pair as slot(i) << 32 | slot(j) into the row
 *     table [nql local rows | fetched rows in id order]: slot(x) = x - q0 if local, else nql + rank of x.
 *   gather_rows: the answer to such a request on the owning rank: rows_out[k] = signature row ids[k] - q0
 *     (row_bytes bytes, a multiple of 16), norms_out[k] its norm.
 *   score_pairs_split: qrlsh_score_pairs against a row table in two pieces -- row x < split_rows from
 *     sig / norm2, the others (x - split_rows) from sig_b / norm2_b -- so the fetched rows are never copied.
 *   edges_localize: directed edges that arrived at the owner of their src (packed, or key + payload when
 *     edge_dst is given) re-based to its id range: (src - q0) << (id_bits + 11) | inv << id_bits | dst, which
 *     fits one word whenever bits(nql) + 11 + id_bits <= 64; the top-K sort then orders (src, value, dst)
 *     completely (edges from several scoring ranks arrive in no useful order). */
size_t qrlsh_idset_workspace_bytes(int64_t nids);
int qrlsh_idset_build(const uint64_t *pairs, int64_t n, int64_t q0, int64_t nql, int64_t nids, int64_t shard,
                      int32_t world, void *workspace, size_t workspace_bytes, int64_t *bounds_out, void *stream);
int qrlsh_idset_list(const void *workspace, int64_t nids, uint64_t *ids_out, void *stream);
int qrlsh_idset_remap(const uint64_t *pairs, int64_t n, int64_t q0, int64_t nql, const void *workspace,
                      int64_t nids, uint64_t *out, void *stream);
int qrlsh_gather_rows(const void *sig, int64_t row_bytes, const int64_t *norm2, const uint64_t *ids, int64_t n,
                      int64_t q0, void *rows_out, int64_t *norms_out, void *stream);
int qrlsh_score_pairs_split(const void *sig, const int64_t *norm2, int64_t split_rows, const void *sig_b,
                            const int64_t *norm2_b, int32_t sig_dtype, int32_t P, const uint64_t *pairs,
                            int64_t n, int32_t *milli_out, void *stream);
int qrlsh_edges_localize(const uint64_t *edges, const uint32_t *edge_dst, int64_t n, int32_t id_bits, int64_t q0,
                         int64_t nql, uint64_t *out, void *stream);

/* ---- N2: answer sets (the producer of the hot path's input) ---------------------------------
 * Replaces Recommender.compute_shingles, recommender.py:68-103, for queries that are
 * conjunctions of attribute=value: bitmaps[row][words_per_row] holds one bit per table row for
 * every (feature, value) of the table (bit i of word w = table row 32*w + i; D = table rows);
 * qrows[q][f] names the bitmap row of query q's value for feature f, -1 = unconstrained (a value
 * absent from the table points at an all-zero row).  count: sizes_out[q] = |A(q)|;
 * fill: rows_out[offsets[q] ..) = the matching table rows, ascending (offsets = exclusive scan
 * of the sizes) -- the CSR qrlsh_minhash consumes.  nfeat <= 64.
 */
int qrlsh_answer_sets_count(const uint32_t *bitmaps, int64_t words_per_row, int64_t D,
                            const int32_t *qrows, int64_t nq, int32_t nfeat, int32_t *sizes_out,
                            void *stream);
int qrlsh_answer_sets_fill(const uint32_t *bitmaps, int64_t words_per_row, int64_t D,
                           const int32_t *qrows, int64_t nq, int32_t nfeat, const int64_t *offsets,
                           int32_t *rows_out, void *stream);

/* one-sweep form of the two calls above: sweep = sizes + the first 64 row ids of every query
 * parked in slots_out[nq][64]; after the exclusive scan of the sizes, compact moves the slots of the
 * queries with <= 64 rows to their CSR positions.  Queries with more rows (sizes_out > 64) still
 * need qrlsh_answer_sets_fill (pass it a qrows/offsets subset, or call it for all). */
int qrlsh_answer_sets_sweep(const uint32_t *bitmaps, int64_t words_per_row, int64_t D,
                            const int32_t *qrows, int64_t nq, int32_t nfeat, int32_t *sizes_out,
                            int32_t *slots_out, void *stream);
int qrlsh_answer_sets_compact(const int32_t *slots, const int64_t *offsets, int64_t nq,
                              int32_t *rows_out, void *stream);

/* ---- N1: hybrid prediction loop (the consumer of the hot path's output) ---------------------
 * Replaces the per-cell loop of Recommender.compute_scores, recommender.py:301-331, and
 * weighted_average, recommender.py:36-47.  ratings int32 [nu][nq] (0 = missing).  Query
 * neighbours in CSR form (q_off[nq+1], q_idx, q_val = rounded cosine, i.e. milli / 1000.0) as
 * qrlsh_topk_* produce them; user neighbours padded [nu][ku] (u_idx = -1 past the end).
 * out[nu][nq] = the utility matrix with every zero cell replaced by round(blend) (0 when neither
 * side predicts).  float64 arithmetic, no FMA, round half to even.  sum_order picks the order of the two
 * np.sum calls inside weighted_average: QRLSH_SUM_PAIRWISE = numpy's pairwise sum (the reference run as
 * plain Python; the order the committed fixtures pin), QRLSH_SUM_SEQUENTIAL = one accumulator in index
 * order (what numba's nopython np.sum does where numba is installed; unpinned here).
 * Limits: ku <= 64 (QRLSH_EINVAL otherwise); a query with more than 64 neighbours sets *too_long_out
 * (device uint32, required) to 1; its cells are never walked (they get 0) and the result is not to be used -- the
 * caller reads the flag back.
 * kq > 0 with a workspace of qrlsh_predict_workspace_bytes(nu, nq, kq): the caller states the longest query list
 * (kq <= 64; a longer one sets the flag, as above) and the kernel that fits the data runs, same results from all:
 *   tile form (ku <= 32, every rating in 0 .. 255 -- the reference's are 0 .. 100): the matrix is transposed to
 *     bytes in the workspace, a workgroup owns 64 users x 16 queries, every list is read once per tile and the
 *     rating gathers are 64 consecutive bytes (query side) or stay inside one nu-byte row (user side);
 *   row form (nq <= 131072; what runs when a rating does not fit a byte -- decided on the device, no read-back):
 *     one workgroup per user slice, the lists transposed to [kq][nq] in the workspace, the user's row in LDS;
 *   cell form otherwise: one thread per cell over the transposed lists.
 * kq = 0 / workspace = NULL: one thread per cell over the lists in their CSR form.
 */
#define QRLSH_SUM_PAIRWISE 0
#define QRLSH_SUM_SEQUENTIAL 1
size_t qrlsh_predict_workspace_bytes(int64_t nu, int64_t nq, int32_t kq);
int qrlsh_predict(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off,
                  const int32_t *q_idx, const double *q_val, const int32_t *u_idx, const double *u_val,
                  int32_t ku, double query_weight, double user_weight, double default_mean,
                  int32_t sum_order, int32_t *out, uint32_t *too_long_out, int32_t kq, void *workspace,
                  size_t workspace_bytes, void *stream);

/* Column prediction for NEW queries (not columns of the matrix): x has no ratings, so the user side of every cell
 * (u, x) is 0 (recommender.py:320 over an all-zero column) and
 *     out[x][u] = qp == 0 ? 0 : round(qp * (query_weight + user_weight * 0.5) + default_mean * (user_weight * 0.5)),
 *     qp = weighted_average(ratings[u], idx[off[x] ..), milli[off[x] ..) / 1000.0)
 * -- qrlsh_predict's cell of a zero column appended to the matrix, same arithmetic (float64, no FMA, half to even, the
 * similarity a true division, both sum orders).  ratings int32 [nu][nq]; x's neighbour list in CSR form (off[m+1],
 * idx in [0, nq), milli) as qrlsh_index_probe_finish writes it; out int32 [m][nu] (query-major: the rows
 * qrlsh_recommend_topk reads for the users of each new query).  *flags_out (device uint32, required) = 0, or bit 0:
 * a list is longer than 64 entries, bit 1: an index outside [0, nq); such a list is never walked, its row gets 0
 * and the result is not to be used -- the caller reads the flags back.  nu <= 65535 * 256. */
int qrlsh_predict_columns(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *off, const int32_t *idx,
                          const int32_t *milli, int64_t m, double query_weight, double user_weight, double default_mean,
                          int32_t sum_order, int32_t *out, uint32_t *flags_out, void *stream);

/* ---- serving new queries: a band-key index of a finished run, probed many times ---------------------------------
 * The neighbours a query x that was NOT in the indexed set gets (LSH.get_candidates, lsh.py:40-55, and
 * recommender.py:187-214 for x appended alone, K held fixed): its candidates are the indexed ids that share with x a
 * band whose r = P / b values are equal after the int16 cast and not all -1 (65535 counts as -1); each once, however
 * many bands it shares.  Score: milli = rint(1000 * dot / (sqrt(na) * sqrt(nb))), qrlsh_score_pairs bit for bit.
 * List: the K best candidates by milli descending, then id ascending.  New queries of one probe never see each other,
 * so a query's result does not depend on the batch around it; they become visible to later probes through append.
 *   build: keys [b][n] (band keys of the n indexed queries: qrlsh_band_keys / qrlsh_minhash keys_out, or the
 *     caller's own -- keys only filter, every candidate is checked against the rows) are sorted in place per band with
 *     their ids (ids [b][n] uint32 output; keys_tmp / ids_tmp scratch of the same size; qrlsh_sort_u64 over the top
 *     32 bits of mix64(key), workspace qrlsh_index_build_workspace_bytes) and dir_out (qrlsh_index_dir_words uint32)
 *     receives a per-band directory over the top qrlsh_index_dir_bits(n) bits of mix64(key).  n < 2^32 - 1.
 *   probe count / fill: probe_keys [b][m] of the new queries' signatures (same key rule as the index).  count
 *     leaves the number of raw candidate words in *total_out (device uint64) and per-(query, band) offsets in
 *     `workspace` (qrlsh_index_probe_workspace_bytes(m, b)); fill writes them: raw_out[*] = (q * b + band) << 32 | id,
 *     duplicates across bands included.  m * b < 2^32.
 *   finish: dedupe, verify and score the raw words against the rows (sig / norm2 of the index, probe_sig /
 *     probe_norm2 of the new queries, one sig_dtype for both; a norm may be NULL: summed from the rows), select and
 *     cut.  probe_workspace: the workspace count / fill used; workspace: qrlsh_index_finish_workspace_bytes(m, K,
 *     n_raw).  Outputs: off_out int64 [m+1] (CSR), idx_out / milli_out int32 [m * K] capacity (off_out[m] used),
 *     avail_out int32 [m] = number of distinct candidates before the cut.  1 <= K <= 256 (QRLSH_EINVAL otherwise).
 *     Lists of up to 4096 raw words are selected in one LDS image; longer ones (a popular key) stream through it,
 *     decided on the device.  Afterwards the first n_raw uint64 words of `workspace` hold, per raw word, its
 *     select key (1000 - milli) << 32 | id, or ~0 for a word dropped as a duplicate or a key collision: every
 *     candidate uncut (LSH.query reads them). */
int32_t qrlsh_index_dir_bits(int64_t n);
size_t qrlsh_index_dir_words(int64_t n, int32_t b);
size_t qrlsh_index_build_workspace_bytes(int64_t n, int32_t b);
int qrlsh_index_build(uint64_t *keys, uint64_t *keys_tmp, uint32_t *ids, uint32_t *ids_tmp, int64_t n, int32_t b,
                      uint32_t *dir_out, void *workspace, size_t workspace_bytes, void *stream);
size_t qrlsh_index_probe_workspace_bytes(int64_t m, int32_t b);
int qrlsh_index_probe_count(const uint64_t *sorted_keys, const uint32_t *dir, int64_t n, int32_t b, int32_t r,
                            const uint64_t *probe_keys, int64_t m, void *workspace, size_t workspace_bytes,
                            uint64_t *total_out, void *stream);
int qrlsh_index_probe_fill(const uint64_t *sorted_keys, const uint32_t *sorted_ids, const uint32_t *dir, int64_t n,
                           int32_t b, int32_t r, const uint64_t *probe_keys, int64_t m, const void *workspace,
                           size_t workspace_bytes, uint64_t *raw_out, void *stream);
size_t qrlsh_index_finish_workspace_bytes(int64_t m, int32_t K, int64_t n_raw);
int qrlsh_index_probe_finish(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig,
                             const int64_t *probe_norm2, int32_t sig_dtype, int32_t P, int32_t b, int64_t m,
                             const void *probe_workspace, const uint64_t *raw, int64_t n_raw, int32_t K,
                             int64_t *off_out, int32_t *idx_out, int32_t *milli_out, int32_t *avail_out,
                             void *workspace, size_t workspace_bytes, void *stream);
/*   append: m new queries enter a built index without a rebuild.  keys / ids / dir: a built index of n queries
 *     (qrlsh_index_build's outputs, or an earlier append's; read only; may be NULL when n == 0); new_keys [b][m]: the
 *     band keys of the new queries (consumed: sorted in place).  keys_out [b][n + m], ids_out [b][n + m] and dir_out
 *     (qrlsh_index_dir_words(n + m, b)) receive the grown index, out of place (the band-major layout moves every band's
 *     base when n changes): the new queries get the ids n .. n + m - 1 in the order given, and the three arrays are byte
 *     for byte what qrlsh_index_build makes of the concatenated [b][n + m] keys (the batch is sorted as the build sorts
 *     it, then merged stably behind the old records of equal mix bits; the directory is written in the same pass).
 *     No allocation, no read-back.  n + m < 2^32 - 1.  m == 0 returns at once and writes nothing.  workspace:
 *     qrlsh_index_append_workspace_bytes(m, b). */
size_t qrlsh_index_append_workspace_bytes(int64_t m, int32_t b);
int qrlsh_index_append(const uint64_t *keys, const uint32_t *ids, const uint32_t *dir, int64_t n, int32_t b,
                       uint64_t *new_keys, int64_t m, uint64_t *keys_out, uint32_t *ids_out, uint32_t *dir_out,
                       void *workspace, size_t workspace_bytes, void *stream);
#define QRLSH_INDEX_MAX_K 256
/*   finish for probe rows that ARE indexed: qrlsh_index_probe_finish with one more argument, first_id: probe row q is
 *     indexed query first_id + q (0 <= first_id, first_id + m <= n; probe_sig = rows first_id .. of sig, or a copy).  A
 *     raw word that names the query itself is dropped like a duplicate -- select key ~0, not counted in avail_out --
 *     so a query is never in its own list; everything else is the plain finish (rows with identical signatures and
 *     different ids stay each other's neighbours, at 1000).  Probed against the index they are in, this gives the
 *     lists of a range of indexed queries: new queries of one appended batch do see each other. */
int qrlsh_index_probe_finish_indexed(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig,
                                     const int64_t *probe_norm2, int32_t sig_dtype, int32_t P, int32_t b, int64_t m,
                                     int64_t first_id, const void *probe_workspace, const uint64_t *raw, int64_t n_raw,
                                     int32_t K, int64_t *off_out, int32_t *idx_out, int32_t *milli_out,
                                     int32_t *avail_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- keeping the top-K lists current when queries are appended (csrc/lists.hip) ---------------------------------
 * Input: the lists of a run over queries 0 .. n-1 with list length K -- COO src / dst / val int32 [n_edges] as
 * qrlsh_topk_*_fill writes them: ordered by src, then value descending, then dst ascending, at most K per src, queries
 * without candidates absent -- and a batch of m queries n .. n+m-1 that was appended to the index (qrlsh_index_append)
 * and then probed against the GROWN index: raw [n_raw] from qrlsh_index_probe_fill, select_keys [n_raw] = the first
 * n_raw words qrlsh_index_probe_finish_indexed (first_id = n, the same K) leaves in its workspace, new_off [m + 1] /
 * new_idx / new_milli its lists.  Output: src_out / dst_out / val_out, element for element the lists of a run over all
 * n + m queries with the same K and b:
 *   old row i < n:  the first K of the merge (value descending, then id ascending) of its stored row and its new
 *     neighbours (milli, n + x) for every kept raw word of probe query x that names i; a new id is larger than every
 *     old id and loses ties; a row that did not exist may appear;
 *   new row n + x:  the finish's list of x.
 * K is held fixed: a stored row was cut at K, so the result is that of a run with the SAME K over the n + m queries, not
 * with the K a fresh run would default to.  (The list length is changed on purpose with qrlsh_lists_cut_* and
 * qrlsh_lists_regrow_mark below: a cut row is regrown by probing it again against the index.)  Splitting a batch into successive appends-with-update
 * gives the same lists; n = 0 (from empty lists), m > n and m = 0 (the stored lists, unchanged) are served.
 * count: the reverse records (one per kept raw word with id < n: id << 11 | (1000 - milli), payload x) are sorted with
 *   qrlsh_sort_u64 over bits [0, 11 + bits(n)), rows get their stored and reverse extents, a scan their output offsets;
 *   *total_out (device uint64; the one read-back) = the number of output entries -- or ~0 when the stored lists break
 *   the contract in a way the kernels see (src not ascending, src or dst outside [0, n)); nothing may be filled then.
 * fill: follows a count on the same workspace and arguments; writes exactly `total` entries.  Every stored entry and
 *   every record ranks itself (place in its own sequence + a binary search in the other); no row is walked serially.
 * No allocation, one stream.  Limits: 1 <= K <= QRLSH_INDEX_MAX_K, n + m < 2^31, n_edges < 2^31, n_raw < 2^32,
 * m * b < 2^32 per call (QRLSH_EINVAL otherwise).  workspace: qrlsh_lists_update_workspace_bytes(n, m, n_edges, n_raw)
 * (two record + payload buffers of n_raw, 24 bytes per row, the sort's workspace). */
size_t qrlsh_lists_update_workspace_bytes(int64_t n, int64_t m, int64_t n_edges, int64_t n_raw);
int qrlsh_lists_update_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                             int64_t m, int32_t b, int32_t K, const uint64_t *raw, const uint64_t *select_keys,
                             int64_t n_raw, const int64_t *new_off, void *workspace, size_t workspace_bytes,
                             uint64_t *total_out, void *stream);
int qrlsh_lists_update_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                            int64_t m, int32_t b, int32_t K, int64_t n_raw, const int64_t *new_off,
                            const int32_t *new_idx, const int32_t *new_milli, const void *workspace,
                            size_t workspace_bytes, int64_t total, int32_t *src_out, int32_t *dst_out, int32_t *val_out,
                            void *stream);

/*   finish for probe rows scattered over the index: qrlsh_index_probe_finish_indexed with self_ids (device uint32 [m]) in
 *     the place of first_id: probe row q is indexed query self_ids[q].  A raw word that names the row itself is dropped
 *     like a duplicate; rows with identical signatures and different ids stay neighbours at 1000. */
int qrlsh_index_probe_finish_rows(const void *sig, const int64_t *norm2, int64_t n, const void *probe_sig,
                                  const int64_t *probe_norm2, int32_t sig_dtype, int32_t P, int32_t b, int64_t m,
                                  const uint32_t *self_ids, const void *probe_workspace, const uint64_t *raw, int64_t n_raw,
                                  int32_t K, int64_t *off_out, int32_t *idx_out, int32_t *milli_out, int32_t *avail_out,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- removing queries from a built index (csrc/remove.hip) ------------------------------------------------------
 * A set R of ids leaves 0 .. n-1 and the survivors are renumbered by rank: new id = old id - |{r in R : r < old id}|.
 * The map is monotone, so every order the index and the lists keep among ids is kept, and ids stay dense.
 *   id map: a set of ids over [0, n) with O(1) membership and rank: one 8-byte entry {32 bits, members below the word}
 *     per 32 ids, in caller memory of qrlsh_idmap_workspace_bytes(n) bytes (entries, then scratch of the build).
 *     build: ids uint32 [m] in any order, duplicates allowed; out2 (device uint64 [2]) receives {the number of distinct
 *     ids, a flag word: bit 0 = an id >= n was seen -- the map is then not to be used}: the one read-back that sizes
 *     what follows.  list: the members in ascending order (uint32 [count]).  positions: pos_out int64 [n], the new id
 *     of every old id, -1 for a member.  n < 2^32 - 1.
 *   rows: rows [n] of row_bytes (both arrays 16-byte aligned) and norm2 [n] (or NULL) -> rows_out / norm2_out [n - |R|],
 *     out of place: survivor i goes to row i - rank(i).  A row whose width is a multiple of 16 bytes -- every width the
 *     hot path makes at P a multiple of 8 -- is moved as 16-byte vectors; any other even width (P = 180 compact rows:
 *     360 bytes) as the widest of 8, 4 or 2 bytes that divides it.  An odd row_bytes is QRLSH_EINVAL.
 *   index: keys / ids [b][n] of a built index -> keys_out / ids_out [b][n - n_removed] and dir_out
 *     (qrlsh_index_dir_words(n - n_removed, b)), byte for byte qrlsh_index_build of the survivors' keys in their order:
 *     one stable compaction per band (count per tile of 2048 records, one scan, fill), ids remapped, then the directory
 *     kernel of the build over the output.  Keys are read once, ids twice, every output written once; no read-back.
 *     n_removed = the map's member count (out2[0]).  pick_map / n_pick / pick_keys_out [b][n_pick] (optional: NULL, 0,
 *     NULL): a second id map over OLD ids; the key of every surviving record whose id is in it is also written to
 *     pick_keys_out[band][rank_pick(id)] -- the probe keys of those rows, in qrlsh_idmap_list order, taken from the
 *     index itself (so an index built on caller keys behaves the same).  n_removed == 0 returns at once and writes
 *     nothing; n_removed == n writes nothing and succeeds (the caller holds the empty index).  workspace:
 *     qrlsh_index_remove_workspace_bytes(n, b).
 *   lists: src / dst / val as qrlsh_lists_update_* take them, list length K.  A stored row with fewer than K entries
 *     was never cut and holds every candidate of its query: it loses its removed entries and is renumbered.  A
 *     surviving row of exactly K entries that loses at least one may need candidates the cut threw away:
 *     mark: every such row enters pick_map_out (an id map over old ids, qrlsh_idmap_workspace_bytes(n) bytes); out2
 *       (device uint64 [2]) = {picked rows, 0 -- or ~0 when the stored lists break the contract (src not ascending, an
 *       id outside [0, n)); nothing may follow then}.
 *     The caller probes the picked rows against the SHRUNK index (pick_keys_out, qrlsh_index_probe_*,
 *     qrlsh_index_probe_finish_rows with their new ids, the same K): re_off int64 [n_pick + 1] / re_idx / re_milli,
 *     rows in qrlsh_idmap_list order; re_self uint32 [n_pick] = their new ids.
 *     count / fill: src_out / dst_out / val_out ordered by new src: an unpicked surviving row becomes its surviving
 *       entries, remapped, in stored order; a picked row its re-probed list; rows of removed queries and rows left
 *       empty are absent.  *total_out (device uint64; the one read-back) = the number of entries, or ~0 on a contract
 *       break.  fill follows a count on the same workspace and arguments and writes exactly `total` entries.  Stored
 *       entries are compacted like the bands (tiles of 2048, one scan); every entry places itself.
 * Limits: 1 <= K <= QRLSH_INDEX_MAX_K, n < 2^31 and n_edges < 2^31 with lists, n < 2^32 - 1 without (QRLSH_EINVAL
 * otherwise).  No allocation, one stream.  workspace: qrlsh_lists_remove_workspace_bytes(n, n_edges). */
size_t qrlsh_idmap_workspace_bytes(int64_t n);
int qrlsh_idmap_build(const uint32_t *ids, int64_t m, int64_t n, void *map, size_t map_bytes, uint64_t *out2, void *stream);
int qrlsh_idmap_list(const void *map, int64_t n, uint32_t *ids_out, void *stream);
int qrlsh_idmap_positions(const void *map, int64_t n, int64_t *pos_out, void *stream);
int qrlsh_rows_remove(const void *rows, int64_t row_bytes, const int64_t *norm2, int64_t n, const void *removed_map,
                      void *rows_out, int64_t *norm2_out, void *stream);
size_t qrlsh_index_remove_workspace_bytes(int64_t n, int32_t b);
int qrlsh_index_remove(const uint64_t *keys, const uint32_t *ids, int64_t n, int32_t b, const void *removed_map,
                       int64_t n_removed, const void *pick_map, int64_t n_pick, uint64_t *keys_out, uint32_t *ids_out,
                       uint32_t *dir_out, uint64_t *pick_keys_out, void *workspace, size_t workspace_bytes, void *stream);
size_t qrlsh_lists_remove_workspace_bytes(int64_t n, int64_t n_edges);
int qrlsh_lists_remove_mark(const int32_t *src, const int32_t *dst, int64_t n_edges, int64_t n, int32_t K,
                            const void *removed_map, void *pick_map_out, uint64_t *out2, void *stream);
int qrlsh_lists_remove_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                             int32_t K, const void *removed_map, const void *pick_map, const int64_t *re_off,
                             int64_t n_pick, void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream);
int qrlsh_lists_remove_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                            int32_t K, const void *removed_map, const void *pick_map, const int64_t *re_off,
                            const int32_t *re_idx, const int32_t *re_milli, const uint32_t *re_self, int64_t n_pick,
                            void *workspace, size_t workspace_bytes, int64_t total, int32_t *src_out, int32_t *dst_out,
                            int32_t *val_out, void *stream);

/* ---- changing the list length of stored lists (csrc/listcut.hip) -------------------------------------------------
 * Stored lists at list length K_old become, element for element, the lists of a run over the same rows at K_new.
 *   cut (K_new < K_old): the first K_new entries of a stored row are the row a run with K_new would have stored, so
 *     entry i survives exactly when i < K_new or src[i - K_new] != src[i]: a stream compaction with a predicate on src
 *     alone.  count: one workgroup per tile of 2048 entries reads src (16-byte loads; the predicate looks back across
 *     the tile's start through a halo in LDS), one scan follows; *total_out (device uint64; the one read-back) = the
 *     surviving entries -- or ~0 when the stored lists break the contract (src not ascending or outside [0, n), a row
 *     longer than K_old); nothing may be filled then.  K_new >= K_old keeps every entry (the total is n_edges).
 *     fill follows a count on the same workspace and arguments: src again, dst / val (16-byte loads) of the vectors that
 *     hold a survivor, every output written once; exactly `total` entries.  No atomic on a shared cursor, no serial walk
 *     of a row, no scratch.  src / dst / val must be 16-byte aligned.  A null or short workspace is QRLSH_EINVAL.
 *     workspace: qrlsh_lists_cut_workspace_bytes(n_edges).
 *   regrow (K_new > K_old): a stored row with fewer than K_old entries was never cut and is already its list at K_new;
 *     a row of exactly K_old entries may be missing candidates and is probed again against the unchanged index.
 *     mark: entry i is the head of such a row iff it is a run head and src[i + K_old - 1] == src[i]; the rows enter
 *       pick_map_out (qrlsh_idmap_workspace_bytes(n) bytes); out2 (device uint64 [2]) = {picked rows, 0 -- or ~0 on a
 *       contract break as above; nothing may follow then}.
 *     pick keys: the key of every record of keys / ids [b][n] whose id is in pick_map goes to
 *       pick_keys_out[band][rank_pick(id)] -- the probe keys of the picked rows in qrlsh_idmap_list order, from the
 *       index itself (an index built on caller keys behaves the same); what qrlsh_index_remove writes on its way,
 *       without a removal.  n_pick == 0 returns at once.
 *     The caller probes the picked rows (qrlsh_index_probe_*, qrlsh_index_probe_finish_rows with K_new) and puts the
 *     probed lists in their place with qrlsh_lists_remove_count / _fill over an EMPTY removed map (a zeroed
 *     qrlsh_idmap_workspace_bytes(n) buffer) and K = K_new: unpicked rows are copied as stored, picked rows take their
 *     probed lists.
 * Limits: 1 <= K_old, K_new <= QRLSH_INDEX_MAX_K, n < 2^31, n_edges < 2^31.  No allocation, one stream. */
size_t qrlsh_lists_cut_workspace_bytes(int64_t n_edges);
int qrlsh_lists_cut_count(const int32_t *src, int64_t n_edges, int64_t n, int32_t K_old, int32_t K_new, void *workspace,
                          size_t workspace_bytes, uint64_t *total_out, void *stream);
int qrlsh_lists_cut_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                         int32_t K_old, int32_t K_new, const void *workspace, size_t workspace_bytes, int64_t total,
                         int32_t *src_out, int32_t *dst_out, int32_t *val_out, void *stream);
int qrlsh_lists_regrow_mark(const int32_t *src, int64_t n_edges, int64_t n, int32_t K_old, void *pick_map_out,
                            uint64_t *out2, void *stream);
int qrlsh_index_pick_keys(const uint64_t *keys, const uint32_t *ids, int64_t n, int32_t b, const void *pick_map,
                          int64_t n_pick, uint64_t *pick_keys_out, void *stream);

/* ---- replacing queries of a built index in place (csrc/replace.hip; the lists: the merge of csrc/lists.hip) -------------
 * m distinct ids R of 0 .. n-1 get new rows: batch row x goes to id replaced_ids[x] (device uint32 [m], ASCENDING;
 * replaced_map = qrlsh_idmap_build over them, whose member count must be m).  n, b, qrlsh_index_dir_bits(n) and every
 * other id stay as they are.  Afterwards the arrays are byte for byte those of qrlsh_index_build over the key matrix with
 * columns R overwritten, and the lists element for element those of a run over the row matrix with rows R overwritten.
 *   rows: new_rows [m] of row_bytes and new_norm2 [m] overwrite rows / norm2 at replaced_ids[x], in place; 16-byte
 *     vectors, or the widest of 8, 4 or 2 bytes that divides row_bytes, as qrlsh_rows_remove.
 *   index: keys / ids / dir of the built index, new_keys [b][m] of the batch (consumed: sorted in place) -> keys_out /
 *     ids_out [b][n], dir_out.  A band's order is "top 32 bits of mix64(key), then id ascending": the new band is the old
 *     one without the records of R merged with the sorted batch by (mix bits, id), so a new record goes among the
 *     equal-bit records by its id.  Sort of the batch (bits 32..64, payload = batch index = id order); count per tile of
 *     2048 records (ids read, one map load each), which also lists the (mix bits, id) of the records that leave, sorted
 *     on their bits; a scan; rank: one lane per sorted batch record j finds the old records before it (old directory + a
 *     binary search on (bits, id)) and the leaving ones among them (a search in that list): s_j survivors precede it and
 *     it lands at s_j + j; fill: every surviving record ranks itself in its tile with ballots and goes to
 *     s + #{j : s_j <= s} (the batch range narrowed once per tile; a tile without batch records is a shifted copy); then
 *     the directory kernel of the build.  Keys are read once and written once, ids read twice.  pick_map / n_pick /
 *     pick_keys_out as qrlsh_index_remove.  m == 0 returns at once and writes nothing; m == n is served.  workspace:
 *     qrlsh_index_replace_workspace_bytes(n, m, b).
 *   lists: stored src / dst / val at list length K.  The rows to probe again are those of qrlsh_lists_remove_mark over
 *     replaced_map: rows outside R with exactly K entries, at least one of them in R (pick_map; pick_ids = its
 *     qrlsh_idmap_list).  The caller probes the batch against the NEW index with the new rows (raw / select_keys of
 *     qrlsh_index_probe_fill / qrlsh_index_probe_finish_rows, self ids replaced_ids, m * b < 2^32: r_off / r_idx /
 *     r_milli) and the picked rows with pick_keys_out (p_off / p_idx / p_milli; may be NULL when n_pick == 0).
 *     An unpicked row outside R becomes the first K of the merge of its stored entries whose dst is outside R with the
 *     replaced queries that name it (every kept raw word), by value descending, then id ascending -- ties go by id both
 *     ways; rows of R and picked rows take the finish's lists.  count leaves the number of entries in *total_out
 *     (device uint64; the one read-back), or ~0 when the stored lists break the contract (src not ascending, an id
 *     outside [0, n)); fill follows a count on the same workspace and arguments and writes exactly `total` entries;
 *     every stored entry and every reverse record ranks itself.  workspace: qrlsh_lists_replace_workspace_bytes.
 * Limits as for the removal.  No allocation, one stream, no fallback path. */
int qrlsh_rows_replace(void *rows, int64_t row_bytes, int64_t *norm2, int64_t n, const uint32_t *replaced_ids,
                       const void *new_rows, const int64_t *new_norm2, int64_t m, void *stream);
size_t qrlsh_index_replace_workspace_bytes(int64_t n, int64_t m, int32_t b);
int qrlsh_index_replace(const uint64_t *keys, const uint32_t *ids, const uint32_t *dir, int64_t n, int32_t b,
                        const void *replaced_map, const uint32_t *replaced_ids, uint64_t *new_keys, int64_t m,
                        const void *pick_map, int64_t n_pick, uint64_t *keys_out, uint32_t *ids_out, uint32_t *dir_out,
                        uint64_t *pick_keys_out, void *workspace, size_t workspace_bytes, void *stream);
size_t qrlsh_lists_replace_workspace_bytes(int64_t n, int64_t n_edges, int64_t n_raw);
int qrlsh_lists_replace_count(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                              int64_t m, int32_t b, int32_t K, const void *replaced_map, const uint32_t *replaced_ids,
                              const void *pick_map, const uint32_t *pick_ids, int64_t n_pick, const uint64_t *raw,
                              const uint64_t *select_keys, int64_t n_raw, const int64_t *r_off, const int64_t *p_off,
                              void *workspace, size_t workspace_bytes, uint64_t *total_out, void *stream);
int qrlsh_lists_replace_fill(const int32_t *src, const int32_t *dst, const int32_t *val, int64_t n_edges, int64_t n,
                             int64_t m, int32_t b, int32_t K, const void *replaced_map, const uint32_t *replaced_ids,
                             const void *pick_map, const uint32_t *pick_ids, int64_t n_pick, int64_t n_raw,
                             const int64_t *r_off, const int32_t *r_idx, const int32_t *r_milli, const int64_t *p_off,
                             const int32_t *p_idx, const int32_t *p_milli, const void *workspace, size_t workspace_bytes,
                             int64_t total, int32_t *src_out, int32_t *dst_out, int32_t *val_out, void *stream);

/* ---- recommendations: top-k unrated queries per user (the consumer of N1's output) ---------------------
 * Replaces the selection of the interactive prompt, recommender.py:357-375 (just_scored of :361, the argsort of
 * :370), in batch form over the completed matrix.  ratings / pred int32 [nu][nq] (qrlsh_predict's input and output),
 * both base pointers 16-byte aligned.  users[m] (int32 row ids), or NULL for all nu rows in order (then m = nu).
 * For each requested user u: eligible = { j : ratings[u][j] == 0 and pred[u][j] != 0 } (negative values included),
 * avail_out[i] = |eligible|, idx_out[i][0 .. min(k, avail) - 1] = the eligible columns with the largest pred, ordered
 * by value descending then column ascending, val_out[i][.] their values; unused slots idx -1 / val 0.  The result
 * is exact and depends on neither the form nor `slices` nor `lo`.
 * A user id outside [0, nu) is not read: its row gets avail_out = -1 and a padded output (the host reads it back).
 * Forms (qrlsh_recommend_workspace_bytes(m, nq, k, slices) bytes of workspace; 0 = none needed):
 *   rows form (nq <= 2048, slices = 0): one workgroup per row sorts the row's eligible cells in LDS; no workspace;
 *   slice form: (row, slice) workgroups, slices = 1 .. 256 (0 = auto: about 2048 workgroups, >= 8192 columns per
 *     slice).  An LDS histogram of the values over the window [lo, lo + 4096) finds the k-th largest value; when it
 *     falls outside the window (wide-range values) up to three radix rounds (12 / 12 / 8 bits of the biased key)
 *     find it, decided on the device; then one sweep emits the <= k winners and a per-row sort orders them.
 * Limits: 1 <= k <= QRLSH_RECOMMEND_MAX_K, nq < 2^31 (QRLSH_EINVAL otherwise); m x max(slices, 1) <= 2^24
 * workgroups (QRLSH_EUNSUPPORTED above).  m = 0 returns at once; nq = 0 gives avail 0 and padded rows.
 */
#define QRLSH_RECOMMEND_MAX_K 1024
size_t qrlsh_recommend_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices);
int qrlsh_recommend_topk(const int32_t *ratings, const int32_t *pred, int64_t nu, int64_t nq, const int32_t *users,
                         int64_t m, int32_t k, int32_t lo, int32_t slices, int32_t *idx_out, int32_t *val_out,
                         int32_t *avail_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- serving chosen users: their rows and their top-k from the live lists, no [nu][nq] prediction matrix ----------
 * "What do I show user u now?" needs the user's own row, the rows of its <= 64 neighbour users and the query lists:
 * qrlsh_predict_users computes qrlsh_predict's cells for the requested rows only, qrlsh_recommend_users selects from
 * them as qrlsh_recommend_topk would from the completed matrix.  Same arithmetic as qrlsh_predict (float64, no FMA,
 * half to even, both sum orders) cell for cell.
 * ratings int32 [nu][nq].  Query lists in CSR with integer milli values, as qrlsh_topk_* / a QueryIndex's lists hold
 * them: q_off int64 [nq + 1], q_idx int32, q_milli int32; the similarity is (double)milli / 1000.0, a true division
 * (8 bytes per entry; no transposed copy is made).  User lists u_idx / u_val [nu][ku] as qrlsh_predict takes them,
 * for ALL nu users, indexed by the requested user's id.  users int32 [m]: any order, repeats allowed; NULL = all rows
 * in order (then m = nu).
 * qrlsh_predict_users: out int32 [m][nq] = the completed rows (the rating where rated, else the prediction): rows
 * users[.] of qrlsh_predict's output.  qrlsh_predict_users_workspace_bytes is 0 (the lists are read where they are;
 * workspace may be NULL).
 * qrlsh_recommend_users: writes the rows in eligible mode (0 where rated, else the prediction; row stride rounded up to
 * 16 bytes) into its workspace (qrlsh_recommend_users_workspace_bytes(m, nq, k, slices), 16-byte aligned) and selects
 * from them; idx_out / val_out [m][k] and avail_out [m] under qrlsh_recommend_topk's contract (value descending, then
 * column ascending; padding -1 / 0; avail = eligible cells), `lo` and `slices` as there; the result depends on
 * neither, nor on the form.  A user id outside [0, nu) gives avail_out = -1 and a padded row.
 * One kernel sweeps (column slice, requested user) workgroups, the users of a slice together so that they share the
 * slice's lists in L2; per workgroup, decided on the device: the user's row staged in LDS as bytes (nq <= 131072 and
 * every value of the row in 0 .. 255), or read from memory.
 * *flags_out (device uint32, required) = 0, or bit 0: a query list longer than 64, bit 1: a list index outside
 * [0, nq), bit 2: a requested user id outside [0, nu).  Such lists are never walked (their cells get 0) and such rows
 * are never read (the row is all 0); the result is not to be used -- the caller reads the flags back.
 * Limits: ku <= 64, 1 <= k <= QRLSH_RECOMMEND_MAX_K, nq < 2^31, sum_order one of the two (QRLSH_EINVAL otherwise);
 * m <= 2^24 and m x max(slices, 1) <= 2^24 (QRLSH_EUNSUPPORTED above).  Every check precedes any device work.
 * m = 0 returns at once (nothing is written, *flags_out included); nq = 0 gives avail 0.  No allocation, one stream,
 * no read-back.
 */
size_t qrlsh_predict_users_workspace_bytes(int64_t m, int64_t nq);
int qrlsh_predict_users(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                        const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                        double query_weight, double user_weight, double default_mean, int32_t sum_order,
                        const int32_t *users, int64_t m, int32_t *out, uint32_t *flags_out, void *workspace,
                        size_t workspace_bytes, void *stream);
size_t qrlsh_recommend_users_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices);
int qrlsh_recommend_users(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                          const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                          double query_weight, double user_weight, double default_mean, int32_t sum_order,
                          const int32_t *users, int64_t m, int32_t k, int32_t lo, int32_t slices, int32_t *idx_out,
                          int32_t *val_out, int32_t *avail_out, uint32_t *flags_out, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ---- serving chosen queries: their columns, their top-k users and their utility from the live lists ----------------
 * The question the other way round: "whom do I show query j?" and "how useful is query j to the user base?", for
 * queries that ARE columns of the matrix (qrlsh_predict_columns covers new ones, whose user side is 0).  Same
 * arithmetic as qrlsh_predict cell for cell (float64, no FMA, half to even, both sum orders); no [nu][nq] prediction
 * matrix.  ratings, the query lists (CSR, milli) and the user lists u_idx / u_val [nu][ku] as qrlsh_predict_users
 * takes them.  u_idx entries >= 0 are TRUSTED to lie in [0, nu), exactly as qrlsh_predict_users trusts them.
 * queries int32 [m]: any order, repeats allowed; NULL = all nq columns in order (then m = nq).
 * cols_tmp int32 [m][nu] (required): caller-provided scratch of the same size as the output (the convention of
 * qrlsh_index_build's keys_tmp / ids_tmp; there is no size export).  It receives the raw columns ratings[.][queries[x]],
 * gathered once per call; the user side of every cell reads them, never cells this call has written.
 * qrlsh_predict_queries: out int32 [m][nu], query-major = the completed columns (the rating where rated, else the
 * prediction): columns queries[.] of qrlsh_predict's output, transposed.  out = NULL: only util_out is made.
 * qrlsh_recommend_queries: writes the columns in eligible mode (0 where rated; stride rounded up to 16 bytes) into its
 * workspace and selects from them with qrlsh_recommend_users' selection, the roles swapped: idx_out / val_out [m][k] =
 * per request the USERS with the largest predictions among the eligible cells of the column (unrated, prediction != 0),
 * value descending, then user ascending; padding -1 / 0; avail_out [m] = the eligible users, -1 for a query id outside
 * [0, nq) (its row padded).  `lo` and `slices` as qrlsh_recommend_topk takes them; the result depends on neither.
 * The workspace is qrlsh_recommend_users_workspace_bytes(m, nu, k, slices) bytes, 16-byte aligned: that call's layout
 * (compact rows, then the selection's own) with rows of length nu.
 * util_out int64 [m][8], zeroed by the caller (the words are ADDED: exact in any launch order), or NULL: per request
 *   [0] users who rated the query, [1] the sum of their ratings, [2] unrated users with a non-zero prediction, [3] the
 *   sum of those predictions, [4] unrated users with prediction 0 (missed), and the unrated users by the sides of the
 *   blend that are non-zero: [5] the query side alone, [6] the user side alone, [7] both (neither: counted in [4] only).
 *   A request outside [0, nq) adds nothing.
 * One gather kernel (nu strided reads per request), then one sweep of (user slice, request) workgroups, the requests of a
 * slice together; per workgroup, decided on the device: the compact column staged in LDS as bytes (nu <= 131072 and
 * every value in 0 .. 255), or read from memory.  The query side costs one memory transaction per (user, neighbour of
 * the query).
 * *flags_out (device uint32, required) = 0, or bit 0: a query list longer than 64, bit 1: a list index outside
 * [0, nq), bit 2: a requested query id outside [0, nq).  Such lists are never walked (the unrated cells get 0) and such
 * columns are never read (all 0); the result is not to be used -- the caller reads the flags back.
 * Limits: ku <= 64, 1 <= k <= QRLSH_RECOMMEND_MAX_K, nq < 2^31, nu < 2^31, sum_order one of the two (QRLSH_EINVAL
 * otherwise); m <= 2^24 and m x max(slices, 1) <= 2^24 (QRLSH_EUNSUPPORTED above).  Every check precedes any device
 * work.  m = 0 returns at once (nothing is written, *flags_out included); nu = 0 gives avail 0 and padded rows.  No
 * allocation, one stream, no read-back.
 */
int qrlsh_predict_queries(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                          const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                          double query_weight, double user_weight, double default_mean, int32_t sum_order,
                          const int32_t *queries, int64_t m, int32_t *out, int32_t *cols_tmp, int64_t *util_out,
                          uint32_t *flags_out, void *stream);
int qrlsh_recommend_queries(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                            const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                            double query_weight, double user_weight, double default_mean, int32_t sum_order,
                            const int32_t *queries, int64_t m, int32_t k, int32_t lo, int32_t slices, int32_t *idx_out,
                            int32_t *val_out, int32_t *avail_out, int64_t *util_out, uint32_t *flags_out,
                            int32_t *cols_tmp, void *workspace, size_t workspace_bytes, void *stream);

/* ---- diversified lists: rerank a served pool by the stored neighbour lists; the redundancy of a served list ----------
 * The project's own rule (the reference has no counterpart); integer arithmetic only.  Query lists in CSR with milli
 * values (0 .. 1000) as qrlsh_recommend_users takes them, rows of any length.
 *   sim(a, b) = the largest stored milli among the entries a -> b and b -> a; 0 when neither is stored.
 * qrlsh_diversify: cand_idx / cand_val int32 [m][N] and avail int32 [m] are rows of qrlsh_recommend_topk /
 * qrlsh_recommend_users output at k = N: request x has the pool of its first n = min(N, max(avail[x], 0)) candidates
 * in served order.  For t = 0 .. k - 1, over the unpicked candidates c: r_c = max over the picked s of sim(c, s) (0 while
 * nothing is picked); c is eligible when r_c < max_sim; score_c = 1000 * val_c - penalty * r_c (int64); the eligible c
 * with the largest score is picked, ties to the smaller pool position; the request ends early when nobody is eligible.
 * idx_out / val_out / red_out int32 [m][k]: the picks' columns, values and the r_c each had when taken, -1 / 0 / 0 past
 * the picks; count_out int32 [m]: the picks.  penalty = 0, max_sim = 1001 gives the first min(k, n) of the pool.
 * qrlsh_list_redundancy: idx int32 [m][k], entries of -1 are padding.  words_out int64 [m][4] per list: the entries
 * listed, the unordered in-list pairs with sim > 0, the sum of sim over them, the largest sim.  totals_out int64 [4]
 * (zeroed by the caller) gets the sums of the first three over the lists and the max of the last.
 * One 256-thread workgroup per request.  The pool's columns go into an LDS hash, the candidates' list rows are walked
 * and the pool-internal edges become, in both directions, a CSR over pool positions in the workspace (a half-edge is one
 * word: 10 bits of position, 10 of milli); the selection then keeps r and the picked bits in LDS and per step takes an
 * argmax over the workgroup and walks the pick's half-edges alone.  The workspace is divided evenly among the m
 * requests; qrlsh_diversify_workspace_bytes(m, N, max_row) holds every pool of N whose list rows are at most max_row
 * long and name no query twice (2 N min(max_row, N - 1) half-edges per request), for qrlsh_list_redundancy with N = k.
 * *flag_out (device uint32, zeroed by the caller, required) gets bit 0: a neighbour index outside [0, nq), bit 1: a
 * candidate column outside [0, nq) before avail (for a list: other than -1), bit 2: a column twice in one pool, bit 3:
 * a pool whose half-edges do not fit its share of the workspace (none of them is written).  A flagged result is not to
 * be used; nothing outside the arguments is read or written.
 * Limits: 1 <= k <= N <= QRLSH_DIVERSIFY_MAX_POOL, 0 <= penalty <= QRLSH_DIVERSIFY_MAX_PENALTY, 0 <= max_sim <= 1001
 * (1001: nothing is excluded), nq < 2^31 (QRLSH_EINVAL otherwise); m <= 2^24 (QRLSH_EUNSUPPORTED above); a workspace
 * below the offsets' m (N + 4) words gives QRLSH_EWORKSPACE.  m = 0 returns at once.  No allocation, one stream, no
 * read-back.
 */
#define QRLSH_DIVERSIFY_MAX_POOL 1024
#define QRLSH_DIVERSIFY_MAX_PENALTY (1 << 20)
size_t qrlsh_diversify_workspace_bytes(int64_t m, int32_t N, int64_t max_row);
int qrlsh_diversify(const int32_t *cand_idx, const int32_t *cand_val, const int32_t *avail, int64_t m, int32_t N,
                    int64_t nq, const int64_t *q_off, const int32_t *q_idx, const int32_t *q_milli, int32_t k,
                    int64_t penalty, int32_t max_sim, int32_t *idx_out, int32_t *val_out, int32_t *red_out,
                    int32_t *count_out, uint32_t *flag_out, void *workspace, size_t workspace_bytes, void *stream);
int qrlsh_list_redundancy(const int32_t *idx, int64_t m, int32_t k, int64_t nq, const int64_t *q_off,
                          const int32_t *q_idx, const int32_t *q_milli, int64_t *words_out, int64_t *totals_out,
                          uint32_t *flag_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- tuning the rerank: qrlsh_diversify under S settings over one adjacency, each list scored on the device ---------
 * qrlsh_diversify_grid applies qrlsh_diversify's rule, unchanged, to the same pools (cand_idx, cand_val, avail, m, N, k,
 * the lists in CSR) under S settings: penalties int64 [S] and max_sims int32 [S], device arrays read on the device.
 * Neither enters the adjacency, which is built ONCE per request (qrlsh_diversify's kernel and workspace:
 * qrlsh_diversify_workspace_bytes(m, N, max_row)); one 256-thread workgroup per (request, setting) then runs the greedy
 * loop (one copy of it serves both entry points), gathers the truth at the picks and folds the picks' half-edges of the
 * POOL's adjacency towards later-ranked picks -- a served list is a subset of its pool, so no second adjacency is built.
 * Scoring against held-out truth (truth == NULL switches it off): truth int32 [nu][nq]; users int32 [m] or NULL (request
 *   x is user x); a pick is a hit when truth[user][col] >= relevant (>= 1); gain int64 [k], gain_prefix int64 [k + 1] as
 *   qrlsh_evaluate_ranking takes them (a negative gain: flag bit 6); request_counts int64 [m][2] or NULL (zeros): the
 *   relevant test cells and the test cells of each request, words 5 and 6 of a qrlsh_evaluate_ranking line.
 * idx_out / val_out / red_out int32 [S][m][k], count_out int32 [S][m]: each NULL or, per setting, word for word what
 *   qrlsh_diversify writes for that setting.
 * per_request_out NULL or int64 [S][m][12]: 0 listed (the picks); 1 hits; 2 known (picks with truth != 0); 3 the 1-based
 *   rank of the first hit (0 = none); 4 dcg = the sum of gain[p] over the hit positions; 5 relevant test cells and 6 test
 *   cells (request_counts); 7 avail[x]; 8 the unordered in-list pairs with sim > 0; 9 the sum of sim over them; 10 the
 *   largest sim (8-10 = qrlsh_list_redundancy's words 1-3 over the setting's list; a pair stored in both directions counts
 *   once, at the larger milli); 11 the sum of red over the picks.  A request is not served when avail[x] < 0 or, with a
 *   truth, when its user is outside [0, nu) (flag bit 5): words 0-6 and 8-11 = 0, word 7 = avail[x], nothing added to the
 *   totals.
 * totals_out int64 [S][24], required, ADDED to (the caller zeroes it; request blocks accumulate on the device): words
 *   0-7 the column sums of words 0-7 over the requests served; 8 requests served; 9 requests with >= 1 relevant test
 *   cell; 10 requests with >= 1 hit; 11 the sum of gain_prefix[min(k, relevant test cells)] (0-11 = qrlsh_evaluate_ranking's
 *   totals over the diversified lists); 12 the sum of word 8; 13 of word 9; 14 the maximum of word 10; 15 the sum of word
 *   11; 16 requests whose list differs from the plain prefix of their pool (a pick at step t that is not pool position
 *   t, or fewer picks than min(k, n)); 17 requests that ended early (picks < min(k, n)); 18-23 = 0.  64-bit integer
 *   atomic adds and one atomic max: exact in any launch order.  Without a truth words 1-6, 9, 10 and 11 stay 0.
 * *flag_out as qrlsh_diversify (bits 0-3), and bit 4: a penalty outside 0 .. QRLSH_DIVERSIFY_MAX_PENALTY or a max_sim
 *   outside 0 .. 1001 (that setting's lines are all zero, its lists empty, nothing added to its totals), bit 5, bit 6.
 * Limits: qrlsh_diversify's (N, k, nq, m <= 2^24, the workspace), 1 <= S <= QRLSH_GRID_MAX_SETTINGS, and with a truth
 * nu < 2^31 and relevant >= 1; QRLSH_EINVAL / QRLSH_EUNSUPPORTED / QRLSH_EWORKSPACE before any device work.  m = 0
 * returns at once, the totals untouched.  No allocation, one stream, no read-back. */
int qrlsh_diversify_grid(const int32_t *cand_idx, const int32_t *cand_val, const int32_t *avail, int64_t m, int32_t N,
                         int64_t nq, const int64_t *q_off, const int32_t *q_idx, const int32_t *q_milli, int32_t k,
                         const int64_t *penalties, const int32_t *max_sims, int32_t S, const int32_t *truth, int64_t nu,
                         const int32_t *users, int32_t relevant, const int64_t *gain, const int64_t *gain_prefix,
                         const int64_t *request_counts, int32_t *idx_out, int32_t *val_out, int32_t *red_out,
                         int32_t *count_out, int64_t *per_request_out, int64_t *totals_out, uint32_t *flag_out,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- list fidelity: the exact answer-set overlap of the neighbour lists ---------------------------------------------
 * How many of a query's TRUE nearest neighbours does its served list hold?  True = Jaccard over the answer sets, the
 * quantity MinHash estimates.  offsets int64 [nq + 1] / rows int32: the CSR answer sets, rows ascending and distinct per
 * query (TRUSTED to be a CSR, as qrlsh_minhash trusts it after qrlsh_check_csr).  Integer arithmetic only:
 *   J(s, j) = inter / union with union = |A(s)| + |A(j)| - inter, and 0 when union == 0;
 *   J_a > J_b is decided by inter_a * union_b > inter_b * union_a in int64.
 * qrlsh_edge_overlaps: src / dst int32 [n], any edges (the COO of the live lists is the use in mind);
 *   inter_out int32 [n]: inter_out[e] = |A(src[e]) & A(dst[e])|.  src == dst gives |A|, two empty sets 0.  A group of 16
 *   lanes per edge walks the shorter set and binary-searches the longer one.  *flags_out (device uint32, zeroed by the
 *   caller, required) gets bit 0: an edge end outside [0, nq) (its inter_out is 0, nothing is gathered).  n = 0 returns at
 *   once; n <= 2^35 - 16 (QRLSH_EUNSUPPORTED above).
 * qrlsh_list_fidelity: the query lists in CSR as qrlsh_recommend_users takes them (q_off int64 [nq + 1], q_idx int32;
 *   the stored order is the order of the row, the values are not read).  queries int32 [m]: the chosen queries, any
 *   order, repeats allowed; NULL = queries 0 .. m - 1 (m <= nq).  Request x with chosen query s is held to its first
 *   L = min(row length, K) entries -- a prefix, the list a run with that K would have stored -- against ALL nq queries.
 *   Per stored entry e (target d_e), int32 [m][64], 0 past L:
 *     inter_out, union_out = of (s, d_e);  better_out = the j != s with J(s, j) > J_e;
 *     equal_out = the j != s, j != d_e with J(s, j) == J_e.      An entry that names s itself is scored like any other.
 *   words_out int64 [m][8]: 0 listed (L); 1 |A(s)|; 2 positives = the j != s with inter > 0; 3 hits = entries with
 *     better < K (in the exact top K under SOME tie-break); 4 sure = entries with better + equal < K (under EVERY
 *     tie-break); 5 reachable = min(K, positives); 6 disjoint = entries with inter == 0; 7 inversions = pairs of entries
 *     e before f in stored order with J_e < J_f.
 *   totals_out int64 [8], required, ADDED to (the caller zeroes it; request blocks accumulate on the device): the column
 *     sums of the words.  The five [m][.] outputs are written whole by every call.
 *   Four steps on one stream: the outputs zeroed; the intersection kernel of qrlsh_edge_overlaps over the chosen rows;
 *   the sweep -- a 1024-thread workgroup per (group of G requests, slice of the ids j) stages the G answer sets as one
 *   interleaved bitmap over the D table rows in LDS (G bits per row), the G x 64 stored (inter, union) and their
 *   counters beside it, reads the CSR rows of its slice ONCE for the whole group, one LDS read per row id, and takes
 *   only the (request, j) with inter > 0 and j != s on to the <= 64 comparisons -- and a finish that turns the counters
 *   into the words.  Counters leave a workgroup by integer atomic adds: exact in any launch order, the same for every
 *   slice count.  Nothing of size m x nq is written; there is no workspace.
 *   G = qrlsh_list_fidelity_group(D): the largest of 32, 16, 8, 4, 2, 1 with ceil(D G / 32) + 256 G + 128 words within
 *   the 160 KiB of LDS of a CU (0 for a D outside [0, 2^20]).  slices: 0 = automatic (about 1024 workgroups in all,
 *   slices of at least 4096 ids), else 1 .. 256.
 *   *flags_out (device uint32, zeroed by the caller, required): bit 0 a chosen query's list row is longer than 64 (not
 *   walked; that request's words and entries are 0), bit 1 a neighbour index outside [0, nq) among the first L (that
 *   entry's inter and union are 0, nothing is gathered), bit 2 a chosen query outside [0, nq) (all 0), bit 3 an
 *   answer-set row id outside [0, D) (never tested against LDS).  A flagged result is not to be used.
 *   Limits: 1 <= K <= QRLSH_FIDELITY_MAX_K, nq < 2^31, 0 <= D <= 2^20, 0 <= slices <= 256 (QRLSH_EINVAL otherwise); m <=
 *   2^24 (QRLSH_EUNSUPPORTED above).  Every check precedes any device work; m = 0 returns at once, the totals untouched.
 * No allocation, one stream, no read-back. */
#define QRLSH_FIDELITY_MAX_K 64
int32_t qrlsh_list_fidelity_group(int64_t D);
int qrlsh_edge_overlaps(const int64_t *offsets, const int32_t *rows, int64_t nq, const int32_t *src, const int32_t *dst,
                        int64_t n, int32_t *inter_out, uint32_t *flags_out, void *stream);
int qrlsh_list_fidelity(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t D, const int64_t *q_off,
                        const int32_t *q_idx, const int32_t *queries, int64_t m, int32_t K, int32_t slices,
                        int32_t *inter_out, int32_t *union_out, int32_t *better_out, int32_t *equal_out,
                        int64_t *words_out, int64_t *totals_out, uint32_t *flags_out, void *stream);

/* ---- exact lists: the top K by Jaccard over the answer sets, in the served list format -------------------------------
 * What qrlsh_list_fidelity holds the served lists to, produced.  offsets int64 [nq + 1] / rows int32: the CSR answer sets
 * over D table rows, rows ascending and distinct per query (TRUSTED to be a CSR, as above).  queries int32 [m]: the chosen
 * queries, any order, repeats allowed; NULL = queries 0 .. m - 1 (m <= nq).  J, and the comparison of two J, as above:
 * integers only, J_a > J_b decided by inter_a * union_b > inter_b * union_a in int64.
 * The result of request x with chosen query s: the j != s with |A(s) & A(j)| > 0, ordered by J(s, j) descending, ties by
 *   j ascending, cut at K.  That order is total, so the result is unique: it depends on neither the launch order nor the
 *   slice count.  A query that shares no row with s is never listed, however short the list.
 * Outputs, every word written by every call (nothing is accumulated):
 *   dst_out int32 [m][K]: the neighbours, padded with -1;  inter_out, union_out int32 [m][K]: of (s, dst), padded with 0;
 *   counts_out int32 [m][2] = (listed = min(K, positives), positives = the j != s with inter > 0).
 * *flags_out (device uint32, zeroed by the caller, required): bit 2 a chosen query outside [0, nq) (its row is all
 *   padding, its counts 0), bit 3 an answer-set row id outside [0, D) (never tested against LDS).  The bits are
 *   qrlsh_list_fidelity's; bits 0 and 1 are not used.  A flagged result is not to be used.
 * scratch: the partial lists of the slices, m * S * K * 3 int32 words with S = qrlsh_exact_neighbours_slices(nq, m, D,
 *   slices), the resolved slice count (0 for arguments the call would refuse): slices itself when it is not 0, else
 *   qrlsh_list_fidelity's automatic rule over ceil(m / G) workgroups per slice.  4-byte aligned; it need not be
 *   initialised and holds nothing afterwards.  QRLSH_EWORKSPACE when scratch_bytes is smaller.
 * Three steps on one stream: counts_out zeroed; the sweep -- qrlsh_list_fidelity's: a 1024-thread workgroup per (group of
 *   G = qrlsh_list_fidelity_group(D) requests, slice of the ids j), the G answer sets as one interleaved bitmap in LDS,
 *   the CSR rows of the slice read once for the whole group; the 256 words of a request hold its best K so far (inter,
 *   union, id, in order) and the K-th entry as a threshold word.  A (request, j) with inter > 0 is compared once, with
 *   the threshold; only one that may enter takes the request's LDS lock (a try-lock loop, the insertion and the release
 *   inside the successful branch) and is inserted.  Each (request, slice) leaves its K entries in the scratch; a finish
 *   with one wave per request merges the S partial lists under the same order and writes padding and counts.
 * Limits: qrlsh_list_fidelity's -- 1 <= K <= QRLSH_FIDELITY_MAX_K, nq < 2^31, 0 <= D <= 2^20, 0 <= slices <= 256
 *   (QRLSH_EINVAL otherwise); m <= 2^24 (QRLSH_EUNSUPPORTED above).  Every check precedes any device work; m = 0 or
 *   nq = 0 returns at once with nothing written.
 * No allocation, one stream, no read-back. */
int32_t qrlsh_exact_neighbours_slices(int64_t nq, int64_t m, int64_t D, int32_t slices);
int qrlsh_exact_neighbours(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t D, const int32_t *queries,
                           int64_t m, int32_t K, int32_t slices, int32_t *dst_out, int32_t *inter_out, int32_t *union_out,
                           int32_t *counts_out, uint32_t *flags_out, void *scratch, size_t scratch_bytes, void *stream);

/* ---- exact lists from postings: the same lists from a row -> queries index of the answer sets ---------------------------
 * qrlsh_answer_postings: the transpose of the CSR answer sets (offsets int64 [nq + 1], rows int32 [nnz], over D table
 *   rows).  p_off_out int64 [D + 1], p_qry_out int32 [nnz]: the queries whose answer set holds row d are
 *   p_qry[p_off[d] .. p_off[d + 1]), ascending.  The transpose is unique; every word of both outputs is written by every
 *   call (nnz = 0 or D = 0 still writes p_off).
 *   Four steps on one stream: a check of the offsets; one word row << 32 | query per CSR entry, in CSR order;
 *   qrlsh_sort_u64 over bits [32, 32 + bits(D)) -- stable, so the queries of a row stay ascending; p_qry from the low
 *   words and p_off[d] = the first sorted position whose row is >= d, a binary search per d.
 *   *flags_out (device uint32, zeroed by the caller, required): bit 3 a row id outside [0, D) (qrlsh_list_fidelity's bit;
 *   the entry is never used as an index: it is filed under row 0), bit 5 offsets is not a CSR over nnz entries (first != 0,
 *   last != nnz, or decreasing; every index stays inside the arrays all the same).  A flagged result is not to be used.
 *   scratch: qrlsh_answer_postings_scratch_bytes(nnz, D) bytes, 16-byte aligned -- two arrays of nnz 64-bit words and a
 *   qrlsh_sort_workspace_bytes(nnz, 1) behind them; 0 for nnz = 0 and for arguments the call would refuse.  It need not be
 *   initialised and holds nothing afterwards.  QRLSH_EWORKSPACE when scratch_bytes is smaller.
 *   Limits: nq < 2^31, 0 <= D <= 2^20, nnz >= 0 (QRLSH_EINVAL otherwise); nnz <= 2^32 - 1, what qrlsh_sort_u64 serves
 *   (QRLSH_EUNSUPPORTED above).  Every check precedes any device work.
 * qrlsh_exact_neighbours_postings: qrlsh_exact_neighbours' result, word for word, served from the postings.  offsets, rows,
 *   nq, D, queries, m, K, the four outputs and their padding, counts_out, the order (J descending by cross-multiplication in
 *   int64, ties by id ascending, cut at K), the limits and the return codes are qrlsh_exact_neighbours' above; there are
 *   no slices.  p_off int64 [D + 1] / p_qry int32 [offsets[nq]]: qrlsh_answer_postings of the same answer sets.
 *   One 1024-thread workgroup per request s with a = |A(s)| rows.  inter(s, j) is the number of the a posting lists that
 *   hold j and |A(j)| = offsets[j + 1] - offsets[j], so A(j) is never read: the work follows the request's matches.
 *   The ids are served in passes over disjoint windows that tile [0, nq) in ascending order.  A window is a pass when it
 *   holds at most C = qrlsh_exact_postings_pass_entries() list entries (counted exactly beforehand, by binary searches of
 *   its bounds in the a lists) or is a single id; the first cut is ceil(entries / C) windows of equal width, and a window
 *   that is no pass is halved from the same start until it is one.  A pass counts multiplicities in an LDS hash table of
 *   2 C slots (at most half full: at most C distinct ids, or one), then walks the slots: a candidate whose bound
 *   inter / a (union >= a) is below the K-th entry kept so far is dropped before anything is gathered; a survivor goes to
 *   an LDS queue by an atomic cursor, and between two workgroup barriers the queue is drained -- the exact union from two
 *   offsets, the comparison repeated, the kept list updated by one wave -- with the walk repeated for what the queue did
 *   not hold.  No lock and no wait of one thread on another; rows of s beyond the 512 whose list cursors stay in LDS are
 *   read from memory at every window.
 *   *flags_out (device uint32, zeroed by the caller, required): bit 2 a chosen query outside [0, nq) (its row is all
 *   padding, its counts 0), bit 3 a row id of a chosen query outside [0, D) (checked before it indexes p_off; that row is
 *   skipped), bit 4 the postings do not belong to these answer sets: p_off[0] != 0 or p_off[D] != offsets[nq], bounds of a
 *   list a request reads outside [0, offsets[nq]] or decreasing, or an entry of such a list outside [0, nq) (checked
 *   before it indexes offsets; never a candidate).  A flagged result is not to be used.
 *   WHAT BIT 4 DOES NOT SEE: postings built from OTHER answer sets of the same nq, nnz and D (a stale index: two
 *   queries of equal size swapped, sets replaced at the same total size) whose bounds and ids are all in range.  The
 *   intersections then come from the old lists and the unions from the new offsets: plausible numbers under no flag,
 *   for a request whose own set changed as for one whose neighbours changed.  Postings held across any change of the
 *   answer sets are the caller's responsibility.  (Every list a request s reads must hold s exactly once, and a count
 *   of those entries in the fill refuses a request whose own set changed; measured at 0.6 % of the kernel at 16 384
 *   requests, outside the parent's run-to-run spread, it is not built:
 *   profiles/exact_postings_self_check_parent_vs_branch.json.)
 *   Rows twice in one answer set are outside this route as they are outside qrlsh_exact_neighbours' contract (rows
 *   distinct per query); they are not detected: the list of such a row is read twice and its holders count double.
 *   qrlsh_exact_postings_list_cursors() = 512, the lists whose cursors stay in LDS, and qrlsh_exact_postings_queue() =
 *   1024, the survivors the queue holds between two drains, qrlsh_exact_postings_threads() = 1024, the threads of a
 *   request's workgroup (the lanes per list of the fill follow from it): exported, like C, for tests that build shapes
 *   around them.
 *   scratch: qrlsh_exact_postings_scratch_bytes(nq, m, K) bytes = 0: everything stays in LDS; the arguments are there for a
 *   form that needs some.  m = 0 or nq = 0 returns at once with nothing written; nothing of size m x nq is written or
 *   allocated.  Integer arithmetic only.
 * No allocation, one stream, no read-back. */
size_t qrlsh_answer_postings_scratch_bytes(int64_t nnz, int64_t D);
int qrlsh_answer_postings(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t nnz, int64_t D,
                          int64_t *p_off_out, int32_t *p_qry_out, uint32_t *flags_out, void *scratch, size_t scratch_bytes,
                          void *stream);
int32_t qrlsh_exact_postings_pass_entries(void);
int32_t qrlsh_exact_postings_list_cursors(void);
int32_t qrlsh_exact_postings_queue(void);
int32_t qrlsh_exact_postings_threads(void);
size_t qrlsh_exact_postings_scratch_bytes(int64_t nq, int64_t m, int32_t K);
int qrlsh_exact_neighbours_postings(const int64_t *offsets, const int32_t *rows, int64_t nq, int64_t D, const int64_t *p_off,
                                    const int32_t *p_qry, const int32_t *queries, int64_t m, int32_t K, int32_t *dst_out,
                                    int32_t *inter_out, int32_t *union_out, int32_t *counts_out, uint32_t *flags_out,
                                    void *scratch, size_t scratch_bytes, void *stream);

/* ---- evaluation: the prediction error on rated cells, hold-out and leave-one-out -----------------------------------
 * The blend of cell (i, j) never reads ratings[i][j]: a rated cell can be predicted as if it were unrated and compared
 * with its rating.  Predictions and ratings are integers, so every statistic is an exact integer sum, independent of the
 * launch order.  Arguments as qrlsh_predict_users takes them (lists in CSR with milli values, similarity = milli /
 * 1000.0; user lists u_idx / u_val [nu][ku]); same arithmetic cell for cell, both sum orders.
 * Sample rule: `keep` is a 64-bit word in [0, 2^32]; cell (i, j) is KEPT iff
 *     qr_mix64(seed ^ ((uint64)i << 32 | (uint32)j)) >> 32 < keep        (qrlsh_mix64_host is the host twin)
 * keep = 2^32 keeps every cell, 0 none; membership does not depend on nq (it survives column appends).
 * qrlsh_ratings_holdout: out int32 [nu][nq] = in with the kept non-zero cells set to 0 (out of place: in != out, `in` is
 *   not written); *count_out (device int64) = the cells zeroed.  A streaming kernel, 16-byte accesses where both
 *   pointers are 16-byte aligned.
 * qrlsh_evaluate: a cell is EVALUATED iff truth[i][j] != 0 and it is kept; its prediction is the blend computed from
 *   `ratings` exactly as if ratings[i][j] were 0 (the kernel does not read it: a list entry that names the cell's own
 *   column or row reads as 0); err = prediction - truth.  truth == ratings: leave-one-out with the lists held fixed;
 *   ratings = holdout(truth) under the same seed and keep: a hold-out.
 *   per_user_out int64 [nu][16], one 128-byte line per user: words 0-3, 4-7, 8-11 = n, sum err, sum |err|, sum err^2 of
 *   the cells predicted from the query side only, the user side only and both (the three non-zero branches of the
 *   blend); word 12 = evaluated cells whose prediction is 0 (missed: in none of the sums); word 13 = evaluated cells;
 *   words 14-15 = 0.  totals_out int64 [16] = its column sums.  pred_out: NULL, or int32 [nu][nq] = the prediction at
 *   evaluated cells (0 = missed), -1 elsewhere.
 *   One workgroup per (column slice, user): the user's row of `ratings` staged in LDS as bytes (nq <= 131072 and every
 *   value of the row in 0 .. 255) or read from memory; `truth` read coalesced; the evaluated cells of a slice are queued
 *   in LDS and predicted 1024 at a time, so a thin sample costs what its cells cost.  Per-slice sums go to the workspace
 *   (qrlsh_evaluate_workspace_bytes(nu, nq), 8-byte aligned) and two small kernels add them: no atomics.
 * qrlsh_evaluate_cells: an explicit test set of m triplets (cell_user, cell_query, cell_truth int32 [m]); every triplet
 *   is evaluated, repeats once each, whatever `ratings` holds there.  pred_out: NULL or int32 [m] (-1 for a triplet
 *   outside the matrix); totals_out int64 [16] as above (64-bit integer atomics).
 * *flags_out (device uint32, required) = 0, or bit 0: a query list longer than 64, bit 1: a list index outside [0, nq),
 *   bit 2 (cells form): a user or query id outside range.  Such lists are never walked or gathered and such cells never
 *   read; the result is not to be used.  A user-list entry >= nu is not gathered (its rating reads as 0).
 * Limits (QRLSH_EINVAL otherwise): ku <= 64, nq < 2^31, nu < 2^31, keep <= 2^32.  The sums are exact while |err| < 2^31
 * and they fit int64.  nu = 0 or nq = 0: all outputs 0.  No allocation, one stream, no read-back. */
int qrlsh_ratings_holdout(const int32_t *in, int64_t nu, int64_t nq, uint64_t seed, uint64_t keep, int32_t *out,
                          int64_t *count_out, void *stream);
size_t qrlsh_evaluate_workspace_bytes(int64_t nu, int64_t nq);
int qrlsh_evaluate(const int32_t *ratings, const int32_t *truth, int64_t nu, int64_t nq, const int64_t *q_off,
                   const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                   double query_weight, double user_weight, double default_mean, int32_t sum_order, uint64_t seed,
                   uint64_t keep, int64_t *per_user_out, int64_t *totals_out, int32_t *pred_out, uint32_t *flags_out,
                   void *workspace, size_t workspace_bytes, void *stream);
int qrlsh_evaluate_cells(const int32_t *ratings, int64_t nu, int64_t nq, const int64_t *q_off, const int32_t *q_idx,
                         const int32_t *q_milli, const int32_t *u_idx, const double *u_val, int32_t ku,
                         double query_weight, double user_weight, double default_mean, int32_t sum_order,
                         const int32_t *cell_user, const int32_t *cell_query, const int32_t *cell_truth, int64_t m,
                         int32_t *pred_out, int64_t *totals_out, uint32_t *flags_out, void *stream);

/* ---- tuning: qrlsh_evaluate's cells under a grid of list cuts and blend weights, in one sweep -----------------------
 * qrlsh_evaluate_grid evaluates the cells qrlsh_evaluate evaluates (truth != 0 and kept by the sample rule) under
 *     S = ncq x ncu x nw settings,    setting s = (cq * ncu + cu) * nw + w:
 * query lists cut at q_cuts[cq], user lists cut at u_cuts[cu], blended with weights[w] = (query_weight, user_weight,
 * default_mean).  Arguments up to `ku` and sum_order / seed / keep are qrlsh_evaluate's; q_cuts (device int32 [ncq]),
 * u_cuts (device int32 [ncu]) and weights (device double [nw][3]) are read on the device.
 * A cut c >= 0 means "the first min(len, c) entries of the list as stored": 0 switches that side off (the ablation
 *   "user side only" / "query side only"), c >= len is the whole list.  Every stored list is ordered score descending,
 *   ties by id ascending, so that prefix is the list a run with K = c would have stored: the figures under a cut are the
 *   figures of that run.  The two sides of a cell do not depend on the weights: a cell costs one query side per query cut
 *   and one user side per user cut (each with its own accumulation: the pairwise order depends on the length), and per
 *   setting only the blend, the rounding and the error.  The arithmetic is qrlsh_evaluate's, one copy of it; a list
 *   entry naming the cell's own column or row reads 0; both sum orders.
 * Output: 8 exact int64 words per setting.  totals_out int64 [S][8]; per_user_out NULL or int64 [nu][S][8]:
 *     word 0 = n, the cells with a non-zero prediction        word 4 = missed (prediction 0; in none of the sums)
 *     word 1 = sum err   (err = prediction - truth)           word 5 = cells evaluated (the same for every setting)
 *     word 2 = sum |err|                                      word 6 = n predicted from the query side only
 *     word 3 = sum err^2                                      word 7 = n predicted from the user side only
 *   In qrlsh_evaluate's 16 words e[]: word k = e[k] + e[4 + k] + e[8 + k] (k = 0 .. 3), word 4 = e[12], word 5 = e[13],
 *   word 6 = e[0], word 7 = e[4].  One setting with the whole lists gives qrlsh_evaluate's result through that mapping.
 * *flags_out (device uint32, required) = 0, or bit 0 / bit 1 exactly as qrlsh_evaluate raises them (a stored list longer
 *   than 64, a list index outside [0, nq) -- whatever the cuts), bit 3: a negative cut (it reads as 0).  A flagged result
 *   is not to be used; nothing is read out of bounds.
 * One workgroup per (column slice, user) as qrlsh_evaluate; the sums of a workgroup are kept in an LDS table [S][8] and
 * go to the workspace (qrlsh_evaluate_grid_workspace_bytes(nu, nq, S), 8-byte aligned), two small kernels add them: no
 * global atomics, the result does not depend on the launch order.
 * Limits (QRLSH_EINVAL otherwise, before any device work): 1 <= ncq, ncu <= QRLSH_GRID_MAX_CUTS, nw >= 1,
 * S <= QRLSH_GRID_MAX_SETTINGS, and qrlsh_evaluate's: ku <= 64, nq < 2^31, nu < 2^31, keep <= 2^32.  QRLSH_EWORKSPACE for
 * a workspace that is missing or short.  Exact under qrlsh_evaluate's conditions.  nu = 0 or nq = 0: all outputs 0 (the
 * cuts are still checked).  No allocation, one stream, no read-back. */
#define QRLSH_GRID_MAX_CUTS 4
#define QRLSH_GRID_MAX_SETTINGS 128
size_t qrlsh_evaluate_grid_workspace_bytes(int64_t nu, int64_t nq, int32_t settings);
int qrlsh_evaluate_grid(const int32_t *ratings, const int32_t *truth, int64_t nu, int64_t nq, const int64_t *q_off,
                        const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx, const double *u_val,
                        int32_t ku, const int32_t *q_cuts, int32_t ncq, const int32_t *u_cuts, int32_t ncu,
                        const double *weights, int32_t nw, int32_t sum_order, uint64_t seed, uint64_t keep,
                        int64_t *per_user_out, int64_t *totals_out, uint32_t *flags_out, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ---- ranking evaluation: precision, recall and NDCG at k of the served lists against held-out cells ---------------
 * Hold-out only (a rated cell is not ranked while it is rated).  `train` int32 [nu][nq] = the matrix with the test cells
 * zeroed, `truth` = the full matrix, same shape.  A TEST cell of user u: train[u][j] == 0 && truth[u][j] != 0; it is
 * RELEVANT when truth[u][j] >= relevant (int32 >= 1).  The list of request x is qrlsh_recommend_users(train, ...)'s: the
 * eligible cells (train == 0 and a non-zero prediction), value descending then column ascending, cut at k; a test cell
 * is 0 in `train`, so the serving arithmetic over `train` is its hold-out prediction.  Lists, weights, sum_order, users,
 * m, k, lo and slices as qrlsh_recommend_users takes them (slices > 0 also sets the sweep's column slices).
 * candidates: QRLSH_RANK_ALL -- every unrated cell of `train` is a candidate (the list the user would be shown; cells
 *   the truth does not rate count as not relevant, and `known` tells how many listed cells the truth rates);
 *   QRLSH_RANK_HELDOUT -- only the test cells are (a cell of `train` that `truth` does not rate is no candidate).
 * gain int64 [k], gain_prefix int64 [k + 1] (device; gain_prefix[n] = gain[0] + .. + gain[n - 1]): the caller's DCG
 *   gains per list position.  The library computes no logarithm; DCG is an exact integer.  Gains must be >= 0 (flag bit
 *   3 otherwise) and m x gain_prefix[k] must fit int64 (the caller's to ensure).
 * idx_out / val_out int32 [m][k], avail_out int32 [m]: the served lists, as qrlsh_recommend_users writes them.
 * per_user_out int64 [m][8], one 64-byte line per request: word 0 listed = min(k, avail); 1 hits = listed cells that
 *   are relevant; 2 known = listed cells the truth rates; 3 the 1-based rank of the first hit (0 = none); 4 dcg = the sum
 *   of gain[p] over the hit positions p; 5 relevant test cells of the user; 6 test cells of the user (both include cells
 *   whose prediction is 0: the model cannot reach them, recall must not forget them); 7 avail.  A request with a user id
 *   outside [0, nu): words 0-6 = 0, word 7 = avail = -1, nothing added to the totals, flag bit 2.
 * totals_out int64 [16]: words 0-7 = the column sums of the lines of the requests served; 8 = requests served; 9 =
 *   requests with >= 1 relevant test cell; 10 = requests with >= 1 hit; 11 = the sum of the ideal DCG
 *   gain_prefix[min(k, relevant test cells)]; 12-15 = 0.  64-bit integer atomics: exact in any order.
 * *flags_out (device uint32, required) = 0, or bits 0-2 as qrlsh_recommend_users raises them, bit 3: a negative gain.
 * workspace: qrlsh_evaluate_ranking_workspace_bytes(m, nq, k, slices) bytes, 16-byte aligned (0 for arguments outside
 *   the limits).  One sweep workgroup per (column slice, request) in qrlsh_predict_users' two row forms; with
 *   QRLSH_RANK_HELDOUT the test cells of a slice are queued in LDS and predicted 1024 at a time, so the work follows the
 *   test cells, not nq.
 * Limits: those of qrlsh_recommend_users (ku <= 64, lists <= 64, 1 <= k <= 1024, nq < 2^31, m <= 2^24), relevant >= 1,
 * candidates one of the two (QRLSH_EINVAL / QRLSH_EUNSUPPORTED / QRLSH_EWORKSPACE as there, all before any device work).
 * m = 0: totals and flags 0.  No allocation, one stream, no read-back. */
#define QRLSH_RANK_ALL 0
#define QRLSH_RANK_HELDOUT 1
size_t qrlsh_evaluate_ranking_workspace_bytes(int64_t m, int64_t nq, int32_t k, int32_t slices);
int qrlsh_evaluate_ranking(const int32_t *train, const int32_t *truth, int64_t nu, int64_t nq, const int64_t *q_off,
                           const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx, const double *u_val,
                           int32_t ku, double query_weight, double user_weight, double default_mean, int32_t sum_order,
                           const int32_t *users, int64_t m, int32_t k, int32_t relevant, int32_t candidates, int32_t lo,
                           int32_t slices, const int64_t *gain, const int64_t *gain_prefix, int32_t *idx_out,
                           int32_t *val_out, int32_t *avail_out, int64_t *per_user_out, int64_t *totals_out,
                           uint32_t *flags_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- tuning for the order of the list: qrlsh_evaluate_ranking's words under a grid of settings, in one sweep ---------
 * qrlsh_evaluate_ranking_grid computes, for every setting s = (cq * ncu + cu) * nw + w of qrlsh_evaluate_grid's grid
 * (query lists cut at q_cuts[cq], user lists cut at u_cuts[cu], blended with weights[w]; device arrays, read on the
 * device), the eight per-request words and the sixteen totals that qrlsh_evaluate_ranking(..., candidates =
 * QRLSH_RANK_HELDOUT) returns for that setting over lists cut on the host -- word for word.  train, truth, the lists,
 * ku, sum_order, users, m, k, relevant, gain and gain_prefix as qrlsh_evaluate_ranking takes them; the cuts and the
 * weights as qrlsh_evaluate_grid takes them.
 *   The list of (request x, setting s): the test cells of x whose prediction under s is not 0, prediction descending,
 *   then column ascending, cut at k.  Both sides of a test cell are computed once per cut (identical prefixes share one
 *   accumulation), never once per setting; per setting there is the blend, the rounding, an exact selection of the k-th
 *   largest prediction over the whole int32 range (weights may be negative or large: there is no value window) with ties
 *   resolved toward the lowest column, and the exact position of every listed relevant cell.  No list and no (nu, nq)
 *   matrix is written per setting.
 * per_request_out NULL or int64 [m][S][8]: listed = min(k, avail), hits, known (= listed in this mode), the 1-based rank
 *   of the first hit (0 = none), dcg, relevant test cells, test cells, avail.  A request with a user id outside [0, nu):
 *   zeros and avail -1, nothing added to the totals, flag bit 2.
 * totals_out int64 [S][16]: qrlsh_evaluate_ranking's totals per setting (12-15 = 0).  Added through the workspace by two
 *   small kernels: no global atomics, exact in any launch order.
 * cells: the capacity of the record arrays = an upper bound of the test cells of the m requests (a request named twice
 *   counts twice).  The library counts them first (one pass over the rows) and places every column slice's records by a
 *   scan of the counts, so the workspace follows the number of test cells, never nq x S.  *cells_out (device int64, may
 *   be NULL) = the count.  More test cells than `cells`: flag bit 4, nothing is written out of bounds, the result reads
 *   as if no request had a test cell and is not to be used.
 * *flags_out (device uint32, required) = 0, or bit 0 a stored list longer than 64, bit 1 a neighbour index outside
 *   [0, nq), bit 2 a user id outside [0, nu), bit 3 a negative gain or a negative cut (the cut reads as 0), bit 4 above.
 * workspace: qrlsh_evaluate_ranking_grid_workspace_bytes(m, nq, ncq, ncu, S, cells) bytes, 16-byte aligned (0 for
 *   arguments outside the limits): 8 + 8 (ncq + ncu) bytes per test cell, 64 bytes per (request, setting), and the
 *   slices' offsets.
 * Limits (QRLSH_EINVAL / QRLSH_EUNSUPPORTED / QRLSH_EWORKSPACE, all before any device work): 1 <= k <= 1024, ku <= 64,
 * lists <= 64 (flag), 1 <= ncq, ncu <= QRLSH_GRID_MAX_CUTS, nw >= 1, S <= QRLSH_GRID_MAX_SETTINGS, nq < 2^31,
 * m <= 2^24 and m x S < 2^31, relevant >= 1, m x gain_prefix[k] < 2^63 (the caller's to ensure); exact while every
 * |prediction| < 2^31.  m = 0: totals, *cells_out and flags 0.  Not here: QRLSH_RANK_ALL, the lists themselves, graded
 * relevance.  No allocation, one stream, no read-back. */
size_t qrlsh_evaluate_ranking_grid_workspace_bytes(int64_t m, int64_t nq, int32_t ncq, int32_t ncu, int32_t settings,
                                                   int64_t cells);
int qrlsh_evaluate_ranking_grid(const int32_t *train, const int32_t *truth, int64_t nu, int64_t nq, const int64_t *q_off,
                                const int32_t *q_idx, const int32_t *q_milli, const int32_t *u_idx, const double *u_val,
                                int32_t ku, const int32_t *q_cuts, int32_t ncq, const int32_t *u_cuts, int32_t ncu,
                                const double *weights, int32_t nw, int32_t sum_order, const int32_t *users, int64_t m,
                                int32_t k, int32_t relevant, const int64_t *gain, const int64_t *gain_prefix,
                                int64_t cells, int64_t *per_request_out, int64_t *totals_out, int64_t *cells_out,
                                uint32_t *flags_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- N4: user similarity, the part after the clustering ----------------------------------------
 * Recommender.compute_userSimilarities, recommender.py:263-288: inside a cluster every user's row is centred on
 * the mean of its non-zero ratings IN AN INTEGER ARRAY (the centred values are truncated toward zero), then
 * cosine of every pair of rows.  out[u][c] = ratings[u][c] == 0 ? 0 : (int)((double)ratings[u][c] - mean_u),
 * mean_u = (double)sum / (double)count over the non-zero ratings; row stride nq_stride >= nq (padding = 0).
 * The pairs of a cluster are qrlsh_bucket_pairs_emit on the labels (one band), their cosine qrlsh_score_pairs
 * on these rows, the per-user cut qrlsh_topk_select_* (qrlsh/users.py).  The clustering itself (:226-261) is
 * the reference's scikit-learn call and stays on the host.
 */
int qrlsh_center_rows(const int32_t *ratings, int64_t nu, int64_t nq, int64_t nq_stride, int32_t *out,
                      void *stream);

/* The clustering features of the same step (recommender.py:226-234: StandardScaler().fit_transform(ratings), then
 * PCA(min(r, c, 200)).fit(.).transform(.)) for a matrix with far more columns (queries) than rows (users): column
 * statistics as StandardScaler computes them (mean_out[nq]; inv_scale_out[nq] = 1 / scale, scale = sqrt(population
 * variance), 1 for constant columns) and the Gram matrix gram_out[nu][nu] = Z Z^T of the standardized matrix
 * Z = (ratings - mean) * inv_scale, in float64 on the matrix cores (v_mfma_f64_16x16x4_f64), the ratings read as
 * integers and standardized while they are staged (Z is never materialised), summed over column slices in a fixed
 * order (deterministic).  The PCA scores are U_k sqrt(lambda_k) of gram's eigen-decomposition (qrlsh/users.py).
 * workspace: qrlsh_user_gram_workspace_bytes(nu, nq) (the per-slice partial matrices). */
size_t qrlsh_user_gram_workspace_bytes(int64_t nu, int64_t nq);
int qrlsh_user_gram(const int32_t *ratings, int64_t nu, int64_t nq, double *mean_out, double *inv_scale_out,
                    double *gram_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- user lists that stay exact when users rate queries (csrc/userlists.hip) ----------------------------------------
 * After a batch of rating edits the user lists are element for element what qrlsh/users.py's user_similarities gives on
 * the edited matrix, with the cluster labels and K of the build held fixed.  Lists only name users of one cluster, so
 * the rows R that were edited touch their own clusters only.  Every entry point takes device pointers, allocates
 * nothing, works on one stream, and returns at once and writes nothing when its batch is empty (0 cells, rows, pairs).
 *   ratings_set: m cell edits ratings[users[i]][queries[i]] = values[i] (0 = unrate) into ratings int32 [nu][nq], in
 *     place.  The cells of one batch are distinct (the caller's duty).  *flag_out (device uint32): bit 0 = an id outside
 *     range was seen (that cell is not written); nothing is to be used then.
 *   rows_stats: for the m rows in `rows` (uint32 [m]; NULL = all nu rows, m == nu) mean[row] (float64: (double)sum /
 *     (double)count over the non-zero ratings, 0 without any -- qrlsh_center_rows' expression) and norm2[row] (int64: the
 *     squared norm of the truncated centred row), written at the row's own index.  One workgroup per row.
 *   pairs_score: pairs uint64 [n] = a << 32 | b (a, b < nu in any order, grouped by a) -> milli_out [n], what
 *     qrlsh_score_pairs gives on qrlsh_center_rows' output, bit for bit, computed from the raw ratings: an element is
 *     centred on the fly (x == 0 ? 0 : (int32_t)((double)x - mean)), the dot is exact in int64, cs = (na && nb) ?
 *     (double)dot / (sqrt((double)na) * sqrt((double)nb)) : 0, milli = (int32_t)rint(cs * 1000.0).  Grid = (column
 *     slice, tile of 8 consecutive pairs), slices of 256 .. 4096 columns chosen so that a handful of pairs fills the
 *     machine; a run of pairs with one first row centres that row's slice once (LDS) and streams the other rows past
 *     it.  16-byte loads on each address's own alignment, scalar head and tail: only `ratings` itself must be 16-byte
 *     aligned.  Partial dots go to workspace int64 [slices][n] (qrlsh_user_pairs_score_workspace_bytes(nq, n)); a
 *     finish kernel sums them (integers: no atomics, no memset).  No centred row is written to memory.
 *   cluster structure: label int32 [nu] dense in [0, nc); c_off int64 [nc + 1]; c_mem int32 [nu], members ascending
 *     within a cluster; c_pos int32 [nu], a user's place in its cluster.
 *   cluster_pairs: rows uint32 [s] ascending -> count: off_out int64 [s + 1] (exclusive scan of cluster size - 1; [s] =
 *     the number of pairs); fill: pairs_out[off[x] + j - (j > c_pos[rows[x]])] = rows[x] << 32 | member j, for every
 *     other member of rows[x]'s cluster in member order: the slot of a (row, member) is computable without a search.
 *   lists: dense, idx int32 [nu][K] (-1 past the end), milli int32 [nu][K] (0 past the end), len int32 [nu]; a row is
 *     ordered by value descending, then id ascending, and holds positive values only.
 *     mark: changed_map = qrlsh_idmap_build over R.  A row v outside R with len[v] == K and an entry in R enters
 *       pick_map_out (qrlsh_idmap_workspace_bytes(nu) bytes).  out3 (device uint64 [3]; the one read-back of the update)
 *       = {picked rows, 0 -- or ~0 when the lists break the contract (an idx outside [0, nu), a len outside [0, K]);
 *       nothing may follow then, the number of pairs of the picked rows (sum of cluster size - 1)}.
 *     apply (in place): S = R + picked, s = |S|; off / pair_milli = cluster_pairs_count over S ascending and the scores
 *       of cluster_pairs_fill's pairs.  A row of S becomes the first K, by (milli descending, id ascending), of its
 *       positive scored pairs; a row outside S of a touched cluster the first K of the merge of its stored entries whose
 *       idx is outside R with the positive (milli(r, v), r) of every r in R of its cluster (ties by id both ways); every
 *       other row keeps its bytes.  One wave per row; any cluster size (candidates are taken 64 at a time against the
 *       best K so far).
 * Limits (QRLSH_EINVAL otherwise): 1 <= K <= 64, nu < 2^31, nq < 2^31, n < 2^32. */
int qrlsh_ratings_set(int32_t *ratings, int64_t nu, int64_t nq, const uint32_t *users, const uint32_t *queries,
                      const int32_t *values, int64_t m, uint32_t *flag_out, void *stream);
int qrlsh_user_rows_stats(const int32_t *ratings, int64_t nu, int64_t nq, const uint32_t *rows, int64_t m, double *mean,
                          int64_t *norm2, void *stream);
size_t qrlsh_user_pairs_score_workspace_bytes(int64_t nq, int64_t n);
int qrlsh_user_pairs_score(const int32_t *ratings, int64_t nu, int64_t nq, const double *mean, const int64_t *norm2,
                           const uint64_t *pairs, int64_t n, int32_t *milli_out, void *workspace, size_t workspace_bytes,
                           void *stream);
int qrlsh_user_cluster_pairs_count(const uint32_t *rows, int64_t s, const int32_t *label, const int64_t *c_off, int64_t nu,
                                   int64_t nc, int64_t *off_out, void *stream);
int qrlsh_user_cluster_pairs_fill(const uint32_t *rows, int64_t s, const int32_t *label, const int64_t *c_off,
                                  const int32_t *c_mem, const int32_t *c_pos, int64_t nu, int64_t nc, const int64_t *off,
                                  uint64_t *pairs_out, void *stream);
int qrlsh_user_lists_mark(const int32_t *idx, const int32_t *len, int64_t nu, int32_t K, const void *changed_map,
                          const int32_t *label, const int64_t *c_off, int64_t nc, void *pick_map_out, uint64_t *out3,
                          void *stream);
int qrlsh_user_lists_apply(int32_t *idx, int32_t *milli, int32_t *len, int64_t nu, int32_t K, const void *changed_map,
                           const void *pick_map, int64_t s, const int32_t *label, const int64_t *c_off, const int32_t *c_mem,
                           const int32_t *c_pos, int64_t nc, const int64_t *off, const int32_t *pair_milli, int64_t n_pairs,
                           void *stream);

/* ---- the matrix of the user lists follows added, removed and re-rated queries (csrc/usercolumns.hip) -----------------
 * A column operation changes a user's centred row only where the user's old and new values in the affected columns
 * differ (the mean is over the non-zero ratings, zeros stay zero): those rows R take the place of the edited rows in
 * the update above, over the matrix in its new column space.  Device pointers, one stream, nothing allocated; both
 * return QRLSH_OK at once, whatever the pointers, when m == 0 or nu == 0.
 *   columns_changed: cols int32 [m] = the affected old column, or -1 for none (an appended column); block int32
 *     [nu][m] = the incoming values, NULL = all zero (a removal).  With old(u, k) = cols[k] >= 0 ? ratings[u][cols[k]]
 *     : 0 and new(u, k) = block ? block[u][k] : 0, row u enters changed_map_out (an id map over the nu rows,
 *     qrlsh_idmap_workspace_bytes(nu) bytes, ready for qrlsh_idmap_list and qrlsh_user_lists_mark) exactly when some k
 *     has old != new.  out2 (device uint64 [2]) = {rows in the map, 1 when a column lies outside [-1, nq): nothing is
 *     read for it}.  Repeated columns are harmless where block is NULL.  One lane per (row, k) cell.
 *   columns_move: out[u][j] = src[j] >= 0 ? in[u][src[j]] : block[u][~src[j]] for j < nq2; in int32 [nu][nq], block
 *     int32 [nu][m] (NULL = all zero), out a fresh contiguous int32 [nu][nq2] that overlaps neither, 16-byte aligned.
 *     An append is src = 0 .. nq-1, ~0 .. ~(m-1); a removal the surviving old columns in ascending order (m = the
 *     number removed, block NULL); an overwrite the identity with ~k at the positions given.  *flag_out (device
 *     uint32) = 1 when a src value lies outside [-m, nq): nothing is written for that column.  nq2 == 0 launches
 *     nothing.  Grid = (tile of 4096 output columns, rows 4 apart, 8 a trip): such rows split the tile into scalar
 *     head, 16-byte vectors and scalar tail alike, so a lane reads its 17 src values once and keeps them in registers;
 *     per row every load (4-byte gathers) is issued before the first 16-byte store.  No LDS, no scratch.
 * Limits (QRLSH_EINVAL otherwise): 0 <= nu, nq, nq2, m < 2^31. */
int qrlsh_ratings_columns_changed(const int32_t *ratings, int64_t nu, int64_t nq, const int32_t *cols,
                                  const int32_t *block, int64_t m, void *changed_map_out, uint64_t *out2, void *stream);
int qrlsh_ratings_columns_move(const int32_t *in, int64_t nu, int64_t nq, const int32_t *src, int64_t nq2,
                               const int32_t *block, int64_t m, int32_t *out, uint32_t *flag_out, void *stream);

/* ---- users join and leave the live user lists (csrc/userrows.hip) ------------------------------------------------------
 * The user-row counterpart of the column operations: labels and K stay those of the build.  New rows are the changed
 * rows R of the update above over grown arrays (no stored entry names a new id, so nothing is picked); removed rows are
 * R with mean and norm2 set to zero (every score against them is 0 and positive-only lists drop them), after which the
 * survivors are renumbered by rank.  Device pointers, one stream, nothing allocated.
 *   rows_nearest: rows int32 [m][nq] (a block of its own, 16-byte aligned) with rows_mean / rows_norm2 by
 *     qrlsh_user_rows_stats over it; ratings / mean / norm2 the nu existing users.  best_user_out[k] = the existing user
 *     with the largest milli(k, u) -- pairs_score's expression -- ties to the lowest id, best_milli_out[k] that value;
 *     (-1, 0) where no score is positive.  milli_out int32 [m][nu] = every score, NULL to skip.  Grid = (slice of 1024
 *     columns, tile of 8 new rows, group of 128 existing rows that are 4 apart: such rows share their alignment): the
 *     tile's slice is centred once into LDS (32 KB), every wave streams existing rows past it with 16-byte loads, and the
 *     exact integer partial dots are added to workspace int64 [nu][m] (qrlsh_user_rows_nearest_workspace_bytes(nu, m),
 *     8-byte aligned; cleared inside the call) with 64-bit integer atomics -- any order gives the same sum.  The matrix
 *     is read once per tile of new rows.  m == 0 returns at once.
 *   rows_move: out[u2] = src[u2] >= 0 ? in[src[u2]] : block[~src[u2]] for u2 < nu2, whole rows of nq values; in int32
 *     [nu][nq], block int32 [m][nq] (NULL when m == 0), out a fresh contiguous int32 [nu2][nq] that overlaps neither,
 *     16-byte aligned.  An append is src = 0 .. nu-1, ~0 .. ~(m-1); a removal the surviving rows in ascending order
 *     (m = 0).  *flag_out (device uint32) = 1 when a src value lies outside [-m, nu): that row is not written.  16-byte
 *     stores on the output's alignment with scalar head and tail; 16-byte loads where the source piece shares that
 *     alignment (always when nq % 4 == 0 and block is 16-byte aligned), 4-byte loads otherwise.  nu2 == 0 returns at once.
 *   lists_renumber: idx_out / milli_out [nu2][K], len_out [nu2] = row src[u2] of idx / milli / len [nu][K] with every
 *     id d rewritten to new_pos[d] (int32 [nu]; negative = gone); src[u2] < 0 = an empty row (-1 / 0 / 0).  *flag_out
 *     (device uint32) = 1 when an entry's target is gone or outside [0, nu2), an index outside [0, nu), a length outside
 *     [0, K] or a src value >= nu was seen: nothing is to be used then.  One lane per entry of the new lists.
 * Limits (QRLSH_EINVAL otherwise): 1 <= K <= 64; 0 <= nu, nu2, nq, m < 2^31; rows_nearest: m * nu < 2^32. */
size_t qrlsh_user_rows_nearest_workspace_bytes(int64_t nu, int64_t m);
int qrlsh_user_rows_nearest(const int32_t *ratings, int64_t nu, int64_t nq, const double *mean, const int64_t *norm2,
                            const int32_t *rows, int64_t m, const double *rows_mean, const int64_t *rows_norm2,
                            int32_t *best_user_out, int32_t *best_milli_out, int32_t *milli_out, void *workspace,
                            size_t workspace_bytes, void *stream);
int qrlsh_ratings_rows_move(const int32_t *in, int64_t nu, int64_t nq, const int32_t *src, int64_t nu2,
                            const int32_t *block, int64_t m, int32_t *out, uint32_t *flag_out, void *stream);
int qrlsh_user_lists_renumber(const int32_t *idx, const int32_t *milli, const int32_t *len, int64_t nu, int32_t K,
                              const int32_t *src, int64_t nu2, const int32_t *new_pos, int32_t *idx_out,
                              int32_t *milli_out, int32_t *len_out, uint32_t *flag_out, void *stream);

/* ---- dataset rows come and go under a built index (csrc/tablerows.hip) --------------------------------------------------
 * A dataset row lives in a SLOT: slot s owns row s of the permutation table (perm_t[s][0..P)) and bit s of every value
 * bitmap.  A table drawn for `capacity` rows has free slots behind the rows in use; an added row takes the lowest slot
 * never used, a removed row's slot stays dead and is not used again.  After any sequence of row operations signatures,
 * norms, band keys, index arrays and lists are those of qrlsh_answer_sets_* + qrlsh_minhash + a fresh index / run (at the
 * held K) over the edited table IN SLOT NUMBERING WITH THE SAME PERMUTATION TABLE.  The rule is this library's: the
 * reference draws permutation(drows) and never edits the dataset.
 * qrows int32 [n][nfeat]: the served queries as bitmap rows (value ids), -1 = unconstrained; a value that no table row
 * holds has a bitmap row of its own.  batch_cells int32 [m][nfeat]: the value id of every cell of the batch's rows;
 * batch_slots int32 [m]: their slots, distinct, each < the rows of perm_t (the caller's duty: the table is gathered at
 * them unchecked).  Query q matches batch row j iff for every f qrows[q][f] == -1 || qrows[q][f] == batch_cells[j][f];
 * no bitmap is read.  perm_t / perm_dtype / P / P_stride as qrlsh_minhash takes them; sig / sig_dtype the index's rows
 * [n][P] (compact rows need a uint16 table).
 *   mark: one lane per served query tests the batch in tiles of 64 rows (cells staged in LDS, read wave-uniformly) and
 *     keeps a 64-bit match mask per tile; the wave then walks its lanes with a non-zero mask, lanes as positions p in
 *     rounds of 64.  QRLSH_ROWS_ADD: q is changed iff some matched row has perm_t[slot_j][p] < sig[q][p], compared
 *     UNSIGNED, so the -1 / 0xFFFF of an empty answer set loses to every value.  QRLSH_ROWS_REMOVE (run BEFORE the bits
 *     are cleared): q is changed iff some matched row has perm_t[slot_j][p] == sig[q][p]: with a table whose columns hold
 *     distinct values exactly "the minimum was attained there"; with repeated values a query may be marked whose row then
 *     comes back unchanged, which is harmless.  Changed queries enter changed_map (an id map over the n queries,
 *     qrlsh_idmap_workspace_bytes(n) bytes, cleared inside the call, ready for qrlsh_idmap_list); a query that matches
 *     but does not change is not marked.  out2 (device uint64 [2]) = {matched queries, changed queries}.  The table rows
 *     are read where they are (64 rows are 8 - 64 KiB: L1 / L2).
 *   fill (ADD only): changed_ids = qrlsh_idmap_list of the mark (ascending), c of them.  One wave per changed query:
 *     lane j tests batch row j of a tile, the ballot is the mask; sig_out[x][p] = umin(sig[q][p], min over the matched j
 *     of perm_t[slot_j][p]) in the index's row format, norm2_out[x] the exact int64 squared norm.  Rows are written once,
 *     out of place; sig is never written (qrlsh_rows_replace does that).  An id >= n writes nothing.
 *   bitmaps_set_rows: sets (on = 1) or clears (on = 0) bit batch_slots[j] of bitmap rows batch_cells[j][f] and of
 *     live_row, with vector atomics on the words (bitmaps uint32 [rows][words_per_row]); a slot >= 32 * words_per_row or
 *     a negative row is skipped, a cell >= the bitmap's rows is the caller's duty.
 * Limits (QRLSH_EINVAL otherwise): n < 2^32 - 1, 1 <= nfeat <= 63 (the live row is the 64th column an answer-set query
 * can carry), m <= 65536 per call, any P >= 1.  No allocation, one stream, no scratch; m == 0 gives an empty map. */
#define QRLSH_ROWS_ADD 0
#define QRLSH_ROWS_REMOVE 1
int qrlsh_table_rows_mark(const int32_t *qrows, int64_t n, int32_t nfeat, const int32_t *batch_cells,
                          const int32_t *batch_slots, int64_t m, const void *perm_t, int32_t perm_dtype, int32_t P,
                          int32_t P_stride, const void *sig, int32_t sig_dtype, int32_t mode, void *changed_map,
                          uint64_t *out2, void *stream);
int qrlsh_table_rows_fill(const int32_t *qrows, int64_t n, int32_t nfeat, const int32_t *batch_cells,
                          const int32_t *batch_slots, int64_t m, const void *perm_t, int32_t perm_dtype, int32_t P,
                          int32_t P_stride, const void *sig, int32_t sig_dtype, const uint32_t *changed_ids, int64_t c,
                          void *sig_out, int64_t *norm2_out, void *stream);
int qrlsh_bitmaps_set_rows(uint32_t *bitmaps, int64_t words_per_row, const int32_t *batch_cells,
                           const int32_t *batch_slots, int64_t m, int32_t nfeat, int64_t live_row, int32_t on,
                           void *stream);

/* ---- multi-GPU, "sets" mode: answer sets of chosen queries out of the replicated per-shard CSR arrays ------------
 * Every rank holds every shard's answer sets as an all-gather delivered them: offs[world][nql + 1] (off_bytes = 4 or 8)
 * and rows[world][max_nnz] (row_bytes = 2: unsigned 16-bit row ids, tables of at most 65536 rows; or 4), shard g =
 * queries [g * nql, (g + 1) * nql).  For the n global query ids in `ids` (the remote queries a rank's pairs touch:
 * qrlsh_idset_list): _count writes offsets_out[n + 1] = exclusive scan of their set sizes ([n] = number of row ids:
 * the caller reads it back to allocate), _fill the row ids as int32 -- the CSR qrlsh_minhash takes.  Replaces a row
 * fetch from the owners: no signature row crosses a link.  Workspace: qrlsh_gather_sets_workspace_bytes(n). */
size_t qrlsh_gather_sets_workspace_bytes(int64_t n);
int qrlsh_gather_sets_count(const uint64_t *ids, int64_t n, const void *offs, int32_t off_bytes, int64_t nql,
                            int64_t world, uint64_t *offsets_out, void *workspace, size_t workspace_bytes,
                            void *stream);
int qrlsh_gather_sets_fill(const uint64_t *ids, int64_t n, const void *offs, int32_t off_bytes, const void *rows,
                           int32_t row_bytes, int64_t nql, int64_t max_nnz, const uint64_t *offsets,
                           int32_t *rows_out, void *stream);

/* ---- synthetic answer sets (bench / test input) ---------------
 * Bit-identical twin of oracle/qr_oracle.c:qro_synth_*: a pure function of (seed, q).
 * sizes: sizes_out[i] = |A(q0 + i)|; fill: rows at offsets[i] (offsets = exclusive scan).
 */
int qrlsh_synth_sizes(uint64_t seed, int64_t q0, int64_t nq_local, int64_t nq_total, int32_t cluster,
                      uint32_t D, const uint32_t *cdf, int32_t ncdf, uint32_t rep_thresh24,
                      int32_t *sizes_out, void *stream);
int qrlsh_synth_fill(uint64_t seed, int64_t q0, int64_t nq_local, int64_t nq_total, int32_t cluster,
                     uint32_t D, const uint32_t *cdf, int32_t ncdf, uint32_t rep_thresh24,
                     const int64_t *offsets, int32_t *rows_out, void *stream);

/* ---- optional per-kernel profiler ------------------------------------------------------
 * When enabled, every kernel launch of the library is bracketed by two HIP events recorded on
 * the launch stream.  qrlsh_prof_report waits for them and writes one "label count total_ms"
 * line per kernel label into buf_host; returns the number of labels.  enable(on) also clears
 * what was recorded so far; pause(1) / pause(0) stops / resumes the bracketing and keeps the
 * records (the events serialise back-to-back launches -- about 3 us per event, 10 % of a
 * config-2 step -- so bench.py brackets every Nth step of its timed region, not all of them).
 * bench.py uses this for the live roofline figures.
 */
int qrlsh_prof_enable(int on);
/* Intra-call overlap: qrlsh_bucket_pairs_emit* works its bands in groups that alternate between the caller's stream
 * and one auxiliary stream of the library (forked from / joined back into the caller's stream inside the call, so
 * the call stays ONE asynchronous operation on `stream`), letting a group's LDS-bound finish share the device
 * with the next group's memory-bound partition; qrlsh_topk_select_fill runs its medium- and long-list kernels there
 * beside the short-list one (from 2^22 queries on).  On by default; 0 (or the environment variable QRLSH_OVERLAP=0,
 * read on first use) runs everything on the caller's stream.  Steps bracketed by the profiler run serially. */
int qrlsh_set_overlap(int on);
int qrlsh_prof_pause(int paused);
int qrlsh_prof_report(char *buf_host, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* QRLSH_H */
