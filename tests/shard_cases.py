"""References and case builders for the device glue of the query-sharded step (csrc/shard.hip, the tail of
csrc/score.hip, ops.topk_edges_local): the remote id set with its ranks and slots, the row and answer-set gathers,
the directed edge words in both formats, the re-based edge keys with their top-K cut, the exact band predicate and
the two-piece row table.  Shared by tests/test_shard_host.py (the test backend of the gloo driver tests against these
definitions, and the comparisons against planted defects; no GPU) and tests/test_gpu_shard.py (the kernels).

Pure numpy: nothing here needs the library, torch or a GPU.  The definitions are written independently of
tests/dist_worker.py:OracleBackend -- sets, Python integers and loops over explicit lists, no vectorised index
arithmetic -- so the two can be held against each other.  A pair word is i << 32 | j; 64-bit words are uint64 arrays.

WHICH PATH A SIZE RUNS (stated once here -- move the sizes below when the rule moves):
  * qr_scan_u64 scans up to 2 * 16384 words in one workgroup and takes three launches beyond.  The id set scans
    ceil(nids / 32) + 1 words: one workgroup up to nids = 1 048 544.  gather_sets scans n + 1 words: up to n = 32 767.
  * gather_rows caps its grid at 256 * 32 workgroups of 256 lanes, one 16-byte vector per lane and trip: 2 097 152
    vectors per trip, the grid-stride loop turns beyond.
  * the re-based edge key holds local_bits(nql) + 11 + id_bits bits and must fit 64.
"""
import bisect

import numpy as np

M32 = 0xFFFFFFFF
SCAN_ONE_WORKGROUP = 2 * 16384                               # words qr_scan_u64 scans without the chunked path
IDSET_LAST_SINGLE_SCAN = (SCAN_ONE_WORKGROUP - 1) * 32       # 1 048 544: ceil(nids / 32) + 1 == 32 768
GATHER_ROWS_VECTORS_PER_TRIP = 256 * 32 * 256                # 2 097 152
SETS_LAST_SINGLE_SCAN = SCAN_ONE_WORKGROUP - 1               # n + 1 == 32 768

IDSET_SMALL = (1, 31, 32, 33, 64)
IDSET_SCAN = (IDSET_LAST_SINGLE_SCAN, IDSET_LAST_SINGLE_SCAN + 1, (1 << 20) + 7)
IDSET_WIDE = (1 << 27) + 5
PAIR_COUNTS = (0, 1, 255, 256, 257)
WORLDS = (1, 2, 5, 8, 13)
ROW_FORMS = ((16, "u16", 8), (32, "u16", 16), (48, "u16", 24), (256, "u16", 128), (512, "u16", 256), (1024, "i32", 256))
SETS_N = (0, 1, 15, 16, 17, SETS_LAST_SINGLE_SCAN, SETS_LAST_SINGLE_SCAN + 1, 40000)
SET_LENGTHS = (0, 1, 15, 16, 17, 33)
VERIFY_SHAPES = ((5, 1), (40, 8), (96, 12), (128, 8), (7, 7))         # (P, b): r = 5, 5, 8, 16, 1
CHAIN_SHAPES = ((2, 600), (3, 601), (5, 603), (8, 1001), (13, 1001))  # (world, nq)


def ceil_div(a, b):
    return -(-a // b)


def local_bits(nql):
    """bits of a local id in [0, nql), at least 1"""
    lb = 1
    while (1 << lb) < nql:
        lb += 1
    return lb


def words(ints):
    return np.array([int(x) for x in ints], dtype=np.uint64)


def pair_words(ii, jj):
    return words((int(i) << 32) | int(j) for i, j in zip(ii, jj))


def endpoints(pairs):
    return [(int(p) >> 32, int(p) & M32) for p in pairs]


def same(got, want):
    """THE comparison of both test modules: same shape, same word size, every bit equal (signed and unsigned carriers
    of the same words compare equal; nothing is cast or rounded)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype.itemsize != want.dtype.itemsize:
        return False
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return bool(np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u)))


# ---------------------------------------------------------------------------- 1. id set
def ref_need(pairs, q0, nql):
    """the remote ids the pairs touch, ascending (a Python list)"""
    seen = set()
    for i, j in endpoints(pairs):
        for x in (i, j):
            if not q0 <= x < q0 + nql:
                seen.add(x)
    return sorted(seen)


def ref_bounds(need, nql, world, nids):
    """bounds[g] = how many needed ids lie below min(g * nql, nids): the per-owner request sizes, [-1] the total"""
    return np.array([sum(1 for x in need if x < min(g * nql, nids)) for g in range(world + 1)], dtype=np.int64)


def ref_slots(pairs, q0, nql, need):
    """slot(i) << 32 | slot(j) over the row table [local rows | rows of `need`]"""
    pos = {x: k for k, x in enumerate(need)}

    def slot(x):
        return x - q0 if q0 <= x < q0 + nql else nql + pos[x]
    return words((slot(i) << 32) | slot(j) for i, j in endpoints(pairs))


def ref_remap_search(pairs, q0, nql, need):
    """the binary-search entry: (i - q0) << 32 | slot(j), i local, slot(j) = the position where j enters `need`"""
    out = []
    for i, j in endpoints(pairs):
        assert q0 <= i < q0 + nql
        out.append(((i - q0) << 32) | (j - q0 if q0 <= j < q0 + nql else nql + bisect.bisect_left(need, j)))
    return words(out)


def word_edge_ids(edge, nids):
    """ids at the first and last bit of the bitmap words around `edge`, and the ids beside it"""
    w = edge // 32
    ids = {32 * w - 1, 32 * w, 32 * w + 31, 32 * w + 32, edge - 1, edge, edge + 1}
    return sorted(x for x in ids if 0 <= x < nids)


def idset_case(nids, world, rank, n, seed, plant=True):
    """pairs over [0, nids) for the rank that owns [q0, q0 + nql), nql = ceil(nids / world): n random ones and, with
    plant, the endpoints at the edges of the id space and of the bitmap words, one word with every bit set, one remote
    id in 3000 pairs, a pair with both ends remote and one with both local.  i <= j in every word (the kernels treat the
    two ends alike, and with nids = 1 there is only 0 | 0)."""
    rng = np.random.default_rng(seed)
    nql = ceil_div(nids, world)
    q0 = rank * nql
    assert q0 < nids, "a rank past the padding owns no id"
    a = [int(x) for x in rng.integers(0, nids, size=n)]
    c = [int(x) for x in rng.integers(0, nids, size=n)]
    remote = [x for x in range(nids) if not q0 <= x < q0 + nql] if nids <= 4096 else None
    local_hi = min(q0 + nql, nids) - 1
    facts = {}
    if plant:
        edge = [0, nids - 1] + word_edge_ids(q0, nids) + word_edge_ids(q0 + nql, nids)
        a += edge
        c += [int(x) for x in rng.integers(0, nids, size=len(edge))]
        a += [q0, local_hi]                                            # both ends local
        c += [local_hi, q0]
        far = (q0 + nql + 32 * 40) if q0 + nql + 32 * 44 <= nids else (0 if q0 >= 32 * 44 else None)
        if far is not None:
            w0 = 32 * ceil_div(far, 32)
            a += list(range(w0, w0 + 32))                              # every bit of one word
            c += list(range(w0 + 31, w0 - 1, -1))                      # ... from pairs with both ends remote
            hot = w0 + 32 + 5
            a += [hot] * 3000                                          # test-before-set: the bit is set after the first
            c += [int(x) for x in rng.integers(0, nids, size=3000)]
            facts["full_word"], facts["hot"] = w0, hot
    ii, jj = [min(x, y) for x, y in zip(a, c)], [max(x, y) for x, y in zip(a, c)]
    order = rng.permutation(len(ii))
    pairs = pair_words([ii[k] for k in order], [jj[k] for k in order])
    case = dict(pairs=pairs, q0=q0, nql=nql, nids=nids, world=world, facts=facts)
    need = ref_need(pairs, q0, nql)
    if plant:
        assert 0 in need or q0 == 0
        assert (nids - 1) in need or q0 <= nids - 1 < q0 + nql
        assert any(q0 <= i < q0 + nql and q0 <= j < q0 + nql for i, j in endpoints(pairs))
        if remote is not None:
            at_edges = set(word_edge_ids(q0, nids) + word_edge_ids(q0 + nql, nids))
            assert all(x in need for x in remote if x in at_edges)
        if "hot" in facts:
            assert sum(1 for i, j in endpoints(pairs) if facts["hot"] in (i, j)) >= 3000
            assert all(x in need for x in range(facts["full_word"], facts["full_word"] + 32))
            assert any(not q0 <= i < q0 + nql and not q0 <= j < q0 + nql for i, j in endpoints(pairs))
    return case


def all_local_case(nids, world, rank, n, seed):
    """pairs with both ends inside the rank's shard: nothing is remote, every bound is zero"""
    rng = np.random.default_rng(seed)
    nql = ceil_div(nids, world)
    q0 = rank * nql
    hi = min(q0 + nql, nids)
    assert hi > q0
    a, c = rng.integers(q0, hi, size=n), rng.integers(q0, hi, size=n)
    pairs = pair_words(np.minimum(a, c), np.maximum(a, c))
    assert n > 0 and ref_need(pairs, q0, nql) == []
    return dict(pairs=pairs, q0=q0, nql=nql, nids=nids, world=world, facts={})


def idset_cases(large):
    """(label, case) for every size, shard and pair count of the id set; large adds the sizes past the one-workgroup
    scan and the wide-id range.  Every rank listed owns at least one id"""
    out = []
    seed = 100
    for nids in IDSET_SMALL:
        for world in WORLDS:
            nql = ceil_div(nids, world)
            for rank in sorted(r for r in {0, (world - 1) // 2, ceil_div(nids, nql) - 1} if r * nql < nids):
                seed += 1
                out.append(("nids%d-w%d-r%d" % (nids, world, rank), idset_case(nids, world, rank, 40, seed)))
    for n in PAIR_COUNTS:                                                   # pair counts around one workgroup, no plants
        out.append(("n%d" % n, idset_case(1000, 5, 2, n, 200 + n, plant=False)))
    out.append(("n5000", idset_case(100_000, 8, 3, 5000, 300)))
    out.append(("q0=0", idset_case(5000, 2, 0, 500, 301)))
    out.append(("nql=1", idset_case(3000, 3000, 1500, 300, 302)))
    out.append(("padded-last", idset_case(5003, 13, 12, 500, 303)))        # 13 * 385 = 5005 > 5003
    out.append(("all-local", all_local_case(5003, 5, 2, 300, 304)))
    out.append(("all-local-w1", all_local_case(777, 1, 0, 300, 305)))
    if large:
        for k, nids in enumerate(IDSET_SCAN):
            for world, rank in ((1, 0), (5, 2), (13, 12)):
                out.append(("nids%d-w%d-r%d" % (nids, world, rank), idset_case(nids, world, rank, 3000, 400 + 3 * k + world)))
        out.append(("wide-r0", idset_case(IDSET_WIDE, 13, 0, 3000, 500)))
        out.append(("wide-last", idset_case(IDSET_WIDE, 8, 7, 3000, 501)))     # 8 * ceil(nids / 8) = nids + 3: padded
        assert IDSET_WIDE > (1 << 26) and 8 * ceil_div(IDSET_WIDE, 8) > IDSET_WIDE
    labels = [l for l, _ in out]
    assert len(set(labels)) == len(labels)
    assert any(c["nids"] % 32 == 0 and c["world"] * c["nql"] == c["nids"] for _, c in out)      # id == nids reads prefix[nw]
    assert any(c["world"] * c["nql"] > c["nids"] for _, c in out)                                # the clamp
    assert any(c["q0"] + c["nql"] > c["nids"] for _, c in out)
    return out


def search_case(case):
    """the pairs of an id-set case whose first end is local (the input of the binary-search entry)"""
    q0, nql = case["q0"], case["nql"]
    keep = [k for k, (i, j) in enumerate(endpoints(case["pairs"])) if q0 <= i < q0 + nql]
    return case["pairs"][keep]


# ---------------------------------------------------------------------------- 2. gather_rows
def row_table(nrows, kind, P, seed):
    """signature rows: compact uint16 words (carried as int16) or int32, every word random, so no two rows agree"""
    rng = np.random.default_rng(seed)
    if kind == "u16":
        sig = rng.integers(0, 1 << 16, size=(nrows, P)).astype(np.uint16).view(np.int16)
    else:
        sig = rng.integers(-1, 1 << 31, size=(nrows, P)).astype(np.int32)
    norm2 = rng.integers(0, 1 << 62, size=nrows).astype(np.int64)      # any words: the gather copies, it does not sum
    assert len({r.tobytes() for r in sig}) == nrows and len(set(norm2.tolist())) == nrows
    return sig, norm2


def request_ids(nrows, q0, n, seed, form="mixed"):
    """global ids [q0, q0 + nrows) as several ranks' requests arrive: unsorted, repeated, the first and last row in"""
    rng = np.random.default_rng(seed)
    if form == "equal":
        ids = np.full(n, q0 + nrows // 2, dtype=np.int64)
        assert n > 1
        return ids
    ids = rng.integers(q0, q0 + nrows, size=n).astype(np.int64)
    if n >= 4:
        ids[n // 2], ids[n // 3] = q0, q0 + nrows - 1
        ids[0] = ids[n - 1]
        assert np.any(np.diff(ids) < 0) and len(set(ids.tolist())) < n
        assert q0 in ids and q0 + nrows - 1 in ids
    return ids


def ref_gather_rows(sig, norm2, ids, q0):
    rows = [sig[int(x) - q0] for x in ids]
    norms = [int(norm2[int(x) - q0]) for x in ids]
    return (np.stack(rows) if rows else sig[:0].copy()), np.array(norms, dtype=np.int64)


# ---------------------------------------------------------------------------- 3. gather_sets
def shard_sets(world, nql, D, seed, empty_shard=None, off_dtype=np.int32, row_dtype=np.int16):
    """per-shard CSR arrays as the all-gather leaves them: offs [world][nql + 1], rows [world][max_nnz] (16-bit row ids
    are unsigned words carried as int16).  Every length of SET_LENGTHS occurs, the first and the last set of shard 0
    are empty, shard `empty_shard` holds empty sets only.  -> (offs, rows, sets) with sets[g][l] the list of row ids"""
    rng = np.random.default_rng(seed)
    sets = []
    for g in range(world):
        shard = []
        for l in range(nql):
            length = 0 if g == empty_shard else int(SET_LENGTHS[(l + g) % len(SET_LENGTHS)] if l % 7 else rng.integers(0, 40))
            shard.append([int(x) for x in rng.integers(0, D, size=length)])
        sets.append(shard)
    sets[0][0], sets[0][nql - 1] = [], []
    if nql >= 14 and empty_shard != 0:
        assert {len(x) for x in sets[0]} >= set(SET_LENGTHS)
    assert empty_shard is None or not any(sets[empty_shard])
    max_nnz = max(1, max(sum(len(s) for s in shard) for shard in sets))
    offs = np.zeros((world, nql + 1), dtype=off_dtype)
    rows = np.zeros((world, max_nnz), dtype=np.int64)
    for g in range(world):
        at = 0
        for l in range(nql):
            rows[g, at:at + len(sets[g][l])] = sets[g][l]
            at += len(sets[g][l])
            offs[g, l + 1] = at
    rows = rows.astype(np.uint16).view(np.int16) if row_dtype == np.int16 else rows.astype(np.int32)
    if row_dtype == np.int16:
        assert D <= 65536 and (D <= 32768 or any(x >= 32768 for shard in sets for s in shard for x in s))
    elif D > 65536:
        assert any(x > 65535 for shard in sets for s in shard for x in s)
    return offs, rows, sets


def set_ids(world, nql, n, seed):
    """n global query ids inside [0, world * nql), unsorted and repeated once n allows it"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, world * nql, size=n).astype(np.int64)
    if n >= 4:
        ids[0], ids[1], ids[n - 1] = world * nql - 1, 0, world * nql - 1
        assert np.any(np.diff(ids) < 0) and len(set(ids.tolist())) < n
    return ids


def ref_gather_sets(ids, sets, nql):
    """CSR of the chosen queries' sets: (offsets int64 [n + 1], rows int32)"""
    off, rows = [0], []
    for q in ids:
        g, l = divmod(int(q), nql)
        rows.extend(sets[g][l])
        off.append(len(rows))
    return np.array(off, dtype=np.int64), np.array(rows, dtype=np.int32)


# ---------------------------------------------------------------------------- 4. edge words
def ref_edges(pairs, milli, id_bits, wide):
    """both directed edges of every pair, [2t] = i -> j, [2t + 1] = j -> i: packed src << (id_bits + 11) |
    inv << id_bits | dst, or wide (key src << 11 | inv, dst); inv = 1000 - milli in [0, 2000]
    -> (keys uint64 [2n], dst int32 [2n] | None)"""
    keys, dst = [], []
    for (i, j), m in zip(endpoints(pairs), milli):
        inv = 1000 - int(m)
        assert 0 <= inv <= 2000
        for s, d in ((i, j), (j, i)):
            keys.append((s << 11) | inv if wide else (s << (id_bits + 11)) | (inv << id_bits) | d)
            dst.append(d)
    return words(keys), (np.array(dst, dtype=np.uint32).view(np.int32) if wide else None)


def edge_case(id_bits, n, seed):
    """n pairs with ids in [0, 2^id_bits), ids 0 and 2^id_bits - 1 in, milli over the whole of -1000 .. 1000"""
    rng = np.random.default_rng(seed)
    top = (1 << id_bits) - 1
    a, c = rng.integers(0, top + 1, size=n), rng.integers(0, top + 1, size=n)
    milli = rng.integers(-1000, 1001, size=n).astype(np.int32)
    if n >= 1:
        a[0], c[0], milli[0] = 0, top, -1000
    if n >= 3:
        a[1], c[1], milli[1] = top - (top > 0), top, 1000
        milli[2] = -1
        assert milli.min() == -1000 and milli.max() == 1000 and (milli < 0).sum() >= 2
    pairs = pair_words(np.minimum(a, c), np.maximum(a, c))
    return pairs, milli


def ref_group_by_owner(keys, dst, lo, nql, world):
    """edges in arrival order, grouped by the rank that owns their src (= key >> lo): (keys, dst | None, bounds)"""
    owner = [(int(k) >> lo) // nql for k in keys]
    order = [t for g in range(world) for t in range(len(owner)) if owner[t] == g]
    bounds = [sum(1 for o in owner if o < g) for g in range(world + 1)]
    return keys[order], (dst[order] if dst is not None else None), np.array(bounds, dtype=np.int64)


# ---------------------------------------------------------------------------- 5. re-based keys and the top-K cut
def ref_localize(keys, dst, id_bits, q0):
    """(src - q0) << (id_bits + 11) | inv << id_bits | dst of packed (dst None) or key + payload edges"""
    out = []
    for t, k in enumerate(keys):
        k = int(k)
        if dst is None:
            src, inv, d = k >> (id_bits + 11), (k >> id_bits) & 0x7FF, k & ((1 << id_bits) - 1)
        else:
            src, inv, d = k >> 11, k & 0x7FF, int(dst[t]) & M32
        out.append(((src - q0) << (id_bits + 11)) | (inv << id_bits) | d)
    assert all(0 <= x < (1 << 64) for x in out)
    return words(out)


def ref_topk(triples, K):
    """the K best of every src out of (src, inv, dst) triples in any order: ascending (src, inv, dst), i.e. value
    descending and the smaller id first among equal values -> (src, dst, milli) int32"""
    out, run = [], 0
    last = None
    for s, inv, d in sorted(triples):
        run = run + 1 if s == last else 1
        last = s
        if run <= K:
            out.append((s, d, 1000 - inv))
    a = np.array(out, dtype=np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


def pack_triples(triples, id_bits, wide):
    """(src, inv, dst) -> (keys uint64, dst int32 | None) in the packed or the key + payload format"""
    if wide:
        return (words((s << 11) | inv for s, inv, d in triples),
                np.array([d for _, _, d in triples], dtype=np.uint32).view(np.int32))
    assert 2 * id_bits + 11 <= 64
    return words((s << (id_bits + 11)) | (inv << id_bits) | d for s, inv, d in triples), None


def local_edges_case(id_bits, q0, nql, K, seed, lengths=None):
    """edges as a rank receives them (shuffled) for its queries [q0, q0 + nql): lists shorter than, equal to and longer
    than K, on the first and the last local query among them, a few values only (ties at the cut), inv past 1000
    (negative milli), dst < 2^min(id_bits, 31).  -> list of (src, inv, dst)"""
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = {0: K + 7, nql - 1: K, nql // 2: max(1, K - 1), nql // 3: 3 * K + 1, 1 % nql: 1}
    dmax = 1 << min(id_bits, 31)
    for _ in range(50):                                 # drawn again (same generator) until the shuffle tells the orders apart
        triples = []
        for l, length in sorted(lengths.items()):
            dsts = set()
            while len(dsts) < min(length, dmax):
                dsts.add(int(rng.integers(0, dmax)))
            for d in dsts:
                triples.append((q0 + l, int(rng.choice((0, 3, 999, 1000, 1001, 2000))), d))
        order = rng.permutation(len(triples))
        triples = [triples[k] for k in order]
        if any(inv > 1000 for _, inv, _ in triples) and (dmax <= 4 * K or ties_depend_on_order(triples, K)):
            break
    assert {s for s, _, _ in triples} >= {q0, q0 + nql - 1}
    assert any(inv > 1000 for _, inv, _ in triples)
    if dmax > 4 * K:
        assert ties_depend_on_order(triples, K), "the cut must tell arrival order from id order"
    return triples


def ties_depend_on_order(triples, K):
    """some list longer than K whose ties at the cut, taken in arrival order, are not the ones with the smallest ids"""
    by_src = {}
    for s, inv, d in triples:
        by_src.setdefault(s, []).append((inv, d))
    for lst in by_src.values():
        if len(lst) <= K:
            continue
        cut = sorted(lst)[K - 1][0]
        want = K - sum(1 for inv, _ in lst if inv < cut)
        ties = [d for inv, d in lst if inv == cut]
        if set(ties[:want]) != set(sorted(ties)[:want]):
            return True
    return False


def boundary_case(K, seed):
    """id_bits = 32 and nql = 2^21: the re-based key takes 21 + 11 + 32 = 64 bits.  Edges on local src 0 and nql - 1
    (bit 63 of the key set: negative as int64) and one in between; dst < 2^31"""
    id_bits, nql = 32, 1 << 21
    assert local_bits(nql) + 11 + id_bits == 64 and local_bits(nql + 1) + 11 + id_bits == 65
    return id_bits, nql, {0: K + 5, nql - 1: 2 * K + 3, (nql >> 1) + 1: K, nql - 2: 2}


# ---------------------------------------------------------------------------- 6. the exact band predicate
def ref_verify(sig, b, pairs):
    """1 where the two rows agree on the low 16 bits of every value of some band that is not all 0xFFFF (the -1 of an
    empty answer set) in them"""
    P = sig.shape[1]
    r = P // b
    assert r * b == P
    flags = []
    for i, j in endpoints(pairs):
        hit = 0
        for band in range(b):
            x = [int(v) & 0xFFFF for v in sig[i, band * r:(band + 1) * r]]
            y = [int(v) & 0xFFFF for v in sig[j, band * r:(band + 1) * r]]
            if x == y and any(v != 0xFFFF for v in x):
                hit = 1
        flags.append(hit)
    return np.array(flags, dtype=np.uint8)


def verify_case(P, b, wide_values, seed, n=257):
    """int64 [rows][P] signature values and n pair words over them.  The first pairs are planted (-> labels):
    equal in exactly the first / a middle / the last band; equal in every band but one value of each; a band all -1 in
    both rows (no hit); a band all -1 in one row only; and with wide_values (int32 rows only) values that differ by
    65536 (equal low halves: a hit) and 65535 beside -1 (equal low halves, all 0xFFFF: no hit).  The rest are random
    pairs of random rows.  -> (sig int64, pairs uint64, labels)"""
    rng = np.random.default_rng(seed)
    r = P // b
    top = 1 << 15                                                       # compact rows: values below 2^15, or -1
    rows, pp, labels = [], [], []

    def fresh():
        return [int(x) for x in rng.integers(0, top, size=P)]

    def add(x, y, label):
        rows.extend([x, y])
        pp.append((len(rows) - 2, len(rows) - 1))
        labels.append(label)

    for band in sorted({0, b // 2, b - 1}):
        x, y = fresh(), fresh()
        for k in range(P):
            if k // r != band and x[k] == y[k]:
                y[k] = (y[k] + 1) % top
        y[band * r:(band + 1) * r] = x[band * r:(band + 1) * r]
        add(x, y, "band %d only" % band)
    x = fresh()
    y = list(x)
    for band in range(b):
        k = band * r + int(rng.integers(0, r))
        y[k] = (y[k] + 1) % top
    add(x, y, "one value of each band differs")
    x, y = fresh(), fresh()
    for k in range(P):
        if x[k] == y[k]:
            y[k] = (y[k] + 1) % top
    x[0:r], y[0:r] = [-1] * r, [-1] * r
    add(x, y, "a band all -1 in both")
    add([-1] * P, [-1] * P, "all -1 in both")
    x, y = fresh(), fresh()
    for k in range(P):
        if x[k] == y[k]:
            y[k] = (y[k] + 1) % top
    x[(b - 1) * r:] = [-1] * r
    add(x, y, "a band all -1 in one row only")
    if wide_values:
        x = fresh()
        y = [v + 65536 * (1 + k % 3) for k, v in enumerate(x)]
        add(x, y, "values differ by multiples of 65536")
        x, y = fresh(), fresh()
        for k in range(P):
            if x[k] == y[k]:
                y[k] = (y[k] + 1) % top
        x[0:r], y[0:r] = [65535] * r, [-1] * r
        add(x, y, "65535 beside -1")
        if r > 1:
            x, y = fresh(), fresh()
            for k in range(P):
                if x[k] == y[k]:
                    y[k] = (y[k] + 1) % top
            y[0:r] = x[0:r]
            x[0], y[0] = 65535, -1
            add(x, y, "65535 beside -1 inside a live band")
    pool = [[fresh()[:r] for _ in range(2 * b + 1)] for _ in range(b)]   # random rows out of few tuples per band: some
    for _ in range(40):                                                 # pairs of them meet in a band, some in none
        rows.append([v for band in range(b) for v in pool[band][int(rng.integers(0, 2 * b + 1))]])
    sig = np.array(rows, dtype=np.int64)
    while len(pp) < n:
        i, j = (int(v) for v in rng.integers(0, len(rows), size=2))
        pp.append((min(i, j), max(i, j)))
    pp = pp[:n]
    pairs = pair_words([p[0] for p in pp], [p[1] for p in pp])
    if n >= len(labels):
        want = dict(zip(labels, ref_verify(sig, b, pairs[:len(labels)])))
        assert all(want[l] == 1 for l in labels if l.startswith("band "))
        assert want["one value of each band differs"] == 0 and want["a band all -1 in both"] == 0
        assert want["all -1 in both"] == 0 and want["a band all -1 in one row only"] == 0
        if wide_values:
            assert want["values differ by multiples of 65536"] == 1 and want["65535 beside -1"] == 0
            assert r == 1 or want["65535 beside -1 inside a live band"] == 1
        assert n < 100 or 0 < int(ref_verify(sig, b, pairs[len(labels):]).sum()) < n - len(labels)
    return sig, pairs, labels


def sig_rows(sig, kind):
    """int64 signature values -> the device's row words: int32, or compact uint16 (-1 -> 0xFFFF) carried as int16"""
    if kind == "i32":
        return sig.astype(np.int32)
    assert sig.min() >= -1 and sig.max() < 65535
    return np.where(sig < 0, 0xFFFF, sig).astype(np.uint16).view(np.int16)


# ---------------------------------------------------------------------------- 7. the two-piece row table
def split_case(P, split, n_fetched, n, seed, empty_rows=True):
    """signature values for `split` own rows and n_fetched fetched ones, and n pairs of table slots: both halves own,
    both fetched, one of each in both orders (as far as n and the pieces allow).  Some rows are all -1 (an empty answer
    set: cosine 0) and some differ from their partner in sign-free ways only.  -> (sig int64 [split + n_fetched][P],
    pairs uint64)"""
    rng = np.random.default_rng(seed)
    total = split + n_fetched
    sig = rng.integers(0, 30000, size=(total, P)).astype(np.int64)
    sig[rng.integers(0, total, size=max(1, total // 4))] = sig[0]       # near and exact duplicates: milli up to 1000
    if total > 3:
        sig[1] = rng.integers(32768, 65535, size=P)                     # bit 15 set: not the -1 of a compact row
    if empty_rows and total > 2:
        sig[total - 1] = -1
    own = lambda: int(rng.integers(0, split))                           # noqa: E731
    got = lambda: split + int(rng.integers(0, n_fetched))               # noqa: E731
    kinds = [(own, own)] + ([(got, got), (own, got), (got, own)] if n_fetched else [])
    pp = [(kinds[t % len(kinds)][0](), kinds[t % len(kinds)][1]()) for t in range(n)]
    pairs = pair_words([p[0] for p in pp], [p[1] for p in pp])
    if n_fetched and n >= 4:
        ends = endpoints(pairs)
        assert any(i >= split and j >= split for i, j in ends) and any(i < split and j < split for i, j in ends)
        assert any(i < split <= j for i, j in ends) and any(j < split <= i for i, j in ends)
    return sig, pairs


# ---------------------------------------------------------------------------- 8. the chain on one simulated rank
def mix64(z):
    z = int(z)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    return z ^ (z >> 31)


def ref_pair_host(pairs, nql):
    """the rank that scores a pair: the owner of j when the top bit of mix64(pair) is set, else of i"""
    return np.array([((int(p) & M32) if mix64(p) >> 63 else (int(p) >> 32)) // nql for p in pairs], dtype=np.int64)


def chain_case(world, nq, P, seed, shards=None):
    """one global list of sorted candidate pairs over nq queries in `world` shards of nql = ceil(nq / world), and the
    signature values of every (padded) query.  Pairs cluster on few queries, so lists pass K and cross shards.
    shards: the only shards whose queries occur in a pair (the other ranks host nothing and receive no edge)"""
    rng = np.random.default_rng(seed)
    nql = ceil_div(nq, world)
    ids = np.array([q for q in range(nq) if shards is None or q // nql in shards])
    sig = rng.integers(0, 50, size=(world * nql, P)).astype(np.int64)   # few values: equal scores, ties at the cut
    sig[rng.integers(0, nq, size=nq // 10)] = -1                         # empty answer sets: milli 0
    sig[nq:] = -1
    hubs = rng.choice(ids, size=6)
    a = np.concatenate([rng.choice(ids, size=6 * nq), np.repeat(hubs, 60)])
    c = np.concatenate([rng.choice(ids, size=6 * nq), rng.choice(ids, size=360)])
    keep = a != c
    pairs = np.array(sorted(set(pair_words(np.minimum(a, c)[keep], np.maximum(a, c)[keep]).tolist())), dtype=np.uint64)
    host = ref_pair_host(pairs, nql)
    assert 0.3 < np.mean(host == [i // nql for i, _ in endpoints(pairs)]) < 0.95
    if world > 1:
        assert any(i // nql != j // nql for i, j in endpoints(pairs))
    if shards is not None:
        assert set(host.tolist()) == set(shards) and len(shards) < world
    return dict(world=world, nq=nq, nql=nql, sig=sig, pairs=pairs, host=host)
