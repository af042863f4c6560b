"""The exact answer-set overlap of the neighbour lists (qrlsh.edge_overlaps / list_fidelity, csrc/fidelity.hip) restated
with Python sets and fractions (test infrastructure only; nothing is taken from the code under test), and the shapes
their tests run on.

Answer sets are a CSR (offsets int64 [nq + 1], rows int32, ascending per query); the lists a COO (src, dst, val) sorted by
src whose order within a row is the stored order.  J(s, j) = |A(s) & A(j)| / |A(s) | A(j)|, 0 when both are empty.  Every
case builder asserts what makes its case worth running."""
from fractions import Fraction

import numpy as np

import lists_update_cases as LC
import table_rows_cases as TC

MAX_K = 64               # entry slots per request
WORKGROUP_EDGES = 16     # edges a workgroup of the edge-overlap kernel serves (csrc/fidelity.hip FD_EDGES)
WORDS = ("listed", "size", "positives", "hits", "sure", "reachable", "disjoint", "inversions")


# ---- restatements ------------------------------------------------------------------------------------------------------
def as_sets(offsets, rows):
    rows = np.asarray(rows)
    return [set(rows[offsets[q]:offsets[q + 1]].tolist()) for q in range(len(offsets) - 1)]


def overlaps_ref(offsets, rows, src, dst):
    """int32 [n]: |A(src[e]) & A(dst[e])|"""
    sets = as_sets(offsets, rows)
    return np.array([len(sets[int(s)] & sets[int(d)]) for s, d in zip(src, dst)], dtype=np.int32).reshape(-1)


def list_rows(src, dst, nq):
    """the stored rows: row s = the dst of its entries in stored order"""
    out = [[] for _ in range(nq)]
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        out[s].append(d)
    return out


def jaccard(a, b):
    """(inter, union, J as a Fraction)"""
    i = len(a & b)
    u = len(a) + len(b) - i
    return i, u, (Fraction(i, u) if u else Fraction(0))


def fidelity_ref(offsets, rows, src, dst, nq, K, queries=None):
    """-> dict: 'inter', 'union', 'better', 'equal' int32 [m, 64], 'words' int64 [m, 8], 'totals' int64 [8]"""
    sets = as_sets(offsets, rows)
    stored = list_rows(src, dst, nq)
    chosen = list(range(nq)) if queries is None else [int(q) for q in queries]
    m = len(chosen)
    ent = {k: np.zeros((m, MAX_K), dtype=np.int32) for k in ("inter", "union", "better", "equal")}
    words = np.zeros((m, 8), dtype=np.int64)
    for x, s in enumerate(chosen):
        all_j = [jaccard(sets[s], sets[j]) for j in range(nq)]
        listed = stored[s][:K]
        assert len(stored[s]) <= MAX_K
        positives = sum(1 for j in range(nq) if j != s and all_j[j][0] > 0)
        js = []
        hits = sure = disjoint = 0
        for e, d in enumerate(listed):
            i, u, je = all_j[d]
            better = sum(1 for j in range(nq) if j != s and all_j[j][2] > je)
            equal = sum(1 for j in range(nq) if j != s and j != d and all_j[j][2] == je)
            ent["inter"][x, e], ent["union"][x, e], ent["better"][x, e], ent["equal"][x, e] = i, u, better, equal
            hits += better < K
            sure += better + equal < K
            disjoint += i == 0
            js.append(je)
        inversions = sum(1 for e in range(len(js)) for f in range(e + 1, len(js)) if js[e] < js[f])
        words[x] = (len(listed), len(sets[s]), positives, hits, sure, min(K, positives), disjoint, inversions)
    return dict(ent, words=words, totals=words.sum(axis=0))


def fidelity_dense(offsets, rows, D, src, dst, nq, K, queries=None):
    """fidelity_ref's second form: one dense 0/1 matrix [nq, D], its Gram matrix as the intersections, and the comparisons
    by cross-multiplication in int64 -> the same dict"""
    member = np.zeros((nq, max(D, 1)), dtype=np.int64)
    owner = np.repeat(np.arange(nq), np.diff(offsets))
    member[owner, np.asarray(rows, dtype=np.int64)] = 1
    inter = member @ member.T
    size = member.sum(axis=1)
    union = size[:, None] + size[None, :] - inter
    stored = list_rows(src, dst, nq)
    chosen = np.arange(nq) if queries is None else np.asarray(queries, dtype=np.int64)
    m = len(chosen)
    ent = {k: np.zeros((m, MAX_K), dtype=np.int32) for k in ("inter", "union", "better", "equal")}
    words = np.zeros((m, 8), dtype=np.int64)
    for x, s in enumerate(chosen.tolist()):
        i_s, u_s = inter[s], union[s]
        others = np.arange(nq) != s
        listed = stored[s][:K]
        L = len(listed)
        for e, d in enumerate(listed):
            lhs, rhs = i_s * u_s[d], i_s[d] * u_s          # J(s, j) against J_e, cross-multiplied
            ent["inter"][x, e], ent["union"][x, e] = i_s[d], u_s[d]
            ent["better"][x, e] = int(((lhs > rhs) & others).sum())
            ent["equal"][x, e] = int(((lhs == rhs) & others & (np.arange(nq) != d)).sum())
        positives = int(((i_s > 0) & others).sum())
        ie, ue = ent["inter"][x, :L].astype(np.int64), ent["union"][x, :L].astype(np.int64)
        less = (ie[:, None] * ue[None, :]) < (ie[None, :] * ue[:, None])      # J_e < J_f
        words[x] = (L, size[s], positives, int((ent["better"][x, :L] < K).sum()),
                    int((ent["better"][x, :L].astype(np.int64) + ent["equal"][x, :L] < K).sum()), min(K, positives),
                    int((ie == 0).sum()), int(np.triu(less, 1).sum()))
    return dict(ent, words=words, totals=words.sum(axis=0))


def same_result(got, want):
    """every output word equal: got = a ListFidelity (or a dict like want)"""
    g = got if isinstance(got, dict) else dict(got.entries, words=got.per_request, totals=got.totals)
    for k in ("inter", "union", "better", "equal", "words", "totals"):
        a, b = np.asarray(g[k]), np.asarray(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), (k, np.argwhere(a != b)[:5].tolist())


# ---- cases -------------------------------------------------------------------------------------------------------------
class FidelityCase:
    """offsets / rows over D table rows, the lists (src, dst, val) of nq queries, K"""

    def __init__(self, offsets, rows, D, src, dst, val, K, name):
        self.offsets, self.rows, self.D = np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.int32), int(D)
        self.src, self.dst, self.val = (np.asarray(a, dtype=np.int32) for a in (src, dst, val))
        self.nq, self.K, self.name = len(self.offsets) - 1, int(K), name

    def ref(self, queries=None, K=None):
        return fidelity_ref(self.offsets, self.rows, self.src, self.dst, self.nq, self.K if K is None else K, queries)


def from_sets(sets, D):
    sizes = [len(s) for s in sets]
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    rows = np.array([r for s in sets for r in sorted(s)], dtype=np.int32)
    assert rows.size == 0 or (rows.min() >= 0 and rows.max() < D)
    return offsets, rows


LSH_SHAPES = (dict(n=97, P=12, D=40, b=6, K=4, nfeat=3, nvals=3, seed=105),
              dict(n=300, P=32, D=500, b=16, K=8, nfeat=3, nvals=4, seed=31))


def lsh_case(n, P, D, b, K, nfeat, nvals, seed):
    """a real run in small: the answer sets of a random table, MinHash, the oracle's banding, scores and top K"""
    c = TC.Case(n=n, nfeat=nfeat, nvals=nvals, P=P, D=D, m=2, seed=seed)
    live = np.zeros(D + 2, dtype=bool)
    live[:D] = True
    offsets, rows = TC.brute_answer_sets(c.cells, c.qrows, live)
    assert np.array_equal(TC.minhash(offsets, rows, c.tab), c.sig)
    src, dst, val = LC.full_lists(c.sig, b, K)
    case = FidelityCase(offsets, rows, D, src, dst, val, K, "lsh n=%d" % n)
    sizes = np.diff(offsets)
    assert sizes[TC.Case.EMPTY] == 0 and sizes[TC.Case.ALL] == D      # an empty answer set, the whole table
    return case


def assert_lsh_case_is_telling(case, ref):
    t = dict(zip(WORDS, ref["totals"].tolist()))
    assert t["hits"] < t["listed"], "every listed entry is a true neighbour: recall is not tested"
    assert t["sure"] < t["hits"], "no ties at the cut"
    assert t["inversions"] > 0
    assert (ref["words"][:, 2] < case.K).any(), "every request can fill its K"
    assert 0 < t["listed"] and t["reachable"] > 0


def planted_case(D, nq=60, K=3, seed=5, whole=True):
    """Hand-made sets and lists that cover what a real run never stores.  Query 0 and its exact duplicates 1 .. 5 (J = 1
    ties that exceed K: sure < hits), 6 disjoint from 0, 7 empty, 8 the whole table (whole=True), 9 = {0}, 10 = {D - 1},
    11 = {0, D - 1}; the others random sets of 1, 15, 16, 17, 63, 64 and 65 rows drawn from a pool of 96 rows that includes
    both ends of the table, so that they overlap.  Lists: row 0 names its duplicates, the disjoint query and itself; row 7
    (empty set) names others; row 8 nothing; row 9 exactly K entries; row 10 exactly 64; the others random rows of up to
    2 K entries."""
    rng = np.random.default_rng(seed)
    assert D >= 16 and nq >= 20 + K
    pool = np.unique(np.concatenate(([0, D - 1], rng.choice(D, size=min(D, 96), replace=False))))
    base = set(rng.choice(pool, size=min(len(pool) // 2, 9), replace=False).tolist())
    sets = [set(base) for _ in range(6)]
    sets.append(set(int(r) for r in pool.tolist() if r not in base) or {0})
    sets.append(set())
    sets.append(set(range(D)) if whole else set(pool.tolist()))
    sets += [{0}, {D - 1}, {0, D - 1}]
    sizes = (1, 15, 16, 17, 63, 64, 65)
    while len(sets) < nq:
        sz = min(sizes[len(sets) % len(sizes)], len(pool))
        sets.append(set(rng.choice(pool, size=sz, replace=False).tolist()))
    offsets, rows = from_sets(sets, D)
    lists = {0: [1, 6, 2, 0, 3, 4, 5], 7: [0, 8, 7], 8: [], 9: list(range(20, 20 + K)),
             10: [int(j) for j in rng.permutation(nq)[:MAX_K]]}
    for s in range(nq):
        if s not in lists:
            lists[s] = [int(j) for j in rng.permutation(nq)[:int(rng.integers(0, 2 * K + 1))]]
    src = [s for s in range(nq) for _ in lists[s]]
    dst = [d for s in range(nq) for d in lists[s]]
    case = FidelityCase(offsets, rows, D, src, dst, np.zeros(len(src), dtype=np.int32), K, "planted D=%d" % D)
    assert len(lists[0]) > K and len(lists[9]) == K and not sets[0] & sets[6] and len(lists[10]) == min(nq, MAX_K)
    return case


def assert_planted_case_is_telling(case, ref):
    """over ALL requests at the case's K"""
    w = dict(zip(WORDS, ref["words"][0].tolist()))
    assert w["sure"] < w["hits"], "the duplicates of query 0 must tie beyond K"
    assert ref["words"][:, 6].sum() > 0, "no edge between disjoint sets"
    assert ref["words"][7, 1] == 0 and ref["words"][8, 0] == 0
    assert ref["words"][:, 7].sum() > 0


def overlap_case(D=200):
    """sets of 0, 1, 15, 16, 17, 63, 64, 65 and D rows in three placements (a prefix, the even rows = interleaved with the
    odd ones, a suffix = disjoint from short prefixes), pairs that share only their first or only their last row; the
    edges are all ordered pairs, src == dst among them"""
    sets = []
    for sz in (0, 1, 15, 16, 17, 63, 64, 65, D):
        sets.append(set(range(sz)))
        sets.append(set(range(0, 2 * sz, 2)) if 2 * sz <= D else set(range(D - sz, D)))
        sets.append(set(range(1, 2 * sz, 2)) if 2 * sz <= D else set(range(sz)))
        sets.append(set(range(D - sz, D)))
    sets += [{0} | set(range(100, 117)), {0} | set(range(120, 185)),              # the common row first
             set(range(60, 77)) | {D - 1}, set(range(100, 165)) | {D - 1}]       # ... or last
    offsets, rows = from_sets(sets, D)
    n = len(sets)
    src = np.repeat(np.arange(n), n).astype(np.int32)
    dst = np.tile(np.arange(n), n).astype(np.int32)
    want = overlaps_ref(offsets, rows, src, dst)
    assert (want == 0).any() and want.max() == D and len(src) > 3 * WORKGROUP_EDGES
    assert len(sets[-4] & sets[-3]) == 1 and len(sets[-2] & sets[-1]) == 1
    return offsets, rows, src, dst, want


def group_steps(group):
    """the D with group(D) != group(D + 1), D in [1, 2^20), found by bisection over the exported rule (non-increasing)"""
    steps, lo = [], 1
    while group(lo) != group(1 << 20):
        hi = 1 << 20                         # group(lo) > group(hi): the largest D with group(D) == group(lo)
        a = lo
        while hi - a > 1:
            mid = (a + hi) // 2
            if group(mid) == group(lo):
                a = mid
            else:
                hi = mid
        steps.append(a)
        lo = a + 1
    return steps
