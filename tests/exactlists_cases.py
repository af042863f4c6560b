"""The exact neighbour lists (qrlsh.exact_neighbours, csrc/exactlists.hip) restated with Python sets and fractions (test
infrastructure only; nothing is taken from the code under test), and the shapes their tests run on.

Request x with chosen query s gets the j != s with |A(s) & A(j)| > 0, sorted by (-J(s, j), j) and cut at K; dst is padded
with -1, inter and union with 0; counts = (listed, positives).  The COO form drops the entries whose milli =
(2000 inter + union) // (2 union) is 0.  Every case builder asserts what makes its case worth running."""
from fractions import Fraction

import numpy as np

import fidelity_cases as FC

MAX_K = 64
LANE_GROUPS = 64         # 16-lane groups of a sweep workgroup (csrc/fidelitywalk.h FD_SWEEP_GROUPS)


# ---- restatements ------------------------------------------------------------------------------------------------------
def exact_ref(offsets, rows, K, queries=None):
    """-> dict: 'dst', 'inter', 'union' int32 [m, K], 'counts' int32 [m, 2]"""
    sets = FC.as_sets(offsets, rows)
    nq = len(sets)
    chosen = list(range(nq)) if queries is None else [int(q) for q in queries]
    m = len(chosen)
    out = dict(dst=np.full((m, K), -1, dtype=np.int32), inter=np.zeros((m, K), dtype=np.int32),
               union=np.zeros((m, K), dtype=np.int32), counts=np.zeros((m, 2), dtype=np.int32))
    for x, s in enumerate(chosen):
        found = []
        for j in range(nq):
            if j == s:
                continue
            i, u, jac = FC.jaccard(sets[s], sets[j])
            if i > 0:
                found.append((-jac, j, i, u))
        found.sort()
        for e, (_, j, i, u) in enumerate(found[:K]):
            out["dst"][x, e], out["inter"][x, e], out["union"][x, e] = j, i, u
        out["counts"][x] = (min(K, len(found)), len(found))
    return out


def milli_of(inter, union):
    """round-half-up of 1000 J, from the fraction: floor(1000 J + 1 / 2)"""
    v = Fraction(1000 * int(inter), int(union)) + Fraction(1, 2)
    return v.numerator // v.denominator


def coo_ref(ref, queries):
    """the (src, dst, milli) form of a restated result: rows by source ascending, the milli-0 entries left out"""
    queries = [int(q) for q in queries]
    assert len(set(queries)) == len(queries)
    src, dst, val = [], [], []
    for x in sorted(range(len(queries)), key=lambda x: queries[x]):
        for e in range(int(ref["counts"][x, 0])):
            mv = milli_of(ref["inter"][x, e], ref["union"][x, e])
            if mv > 0:
                src.append(queries[x])
                dst.append(int(ref["dst"][x, e]))
                val.append(mv)
    return tuple(np.array(a, dtype=np.int32) for a in (src, dst, val))


def exact_dense(offsets, rows, D, K, queries=None):
    """exact_ref's second form: a dense 0/1 matrix [nq, D], its Gram matrix as the intersections and a selection by
    cross-multiplication -- entry a is before b when inter_a union_b > inter_b union_a, or they are equal and a's id is
    smaller: K rounds of picking the entry no other is before"""
    nq = len(offsets) - 1
    member = np.zeros((nq, max(D, 1)), dtype=np.int64)
    owner = np.repeat(np.arange(nq), np.diff(offsets))
    member[owner, np.asarray(rows, dtype=np.int64)] = 1
    inter = member @ member.T
    size = member.sum(axis=1)
    union = size[:, None] + size[None, :] - inter
    chosen = np.arange(nq) if queries is None else np.asarray(queries, dtype=np.int64)
    m = len(chosen)
    out = dict(dst=np.full((m, K), -1, dtype=np.int32), inter=np.zeros((m, K), dtype=np.int32),
               union=np.zeros((m, K), dtype=np.int32), counts=np.zeros((m, 2), dtype=np.int32))
    ids = np.arange(nq)
    for x, s in enumerate(chosen.tolist()):
        i_s, u_s = inter[s], union[s]
        left = (i_s > 0) & (ids != s)
        positives = int(left.sum())
        for e in range(min(K, positives)):
            cand = ids[left]
            ci, cu = i_s[cand], u_s[cand]
            lhs, rhs = ci[:, None] * cu[None, :], ci[None, :] * cu[:, None]      # [a, b]: J_a against J_b
            beaten = (rhs > lhs) | ((rhs == lhs) & (cand[None, :] < cand[:, None]))   # some b is before a
            first = cand[~beaten.any(axis=1)]
            assert len(first) == 1                                              # the order is total
            j = int(first[0])
            out["dst"][x, e], out["inter"][x, e], out["union"][x, e] = j, i_s[j], u_s[j]
            left[j] = False
        out["counts"][x] = (min(K, positives), positives)
    return out


def same_lists(got, want, what=""):
    """every output word equal: got = an ExactLists (device tensors) or a dict like want"""
    if not isinstance(got, dict):
        got = dict(dst=got.dst, inter=got.inter, union=got.union,
                   counts=np.stack([_host(got.listed), _host(got.positives)], axis=1))
    for k in ("dst", "inter", "union", "counts"):
        a, b = _host(got[k]), np.asarray(want[k])
        assert a.dtype == np.int32 and a.shape == b.shape, (what, k, a.shape, b.shape, a.dtype)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5].tolist())


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


# ---- the one-word key --------------------------------------------------------------------------------------------------
def key_of(inter, union):
    """the sort key the issue allows in place of the cross-multiplication: floor(inter * 2^43 / union)"""
    return (int(inter) << 43) // int(union)


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, sets, D, name):
        self.offsets, self.rows = FC.from_sets(sets, D)
        self.sets, self.D, self.nq, self.name = sets, int(D), len(sets), name

    def ref(self, K, queries=None):
        return exact_ref(self.offsets, self.rows, K, queries)


def planted_case(D, nq=60, seed=5):
    """fidelity_cases' planted sets: query 0 and its five exact duplicates (J = 1 ties cut by id), a disjoint query, an
    empty one, the whole table, single rows at both ends of the table, random sets of 1 .. 65 rows"""
    c = FC.planted_case(D, nq=nq, seed=seed)
    case = Case(FC.as_sets(c.offsets, c.rows), D, "planted D=%d" % D)
    s = case.sets
    assert all(s[j] == s[0] for j in range(6)) and not s[7] and len(s[8]) == D and not s[0] & s[6]
    return case


def sizes_case(D=200):
    """sets of 0, 1, 31, 32, 33, 65 and D rows -- 33 and 65 reach the sweep's second walk past 2 x 16 rows -- as prefixes,
    as even rows and as suffixes, each twice more with one row moved so that no two J coincide by construction; nq stays
    below the 64 lane groups of a workgroup"""
    sets = []
    for sz in (0, 1, 31, 32, 33, 65, D):
        sets.append(set(range(sz)))
        sets.append(set(range(0, 2 * sz, 2)) if 2 * sz <= D else set(range(D - sz, D)))
        sets.append(set(range(D - sz, D)))
        if 1 < sz < D:
            sets.append(set(range(sz - 1)) | {D - 1})
            sets.append(set(range(1, sz)) | {D // 2})
    case = Case(sets, D, "sizes D=%d" % D)
    sizes = set(len(s) for s in sets)
    assert {0, 1, 31, 32, 33, 65, D} <= sizes and case.nq < LANE_GROUPS
    return case


def positives_case(K):
    """four chosen queries (0 .. 3) with exactly 0, K - 1, K and K + 1 queries that share a row with them, each on a row
    block of its own; the sharers hold 1 .. 8 rows of the block and up to 3 rows of their own, so J varies and repeats"""
    B = 8
    counts = (0, K - 1, K, K + 1)
    D = 4 * B + 4
    sets = [set(range(c * B, (c + 1) * B)) for c in range(4)]
    for c, p in enumerate(counts):
        for t in range(p):
            own = set(range(4 * B, 4 * B + t % 4))
            sets.append(set(range(c * B, c * B + 1 + t % B)) | own)
    # the private rows 32 .. 35 are shared among the sharers only
    sets += [set(), {D - 1}]
    case = Case(sets, D, "positives K=%d" % K)
    ref = case.ref(K, range(4))
    assert ref["counts"][:, 1].tolist() == list(counts) and ref["counts"][:, 0].tolist() == [0, K - 1, K, K]
    return case


def tie_case(nq=303, K=10, slices=(2, 7)):
    """One chosen query (0, six rows) whose neighbours fall into three classes spread evenly over the ids: J = 2/3 (every
    50th id), J = 1/2 written as 3/6, 4/8 and 5/10 (every other 3rd id), J = 1/10 (the rest).  The 1/2 class has members
    in every slice at 2 and 7 slices and the cut at K falls inside it: the list is the 2/3 class, then the LOWEST ids of
    the 1/2 class, whichever slice they sit in."""
    D = 64
    A = set(range(6))
    sets = [set(A)]
    for j in range(1, nq):
        if j % 50 == 0:
            sets.append({0, 1, 2, 3})                              # 4 / 6
        elif j % 3 == 0:
            k = 3 + (j // 3) % 3                                   # k rows of A and 2 (k - 3) of its own: k / 2 k
            sets.append(set(range(k)) | set(range(10, 10 + 2 * (k - 3))))
        else:
            sets.append({5, 20 + j % 7, 30, 31, 32})               # 1 / 10
    case = Case(sets, D, "ties nq=%d" % nq)
    ref = case.ref(K, [0])
    jac = [Fraction(int(i), int(u)) for i, u in zip(ref["inter"][0], ref["union"][0])]
    better = sum(1 for v in jac if v > Fraction(1, 2))
    half = [int(j) for j, v in zip(ref["dst"][0], jac) if v == Fraction(1, 2)]
    assert 0 < better < K and better + len(half) == K, (better, half)
    forms = set((int(i), int(u)) for i, u, v in zip(ref["inter"][0], ref["union"][0], jac) if v == Fraction(1, 2))
    assert len(forms) >= 2, forms                                  # equal J under different (inter, union)
    tied = [j for j in range(1, nq) if FC.jaccard(sets[0], sets[j])[2] == Fraction(1, 2)]
    assert half == tied[:len(half)] and len(tied) > K
    for S in slices:
        per = -(-nq // S)
        assert all(any(j // per == y for j in tied) for y in range(S)), S      # the class sits in every slice
    return case


def no_tail_case():
    """a real run's answer sets over a table so small that every positive J rounds to a milli above 0: the COO form drops
    nothing"""
    c = FC.lsh_case(**FC.LSH_SHAPES[0])
    case = Case(FC.as_sets(c.offsets, c.rows), c.D, "real sets D=%d" % c.D)
    assert milli_of(1, 2 * case.D) > 0
    return case


def tail_case():
    """query 0 holds one row of 2500 and shares it with sets large enough for a milli of 1 and of 0: a truncated COO row"""
    D = 2500
    sets = [{0}, {0, 1}, set(range(1100)), set(range(2400)), {0, 5, 6}, {2450}]      # 5 shares no row at all
    case = Case(sets, D, "tail")
    ref = case.ref(8, [0])
    millis = [milli_of(i, u) for i, u in zip(ref["inter"][0, :4], ref["union"][0, :4])]
    assert ref["counts"][0].tolist() == [4, 4] and millis[:2] == [500, 333] and millis[2:] == [1, 0], millis
    return case
