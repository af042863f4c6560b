"""The postings of the answer sets (qrlsh.answer_postings) and the exact lists served from them
(qrlsh.exact_neighbours(postings=...), csrc/postings.hip) restated in numpy (test infrastructure only; nothing is taken
from the code under test), and the shapes their tests run on.

The postings are the transpose of the CSR (offsets, rows): p_qry = the owners of the entries in a STABLE order by row,
p_off the running row counts -- unique, so compared byte for byte.  The lists are exactlists_cases' (exact_ref, Case,
same_lists); for cases too large for Python sets fast_ref restates them per request with a membership gather and a sort
by the one-word key (inter << 43) // union, then id.  Every case builder asserts what makes its case worth running."""
from fractions import Fraction

import numpy as np

import exactlists_cases as XC
import fidelity_cases as FC

PASS_ENTRIES = 8192      # C: list entries per pass (csrc/postingsplan.h PP_PASS_ENTRIES; the library exports it)
QUEUE = 1024             # survivors between two drains (csrc/postings.hip PX_QUEUE)
LIST_CURSORS = 512       # posting lists whose cursors stay in LDS (csrc/postings.hip PX_LISTS)


# ---- restatements ------------------------------------------------------------------------------------------------------
def postings_ref(offsets, rows, D):
    """-> (p_off int64 [D + 1], p_qry int32 [nnz]) by a stable argsort of rows"""
    offsets, rows = np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    owner = np.repeat(np.arange(len(offsets) - 1, dtype=np.int32), np.diff(offsets))
    order = np.argsort(rows, kind="stable")
    p_off = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=D)[:D], out=p_off[1:])
    return p_off, owner[order].astype(np.int32)


def postings_lists(offsets, rows, D):
    """the same as a dict of lists: row -> its queries in the order the queries come"""
    held = {d: [] for d in range(D)}
    for q in range(len(offsets) - 1):
        for r in np.asarray(rows)[offsets[q]:offsets[q + 1]].tolist():
            held[r].append(q)
    return held


def fast_ref(offsets, rows, D, K, queries=None):
    """exact_ref's result without Python sets: per request a membership gather over all entries for the intersections,
    sizes from the offsets, a sort by (-(inter << 43) // union, id) -- the key test_exactlists_host pins as monotone and
    injective for unions up to 2^21"""
    offsets, rows = np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    nq = len(offsets) - 1
    sizes = np.diff(offsets)
    owner = np.repeat(np.arange(nq), sizes)
    chosen = list(range(nq)) if queries is None else [int(q) for q in queries]
    m = len(chosen)
    out = dict(dst=np.full((m, K), -1, dtype=np.int32), inter=np.zeros((m, K), dtype=np.int32),
               union=np.zeros((m, K), dtype=np.int32), counts=np.zeros((m, 2), dtype=np.int32))
    for x, s in enumerate(chosen):
        member = np.zeros(max(D, 1), dtype=bool)
        member[rows[offsets[s]:offsets[s + 1]]] = True
        inter = np.bincount(owner[member[rows]], minlength=nq)
        inter[s] = 0
        cand = np.flatnonzero(inter)
        i = inter[cand]
        u = sizes[s] + sizes[cand] - i
        assert (u < 1 << 21).all()
        key = ((i.astype(np.uint64) << np.uint64(43)) // u.astype(np.uint64)).astype(np.int64)
        top = np.lexsort((cand, -key))[:K]
        n = len(top)
        out["dst"][x, :n], out["inter"][x, :n], out["union"][x, :n] = cand[top], i[top], u[top]
        out["counts"][x] = (n, len(cand))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------
class ArrayCase:
    """a case given as sorted row lists (no Python sets are kept): the attributes of exactlists_cases.Case the tests read"""

    def __init__(self, lists, D, name):
        sizes = [len(r) for r in lists]
        self.offsets = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum(sizes, out=self.offsets[1:])
        self.rows = np.array([r for l in lists for r in l], dtype=np.int32)
        assert all(list(l) == sorted(set(l)) for l in lists)
        assert self.rows.size == 0 or (self.rows.min() >= 0 and self.rows.max() < D)
        self.D, self.nq, self.name = int(D), len(lists), name

    def ref(self, K, queries=None):
        return fast_ref(self.offsets, self.rows, self.D, K, queries)

    def list_length(self, row):
        return int((self.rows == row).sum())


def every_query_case(nq=300, D=10):
    """row 0 is held by every query: one posting list of nq entries; the other rows by every 2nd .. 9th query"""
    case = XC.Case([{0} | {d for d in range(1, D) if q % (d + 1) == 0} for q in range(nq)], D, "row 0 in every query")
    assert len(postings_lists(case.offsets, case.rows, D)[0]) == nq
    return case


def empty_rows_case():
    """D = 2^20 and a handful of queries: rows 0 .. 4 held by nobody, a gap of half the table, the last row empty"""
    D = 1 << 20
    case = XC.Case([{5, 6}, {6, D // 2}, set(), {5, D - 2}, {D // 2}], D, "empty rows at both ends")
    p_off, _ = postings_ref(case.offsets, case.rows, D)
    sizes = np.diff(p_off)
    assert not sizes[:5].any() and not sizes[7:D // 2].any() and sizes[D - 1] == 0 and sizes[D - 2] == 1
    return case


def single_row_case(others, C=PASS_ENTRIES):
    """query 0 = {0}; queries 1 .. others hold row 0 and j % 4 of the rows 1 .. 3; three more do not hold it.  The one
    list of request 0 has others + 1 entries (itself among them), and every candidate has multiplicity a = 1.  The last
    holder is a request of up to four long lists."""
    lists = [[0]] + [[0] + list(range(1, 1 + j % 4)) for j in range(1, others + 1)] + [[], [1], [2, 3]]
    case = ArrayCase(lists, 8, "one row, %d others" % others)
    assert case.list_length(0) == others + 1 and case.nq == others + 4
    case.requests = [0, others, 1]
    assert case.offsets[others + 1] - case.offsets[others] == 1 + others % 4
    return case


def narrow_case(C=PASS_ENTRIES):
    """4 C queries; only the ids [B, B + 3 C / 4) hold anything.  The request B holds rows 0 and 1, the others of the range
    row 0, row 1 or both (plus j % 3 rows of their own): the two lists together exceed C inside a range far narrower than
    the first, even window, which therefore overflows and is halved."""
    nq, B, W = 4 * C, C + 77, 3 * C // 4
    lists = [[] for _ in range(nq)]
    for j in range(B, B + W):
        base = [0] if j % 7 == 0 else [1] if j % 7 == 1 else [0, 1]
        lists[j] = base + list(range(2, 2 + j % 3))
    lists[B] = [0, 1]
    case = ArrayCase(lists, 8, "narrow range")
    total = case.list_length(0) + case.list_length(1)
    passes = -(-total // C)
    width = -(-nq // passes)
    assert total > C and passes == 2 and B + W <= width          # the first even window holds every entry: over C
    assert W < width // 2                                         # and so does its lower half or its upper one
    case.requests = [B, B + 1, B + W - 1, 0]
    return case


def unpruned_case(K=10, n=400):
    """request 0 holds rows 0 .. 2 and every candidate exactly one of them: inter = 1 throughout, so the bound 1 / 3 is
    never below a kept J (the K-th is 1 / (3 + size - 1)) and nothing is dropped before its union is formed"""
    lists = [[0, 1, 2]] + [[j % 3] + list(range(3, 3 + j % 5)) for j in range(1, n)]
    case = ArrayCase(lists, 8, "inter = 1 throughout")
    ref = case.ref(K, [0])
    assert (ref["inter"][0] == 1).all() and ref["counts"][0].tolist() == [K, n - 1]
    assert all(Fraction(1, 3) >= Fraction(int(i), int(u)) for i, u in zip(ref["inter"][0], ref["union"][0]))
    case.requests = [0]
    return case


def survivors_case(n=3000, C=PASS_ENTRIES):
    """request 0 = {0, 1}; n candidates hold both rows (multiplicity a = 2) and 0 .. 49 rows of their own, fewer towards the
    HIGH ids: one pass (2 n + 2 entries <= C) whose walk finds more survivors than the queue holds while nothing is kept
    yet, and the best entries come last"""
    lists = [[0, 1]] + [[0, 1] + list(range(2, 2 + (n - j) // 60)) for j in range(1, n + 1)]
    case = ArrayCase(lists, 64, "more survivors than the queue")
    assert n > 2 * QUEUE and 2 * n + 2 <= C
    ref = case.ref(10, [0])
    assert (ref["inter"][0] == 2).all() and ref["dst"][0].min() > QUEUE
    case.requests = [0, n]
    return case


def long_request_case(D=600, nq=40, seed=11):
    """query 0 holds all D = 600 rows: a = D, more lists than keep their cursors in LDS; the others random sets"""
    rng = np.random.default_rng(seed)
    lists = [list(range(D))] + [sorted(set(rng.choice(D, size=int(rng.integers(1, 30)), replace=False).tolist()))
                                for _ in range(nq - 2)] + [[]]
    case = ArrayCase(lists, D, "a = D = %d" % D)
    assert case.offsets[1] == D > LIST_CURSORS
    case.requests = [0, 1, nq - 1]
    return case
