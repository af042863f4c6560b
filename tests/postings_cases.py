"""The postings of the answer sets (qrlsh.answer_postings) and the exact lists served from them
(qrlsh.exact_neighbours(postings=...), csrc/postings.hip) restated in numpy (test infrastructure only; nothing is taken
from the code under test), and the shapes their tests run on.

The postings are the transpose of the CSR (offsets, rows): p_qry = the owners of the entries in a STABLE order by row,
p_off the running row counts -- unique, so compared byte for byte.  The lists are exactlists_cases' (exact_ref, Case,
same_lists); for cases too large for Python sets fast_ref restates them per request with a membership gather and a sort
by the one-word key (inter << 43) // union, then id.  Every case builder asserts what makes its case worth running; the
builders of the shapes beyond one pass do so through plan_ref (the window rule, restated from the prose at the top of
csrc/postingsplan.h), slot_ref (the home slot, used only to choose ids) and lanes_ref (lanes per list of the fill)."""
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


# ---- the window rule and the home slot, restated ----------------------------------------------------------------------
def plan_ref(case, s, C=PASS_ENTRIES):
    """The passes of request s as csrc/postingsplan.h's prose gives them -> [(lo, hi, count, halvings)].  The request
    reads the posting lists of its rows (its own id among their entries).  total entries -> ceil(total / C) windows of
    equal width ceil(nq / windows) over [0, nq), the last one cut at nq; a window of more than C entries that is wider
    than one id keeps its lo and loses the upper half of its width (rounded down) until it holds at most C entries or is
    one id.  A request without entries has no passes."""
    offsets, rows = np.asarray(case.offsets, dtype=np.int64), np.asarray(case.rows, dtype=np.int64)
    nq = len(offsets) - 1
    member = np.zeros(max(case.D, 1), dtype=bool)
    member[rows[offsets[s]:offsets[s + 1]]] = True
    owner = np.repeat(np.arange(nq), np.diff(offsets))
    ids = np.sort(owner[member[rows]])                   # every entry of every list the request reads
    total = len(ids)
    if total == 0:
        return []
    windows = -(-total // C)
    width = nq if windows <= 1 else max(1, -(-nq // windows))
    passes, lo = [], 0
    while lo < nq:
        hi, halvings = min(lo + width, nq), 0
        while True:
            count = int(np.searchsorted(ids, hi) - np.searchsorted(ids, lo))
            if count <= C or hi - lo <= 1:
                break
            hi, halvings = lo + (hi - lo) // 2, halvings + 1
        passes.append((lo, hi, count, halvings))
        lo = hi
    return passes


def slot_ref(id):
    """the multiplicative home slot of an id in the table of 16384 slots; used to CHOOSE ids, never for a result"""
    return ((int(id) * 2654435761) % (1 << 32)) >> 18


TABLE_SLOTS = 1 << 14    # what slot_ref maps into (csrc/postingsplan.h PP_TABLE_SLOTS = 2 C)
THREADS = 1024           # threads of a request's workgroup (csrc/postings.hip PX_THREADS)


def lanes_ref(a, cursors=LIST_CURSORS, threads=THREADS):
    """lanes per list in the fill: the widest power of two that still gives each of the a lists a group of its own
    (L a <= threads); 1 for a request whose cursors do not stay in LDS"""
    if a > cursors:
        return 1
    L = 1
    while L < threads and 2 * L * a <= threads:
        L *= 2
    return L


def _busy(plan):
    return [p for p in plan if p[2]]


# ---- the shapes no one-pass case reaches ------------------------------------------------------------------------------
def long_windows_case(D=600, nq=4096, base=1500, span=64, per=300, seed=3, C=PASS_ENTRIES, cursors=LIST_CURSORS):
    """MORE THAN PX_LISTS LISTS AND MORE THAN ONE WINDOW: only the ids base .. base + span - 1 hold anything.  base holds
    all D rows, base + 1 / + 2 / + 3 the first cursors - 1 / cursors / cursors + 1 rows (a = 511 / 512 / 513 side by side:
    the last request whose cursors stay in LDS and the first two that recompute their bounds from memory), the rest `per`
    random rows.  The entries exceed 2 C inside a range far narrower than an even window: the requests of a >= cursors - 1
    take at least 3 non-empty passes, every one with lo > 0 -- the pp_lower_bound(.., lo) / (.., hi) pair of the
    out-of-LDS path under windows and under halving.  base + 10 (a = per) stays in LDS and still takes 2 passes."""
    rng = np.random.default_rng(seed)
    assert cursors + 1 < D and base + span <= nq and span > 10
    lists = [[] for _ in range(nq)]
    lists[base] = list(range(D))
    for k, a in enumerate((cursors - 1, cursors, cursors + 1)):
        lists[base + 1 + k] = list(range(a))
    for j in range(base + 4, base + span):
        lists[j] = sorted(rng.choice(D, size=per, replace=False).tolist())
    case = ArrayCase(lists, D, "long windows D=%d C=%d" % (D, C))
    case.requests = [base, base + 1, base + 2, base + 3, base + 10, 0]
    assert case.offsets[1] == 0                                   # request 0 is empty
    sizes = np.diff(case.offsets)
    assert [int(sizes[base + k]) for k in range(4)] == [D, cursors - 1, cursors, cursors + 1]
    for s in case.requests[:4]:
        plan = plan_ref(case, s, C)
        busy = _busy(plan)
        assert len(busy) >= 3 and sum(p[3] for p in plan) >= 1, (s, plan)
        assert all(p[2] <= C for p in plan) and all(p[0] > 0 for p in busy), (s, plan)
        assert any(p[3] and p[2] for p in plan), (s, plan)        # a halved window that holds entries
    assert sizes[base + 10] == per <= cursors and len(_busy(plan_ref(case, base + 10, C))) >= 2
    return case


def hot_id_case(C=PASS_ENTRIES, nq=40):
    """A PASS THAT IS A SINGLE ID OF MORE THAN C ENTRIES (the hi - lo <= 1 arm of the pass rule): D = C + 8 rows; ids 0,
    17 and 18 hold every row, id 19 the first C + 1, id 5 every third, id 30 five.  Request 0 reads D lists; the windows
    at ids 0, 17, 18 and 19 are halved down to one id and still hold D, D, D and C + 1 entries.  The one at id 0 is the
    request itself: every entry is skipped and its table stays empty."""
    D = C + 8
    lists = [[] for _ in range(nq)]
    for j in (0, 17, 18):
        lists[j] = list(range(D))
    lists[19] = list(range(C + 1))
    lists[5] = list(range(0, D, 3))
    lists[30] = [0, 1, C, C + 3, D - 1]
    case = ArrayCase(lists, D, "hot ids C=%d" % C)
    case.requests = [0, 19, 30, 5]
    plan = {p[0]: p for p in plan_ref(case, 0, C)}
    for j, count in ((0, D), (17, D), (18, D), (19, C + 1)):
        assert plan[j][1] == j + 1 and plan[j][2] == count > C and plan[j][3] >= 1, (j, plan.get(j))
    ref = case.ref(4, [0])
    assert ref["dst"][0].tolist() == [17, 18, 19, 5] and ref["inter"][0].tolist()[:2] == [D, D]
    return case


_CHAIN_ROWS = ([0], [1], [2], [0, 1], [1, 2], [0, 2], [0, 1, 2])


def probe_chain_case(nq=1 << 17, C=PASS_ENTRIES, tail=32, head=64):
    """PROBE CHAINS: the candidates are the ids whose home slot (slot_ref) lies in the last `tail` slots of the table, far
    more keys than those slots, so their chains run past slot 16383 and wrap to slot 0 -- where the ids whose home is one
    of the first `head` slots crowd as well.  The request holds rows 0, 1 and 2; a candidate holds one, two or all three
    of them by id % 7 (keys that collide carry DIFFERENT multiplicities) and id % 5 rows of its own.  One pass."""
    slots = np.array([slot_ref(j) for j in range(nq)])
    last = np.flatnonzero(slots >= TABLE_SLOTS - tail)
    first = np.flatnonzero(slots < head)
    chosen = set(last.tolist()) | set(first.tolist())
    s = min(j for j in range(nq) if j not in chosen)
    lists = [[] for _ in range(nq)]
    for j in chosen:
        lists[j] = _CHAIN_ROWS[j % 7] + list(range(3, 3 + j % 5))
    lists[s] = [0, 1, 2]
    case = ArrayCase(lists, 8, "probe chains nq=%d" % nq)
    full = [int(j) for j in last if j % 7 == 6]
    assert nq - 1 not in chosen and nq - 1 != s                                    # the fourth request is an empty query
    case.requests = [s, full[-1], int(first[len(first) // 2]), nq - 1]
    assert len(last) > tail and len(first) > head, (len(last), len(first))       # more keys than home slots: chains
    assert len(last) + len(first) > tail + head                                   # the wrapped chain meets a full band
    for r in case.requests[:3]:
        plan = plan_ref(case, r, C)
        assert len(plan) == 1 and plan[0][:2] == (0, nq) and plan[0][2] <= C, (r, plan)
    ref = case.ref(64, [s])
    assert ref["counts"][0, 1] == len(chosen)
    assert {len(_CHAIN_ROWS[int(j) % 7]) for j in last} == {1, 2, 3}              # >= 3 multiplicities among colliders
    home = {}
    for j in last.tolist():
        home.setdefault(slot_ref(j), set()).add(len(_CHAIN_ROWS[j % 7]))
    assert any(len(v) >= 2 for v in home.values())                                 # and within one home slot
    return case


LANE_SIZES = (1, 2, 3, 5, 8, 9, 16, 17, 64, 100, 256, 257, 512)


def lanes_case(nq=5000, sizes=LANE_SIZES, shared=1200, seed=7, threads=THREADS, cursors=LIST_CURSORS):
    """LANES PER LIST: L = lanes_ref(a) takes another power of two for every request size here (1024 for a = 1 down to 2
    for a = 257 and 512).  Row 0 is held by about 3 in 10 queries, row 1 by 6 in 10; every request has a row nobody else
    holds and draws the rest from `shared` short rows, so each request of a >= 2 reads lists both longer and shorter
    than its L; a = 1 is run twice, on the longest list and on a list of one entry."""
    rng = np.random.default_rng(seed)
    n_req = len(sizes) + 1
    D = 2 + n_req + shared
    lists = [[] for _ in range(nq)]
    for q in range(nq):
        own = sorted(set((2 + n_req + rng.integers(0, shared, size=int(rng.integers(0, 3)))).tolist()))
        lists[q] = ([0] if q % 10 < 3 else []) + ([1] if q % 5 < 3 else []) + own
    step = nq // (n_req + 1)
    case_requests = []
    for k, a in enumerate(sizes + (1,)):
        q = (k + 1) * step + 1
        private = 2 + k
        if k == len(sizes):
            rows = [private]                                                       # a = 1 again: a list of one entry
        elif a == 1:
            rows = [1]
        elif a == 2:
            rows = [1, private]
        else:
            rows = [0, 1, private] + sorted((2 + n_req + rng.choice(shared, size=a - 3, replace=False)).tolist())
        lists[q] = rows
        case_requests.append(q)
    case = ArrayCase(lists, D, "lanes nq=%d" % nq)
    case.requests = case_requests
    length = np.bincount(case.rows, minlength=D)
    seen = set()
    for q, a in zip(case.requests, sizes + (1,)):
        mine = case.rows[case.offsets[q]:case.offsets[q + 1]]
        assert len(mine) == a
        L = lanes_ref(a, cursors, threads)
        assert L * a <= threads and (L == threads or 2 * L * a > threads) and L & (L - 1) == 0
        seen.add(L)
        longer, shorter = (length[mine] > L).any(), (length[mine] < L).any()
        assert (longer and shorter) if a >= 2 else (longer or shorter), (q, a, L)
    assert length[1] > threads and length[2 + len(sizes)] == 1                     # the two a = 1 requests: both sides
    assert min(seen) == 2 and max(seen) == threads and len(seen) == threads.bit_length() - 1, sorted(seen)   # every power
    return case


def late_windows_case(C=PASS_ENTRIES, K=8, stride=13):
    """A THRESHOLD EARNED IN AN EARLY WINDOW PRUNES THE LATER ONES.  Request 0 holds rows 0 .. 5.  Ids 1 .. 8 are its K = 8
    best (J = 5/6 three times, 4/6 four times, then {0, 1, 2}: 3/6) and sit in the first window.  Every later window
    holds candidates strictly below 3/6 (inter 1 or 2: bound below the threshold), subsets {3, 4, 5} of the request with
    J = 3/6 EXACTLY the K-th entry's -- higher ids, so they lose the tie -- and {0, 1, 2, 7}, whose bound 3/6 equals the
    threshold and whose J = 3/7 does not.  Request nq - 2 ({8 .. 11}) has its whole class J = 2/4 at LOWER ids than its
    three better entries, in one window: the lowest ids of the class win the places left."""
    nq, D, M = 3 * C, 16, (3 * C) // 2
    assert K == 8 and nq - 2 > M + 40 and M > 100
    lists = [[] for _ in range(nq)]
    for j in range(9, nq - 2):
        if j % stride == 5:
            lists[j] = [3, 4, 5]
        elif j % stride == 6:
            lists[j] = [0, 1, 2, 7]
        else:
            lists[j] = ([0, 12 + j % 3], [1, 2], [3, 13], [4, 5, 12, 14])[j % 4]
    for j in range(1, 9):
        lists[j] = [0, 1, 2, 3, 4] if j <= 3 else [0, 1, 2, 3] if j <= 7 else [0, 1, 2]
    lists[0] = [0, 1, 2, 3, 4, 5]
    for j in range(M, M + 40):                                    # request nq - 2's block: nothing of request 0's here
        lists[j] = [8, 12 + j % 4]
    klass = [M + 2 * i for i in range(12)]
    for j in klass:
        lists[j] = [8, 9]
    better = [M + 30, M + 31, M + 33]
    for j in better:
        lists[j] = [8, 9, 10]
    lists[nq - 2] = [8, 9, 10, 11]
    case = ArrayCase(lists, D, "late windows C=%d" % C)
    case.requests = [0, nq - 2, nq - 1]
    busy = _busy(plan_ref(case, 0, C))
    assert len(busy) >= 3 and busy[0][0] <= 1 and busy[0][1] > 8, busy            # the K best: all in the first window
    ref = case.ref(K, [0, nq - 2])
    assert ref["dst"][0].tolist() == list(range(1, 9))
    kth = Fraction(int(ref["inter"][0, K - 1]), int(ref["union"][0, K - 1]))
    assert kth == Fraction(3, 6)
    sizes, a = np.diff(case.offsets), 6
    for lo, hi, _, _ in busy[1:]:                                                 # every later window holds all three
        ids = [j for j in range(max(lo, 9), min(hi, nq - 2)) if not M <= j < M + 40]
        tied = [j for j in ids if lists[j] == [3, 4, 5]]
        edge = [j for j in ids if lists[j] == [0, 1, 2, 7]]
        assert tied and edge and min(tied) > 8, (lo, hi)
        assert all(Fraction(3, a + int(sizes[j]) - 3) == kth and a + int(sizes[j]) - 3 == a for j in tied)
        assert all(Fraction(3, a) == kth > Fraction(3, a + int(sizes[j]) - 3) for j in edge)
        assert all(Fraction(len(set(lists[j]) & set(lists[0])), a) < kth for j in ids if j not in tied and j not in edge)
    plan2 = _busy(plan_ref(case, nq - 2, C))
    assert len(plan2) == 1 and plan2[0][0] <= M and plan2[0][1] > max(better)     # one window holds the class and the kept
    assert max(klass) < min(better) and len(klass) > K - len(better)
    assert ref["dst"][1].tolist() == better + klass[:K - len(better)]
    assert all(Fraction(int(i), int(u)) == Fraction(2, 4) for i, u in zip(ref["inter"][1, 3:], ref["union"][1, 3:]))
    return case


RANDOM_GRID = tuple((nq, D) for nq in (257, 5000) for D in (8, 64, 700))
RANDOM_KS = (1, 7, 63, 64)


def random_cases(seed=0, grid=RANDOM_GRID, requests=16):
    """a seeded differential grid: set sizes skewed towards small (about a sixth empty, one query holds every row), rows
    drawn with a skew of their own, so small D gives heavy J ties and D = 700 requests on both sides of the 512 lists.
    Each case carries 16 requests: the largest sets, empty ones, random ones."""
    out = []
    for nq, D in grid:
        rng = np.random.default_rng([seed, nq, D])
        weight = 1.0 / np.arange(1, D + 1) ** 0.7
        weight /= weight.sum()
        lists = []
        for q in range(nq):
            size = 0 if rng.random() < 1 / 6 else min(D, 1 + int(D * rng.random() ** (4 if D <= 64 else 16)))
            lists.append(sorted(rng.choice(D, size=size, replace=False, p=weight).tolist()))
        lists[nq // 3] = list(range(D))
        case = ArrayCase(lists, D, "random nq=%d D=%d seed=%d" % (nq, D, seed))
        sizes = np.diff(case.offsets)
        third = requests // 3
        big = np.argsort(-sizes, kind="stable")[:third].tolist()
        empty = np.flatnonzero(sizes == 0)[:third].tolist()
        some = rng.choice(nq, size=requests - len(big) - len(empty), replace=False).tolist()
        case.requests = [int(q) for q in big + empty + some]
        assert len(case.requests) == requests and empty and sizes[big[0]] == D
        out.append(case)
    return out


def concat_cases(cases, name):
    """block-diagonal: the queries of the cases one after another, each over rows of its own -> an ArrayCase whose
    .requests are the cases' requests under their new ids, and .starts the first id of each case"""
    lists, starts, requests, row0 = [], [], [], 0
    for c in cases:
        starts.append(len(lists))
        requests += [starts[-1] + int(q) for q in c.requests]
        for q in range(c.nq):
            lists.append((c.rows[c.offsets[q]:c.offsets[q + 1]].astype(np.int64) + row0).tolist())
        row0 += c.D
    case = ArrayCase(lists, row0, name)
    case.requests, case.starts = requests, starts
    return case


def mixed_case(C=PASS_ENTRIES, cursors=LIST_CURSORS, **long_kw):
    """EVERY PATH IN ONE LAUNCH: long_windows_case, hot_id_case and three tiny queries side by side over rows of their own.
    The request list interleaves a = 0, a = 1, a = cursors + 1 under windows and halving, the hot-id request with its
    single-id passes of more than C entries, short requests, and repeats, unsorted."""
    long, hot = long_windows_case(C=C, cursors=cursors, **long_kw), hot_id_case(C=C)
    tiny = ArrayCase([[0], [0, 1], [1], []], 2, "tiny")
    tiny.requests = [0, 3]
    case = concat_cases([long, hot, tiny], "mixed C=%d" % C)
    l0, h0, t0 = case.starts
    base = l0 + long.requests[0]
    a513, hot0, one, none = base + 3, h0, t0, t0 + 3
    case.requests = [none, a513, one, hot0, l0, base + 10, a513, h0 + 30, base, one, hot0, h0 + 19, none, base + 2]
    sizes = np.diff(case.offsets)
    assert (sizes[none], sizes[one], sizes[a513], sizes[l0]) == (0, 1, cursors + 1, 0) and sizes[hot0] == C + 8
    plan = plan_ref(case, a513, C)
    assert len(_busy(plan)) >= 3 and sum(p[3] for p in plan) >= 1 and all(p[2] <= C for p in plan)
    single = [p for p in plan_ref(case, hot0, C) if p[2] > C]
    assert len(single) == 4 and all(p[1] - p[0] == 1 for p in single)
    assert len(set(case.requests)) < len(case.requests) and case.requests != sorted(case.requests)
    return case
