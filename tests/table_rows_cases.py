"""The row operations of qrlsh.LiveTable (csrc/tablerows.hip) restated in numpy (test infrastructure only), and the shapes
their tests run on.

A table row lives in a slot: slot s owns row s of the permutation table (tab [slots, P] = perms.T) and its cells are value
ids (one id per (feature, value)).  A query is nfeat value ids, -1 = unconstrained, and matches a row iff every constrained
feature holds the row's id.  The claim under test: after rows come or go, the signatures are those of MinHash over the
answer sets of the edited table in slot numbering under the same permutation table."""
import numpy as np


# ---- restatements ------------------------------------------------------------------------------------------------------
def matches(qrows, cells):
    """bool [n, m]: query q matches row j"""
    q = np.asarray(qrows, dtype=np.int64)[:, None, :]
    c = np.asarray(cells, dtype=np.int64)[None, :, :]
    return ((q == -1) | (q == c)).all(axis=2)


def brute_answer_sets(cells, qrows, live=None):
    """CSR (offsets int64 [n + 1], rows int32): the live slots every query matches, ascending"""
    ok = matches(qrows, cells)
    if live is not None:
        ok &= np.asarray(live, dtype=bool)[None, :]
    sizes = ok.sum(axis=1)
    offsets = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    return offsets, np.nonzero(ok)[1].astype(np.int32)


def minhash(offsets, rows, tab):
    """sig int32 [n, P]: min over the answer set of tab[slot][p], -1 when empty (tab [slots, P])"""
    n = len(offsets) - 1
    sig = np.full((n, tab.shape[1]), -1, dtype=np.int32)
    for q in range(n):
        r = rows[offsets[q]:offsets[q + 1]]
        if len(r):
            sig[q] = tab[r].min(axis=0)
    return sig


def restate_add(sig, qrows, cells, tab_rows):
    """the batch (cells [m, nfeat], tab_rows [m, P] = the table rows of their slots) is added: -> (ids of the queries whose
    row changes, ascending; their new rows int32).  The comparison is unsigned: -1 loses to every value."""
    ok = matches(qrows, cells)
    old = np.asarray(sig, dtype=np.int64) & 0xFFFFFFFF
    t = np.asarray(tab_rows, dtype=np.int64)
    new = old.copy()
    for q in np.nonzero(ok.any(axis=1))[0]:
        new[q] = np.minimum(old[q], t[ok[q]].min(axis=0))
    ids = np.nonzero((new != old).any(axis=1))[0]
    return ids, new[ids].astype(np.uint32).view(np.int32).reshape(len(ids), old.shape[1])


def restate_remove(sig, qrows, cells, tab_rows):
    """the batch leaves: -> ids of the queries that have a matched row holding one of their values (ascending)"""
    ok = matches(qrows, cells)
    s = np.asarray(sig, dtype=np.int64)
    t = np.asarray(tab_rows, dtype=np.int64)
    hit = np.zeros(len(s), dtype=bool)
    for q in np.nonzero(ok.any(axis=1))[0]:
        hit[q] = (t[ok[q]] == s[q][None, :]).any()
    return np.nonzero(hit)[0]


def matched_count(qrows, cells):
    return int(matches(qrows, cells).any(axis=1).sum())


# ---- the string form the oracle reads ----------------------------------------------------------------------------------
def as_strings(ids):
    """value ids -> the cells / query values of the string form ("" = unconstrained)"""
    a = np.asarray(ids)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for k, v in enumerate(a.reshape(-1).tolist()):
        flat[k] = "" if v == -1 else "v%d" % v
    return out


def oracle_signatures(cells, qrows, perms, live=None):
    """oracle.minhash over oracle.answer_sets of the table's string form (slot numbering; dead slots dropped from the sets)"""
    from oracle import oracle as O
    c = as_strings(cells).astype(str)
    off, rows = O.answer_sets([c[:, f] for f in range(c.shape[1])], as_strings(qrows).astype(str))
    if live is not None:
        keep = np.asarray(live, dtype=bool)[rows]
        owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
        rows = rows[keep]
        off = np.concatenate(([0], np.cumsum(np.bincount(owner[keep], minlength=len(off) - 1)))).astype(np.int64)
    return O.minhash(off, rows, perms), off, rows


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case:
    """D rows in slots 0 .. D-1, m more in D .. D+m-1 (the batch of an addition); n queries; perms [P, cap], tab = perms.T.
    Special queries: ALL (all unconstrained), EMPTY (names a value only batch row 0 holds: an empty answer set that the
    addition fills, -1 to values) and, when m >= 2, QUIET (names a value held by slot 0 and by the last batch row only, whose
    hand-made table row exceeds slot 0's everywhere: it matches and must not be listed)."""
    ALL, EMPTY, QUIET = 0, 1, 2

    def __init__(self, n, nfeat, nvals, P, D, m, seed):
        rng = np.random.default_rng(seed)
        self.n, self.nfeat, self.P, self.D, self.m = n, nfeat, P, D, m
        self.cap = cap = D + m + 3
        base = 1 + np.arange(nfeat) * (nvals + 2)                 # ids of feature f: base[f] .. base[f] + nvals + 1
        cells = (rng.integers(0, nvals, size=(D + m, nfeat)) + base).astype(np.int32)
        qrows = (rng.integers(0, nvals, size=(n, nfeat)) + base).astype(np.int32)
        qrows[rng.random((n, nfeat)) < 0.5] = -1
        perms = np.stack([rng.permutation(cap) for _ in range(P)]).astype(np.int32)
        self.quiet = m >= 2
        qrows[self.ALL] = -1
        new_a, new_b = base[0] + nvals, base[nfeat - 1] + nvals + 1
        cells[D, 0] = new_a                                       # only batch row 0 holds it
        qrows[self.EMPTY] = -1
        qrows[self.EMPTY, 0] = new_a
        if self.quiet:
            cells[0, nfeat - 1] = cells[D + m - 1, nfeat - 1] = new_b
            qrows[self.QUIET] = -1
            qrows[self.QUIET, nfeat - 1] = new_b
            perms[:, D + m - 1] = cap + 5                         # hand-made: above every value of the table
        self.cells, self.qrows, self.perms = cells, qrows, perms
        self.tab = np.ascontiguousarray(perms.T)
        self.slots = np.arange(D, D + m, dtype=np.int32)
        live = np.zeros(D + m, dtype=bool)
        live[:D] = True
        self.sig = minhash(*brute_answer_sets(cells, qrows, live), self.tab)      # before the addition
        self.sig_after = minhash(*brute_answer_sets(cells, qrows), self.tab)     # with all D + m rows

    def batch(self):
        return self.cells[self.D:], self.slots, self.tab[self.D:self.D + self.m]

    def removal(self, keep_slot0=True, count=7, seed=0):
        """slots that leave the full table of D + m rows: random ones and, when there is a QUIET query, the hand-made row"""
        rng = np.random.default_rng(seed)
        lo = 1 if keep_slot0 else 0
        s = set(rng.choice(np.arange(lo, self.D + self.m), min(count, self.D + self.m - lo), replace=False).tolist())
        if self.quiet:
            s.add(self.D + self.m - 1)
        if not keep_slot0:
            s.add(0)
        return np.array(sorted(s), dtype=np.int32)


TILE_EDGES = (1, 63, 64, 65, 130)


def host_cases():
    """small: every special, both removals"""
    return [Case(n=97, nfeat=3, nvals=3, P=12, D=40, m=m, seed=100 + m) for m in (1, 2, 5, 65)] + \
           [Case(n=50, nfeat=1, nvals=4, P=8, D=30, m=4, seed=7), Case(n=50, nfeat=63, nvals=2, P=8, D=30, m=4, seed=8)]


# ---- end to end: a table of strings ------------------------------------------------------------------------------------
def string_table(N, D, extra, nfeat=3, nvals=4, seed=21):
    """-> (columns: nfeat arrays of D + extra cells, queries [N, nfeat] with "" = unconstrained).  Query 0, and no
    other, is all unconstrained; row D - 1 alone holds "only" in feature 0 and query 1 names it (it loses its last row when the row goes);
    row D (the first to be added) holds "fresh" in feature 1, a value no row before it and no served query holds."""
    rng = np.random.default_rng(seed)
    cells = np.array([["f%dv%d" % (f, v) for f, v in enumerate(r)] for r in rng.integers(0, nvals, size=(D + extra, nfeat))],
                     dtype=object)
    q = np.array([["f%dv%d" % (f, v) for f, v in enumerate(r)] for r in rng.integers(0, nvals, size=(N, nfeat))], dtype=object)
    q[rng.random((N, nfeat)) < 0.5] = ""
    blank = (q == "").all(axis=1)
    q[blank, nfeat - 1] = "f%dv0" % (nfeat - 1)          # query 0 alone is all unconstrained
    q[0] = ""
    cells[D - 1, 0] = "only"
    q[1] = ""
    q[1, 0] = "only"
    if extra:
        cells[D, 1] = "fresh"
    return [cells[:, f].copy() for f in range(nfeat)], q
