"""The list-update contract of qrlsh.QueryIndex.append(update_lists=True) restated in numpy (test infrastructure only),
and the shapes its tests run on.

The lists of a run over queries 0 .. n-1 (COO src / dst / val, by src, value descending, dst ascending, at most K per
src) and m appended queries n .. n+m-1: the updated lists are the stored rows plus every scored pair that has a new
query at one end, in both directions, ordered by (src, value descending, dst ascending) and cut at K per src.  The
claim under test is that this equals the lists of a full run over all n + m queries with the same K."""
import numpy as np

import query_index_cases as QC


def full_lists(sig, b, K):
    """the oracle's lists over all rows: candidates by exact band comparison, scores, top-K"""
    from oracle import oracle as O
    sig = np.ascontiguousarray(sig, dtype=np.int32)
    if sig.shape[0] == 0:
        e = np.empty(0, dtype=np.int32)
        return e, e.copy(), e.copy()
    pairs = O.candidates_from_sig(sig, b)
    return O.topk(pairs, O.score_pairs(sig, pairs), K)


def cut(src, dst, val, K):
    """order by (src, value descending, dst ascending), keep the first K of every src -> int32 arrays"""
    src, dst, val = (np.asarray(a, dtype=np.int64) for a in (src, dst, val))
    order = np.lexsort((dst, -val, src))
    src, dst, val = src[order], dst[order], val[order]
    head = np.ones(len(src), dtype=bool)
    head[1:] = src[1:] != src[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(len(src)), 0))
    keep = np.arange(len(src)) - start < K
    return src[keep].astype(np.int32), dst[keep].astype(np.int32), val[keep].astype(np.int32)


def _buckets(rows, b):
    """per band: (ids ordered by band tuple, the ordered labels, label of every row); label -1 = the empty band"""
    n, P = rows.shape
    L = QC.low16(rows).reshape(n, b, P // b)
    out = []
    for t in range(b):
        lab = np.unique(L[:, t, :], axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
        lab[(L[:, t, :] == 0xFFFF).all(axis=1)] = -1
        order = np.argsort(lab, kind="stable")
        out.append((order, lab[order], lab))
    return out


def new_pairs(sig_all, n, m, b, K=None):
    """every directed edge with a new query (n .. n+m-1) at one end: (src, dst, val) int64, each once.  Candidates by
    band equality after the int16 cast, empty bands skipped (QC.restate_candidates, bucketed once for all queries);
    scores QC.restate_scores.  K: the edges FROM a new query -- all of them are found in its own step -- are cut to its
    K best there (what the final cut would do; a popular key otherwise leaves tens of millions of edges to sort)"""
    S, D, V = [], [], []
    rows = np.asarray(sig_all)[:n + m].astype(np.int64)
    buckets = _buckets(rows, b) if m else []
    for q in range(n, n + m):
        found = [np.empty(0, dtype=np.int64)]
        for order, sl, lab in buckets:
            if lab[q] >= 0:
                found.append(order[np.searchsorted(sl, lab[q], "left"):np.searchsorted(sl, lab[q], "right")])
        ids = np.unique(np.concatenate(found))
        ids = ids[ids != q]
        mi = QC.restate_scores(rows, ids, rows[q])
        old = ids < n
        fwd = np.lexsort((ids, -mi))[:K]
        S += [np.full(len(fwd), q, dtype=np.int64), ids[old]]
        D += [ids[fwd], np.full(int(old.sum()), q, dtype=np.int64)]
        V += [mi[fwd], mi[old]]
    if not S:
        e = np.empty(0, dtype=np.int64)
        return e, e.copy(), e.copy()
    return np.concatenate(S), np.concatenate(D), np.concatenate(V)


def restate_update(lists, sig_all, n, m, b, K):
    """the stored rows plus the scored new pairs, lexsorted by (src, -val, dst), cut at K"""
    s, d, v = new_pairs(sig_all, n, m, b, K)
    return cut(np.concatenate((np.asarray(lists[0], dtype=np.int64), s)),
               np.concatenate((np.asarray(lists[1], dtype=np.int64), d)),
               np.concatenate((np.asarray(lists[2], dtype=np.int64), v)), K)


def restate_batches(lists, sig_all, n, bounds, b, K):
    """restate_update applied batch after batch: bounds = the ascending ends n < e1 < e2 < ... of the batches"""
    for e in bounds:
        lists = restate_update(lists, sig_all, n, e - n, b, K)
        n = e
    return lists


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def rows_cut(sig, b, K):
    """how many rows of the full lists the cut at K shortens"""
    from oracle import oracle as O
    sig = np.ascontiguousarray(sig, dtype=np.int32)
    p = O.u64_to_pairs(O.candidates_from_sig(sig, b))
    deg = np.bincount(p.reshape(-1), minlength=sig.shape[0])
    return int((deg > K).sum()), len(p)


# ---- shapes ------------------------------------------------------------------------------------------------------------
CROWDED = dict(N=340, P=16, b=8, K=4)


def crowded(hi=3, seed=11):
    """N = 340, P = 16, b = 8 (r = 2), values from 0 .. hi-1, 5 % of the rows all -1, every 7th row with an empty first
    band.  hi = 3: nearly every row is cut at K = 4 and ties at the cut are everywhere; hi = 40: sparse, most rows
    shorter than K, rows that only appear with the appended queries."""
    c = CROWDED
    rng = np.random.default_rng(seed)
    sig = rng.integers(0, hi, size=(c["N"], c["P"])).astype(np.int32)
    sig[rng.random(c["N"]) < 0.05] = -1
    sig[::7, :c["P"] // c["b"]] = -1
    return sig


POPULAR = dict(n=100, m=5100, P=8, b=4, K=5, planted=4200)


def popular(seed=12):
    """P = 8, b = 4, 100 old and 5100 new queries over values 0 .. 5; one planted band tuple shared by old ids 0 .. 2
    and 4200 of the new queries: reverse runs beyond 4096 records, new rows whose candidates stream through the select"""
    c = POPULAR
    rng = np.random.default_rng(seed)
    sig = rng.integers(0, 6, size=(c["n"] + c["m"], c["P"])).astype(np.int32)
    who = np.concatenate((np.arange(3), c["n"] + rng.choice(c["m"], c["planted"], replace=False)))
    sig[who, 2:4] = (7, 9)
    return sig


WIDE = dict(N=600, n=500, P=24, b=4, K=6)


def wide(seed=13):
    """P = 24, b = 4 (r = 6: hashed band keys), values from {0, 1}"""
    c = WIDE
    return np.random.default_rng(seed).integers(0, 2, size=(c["N"], c["P"])).astype(np.int32)


def holdouts(N):
    return sorted({1, 3, N // 2, N - 1, N} & set(range(1, N + 1)))
