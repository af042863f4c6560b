"""The removal contract of qrlsh.QueryIndex.remove restated in numpy (test infrastructure only), and its removal sets.

Queries R leave 0 .. n-1 and the survivors are renumbered by rank (a monotone map).
  layout: a built band filtered in place order, ids remapped, is the band a fresh build of the survivors' keys gives.
  lists:  a stored row with fewer than K entries was never cut: it drops its removed entries and is renumbered.  A
          surviving row of exactly K entries that loses at least one is computed again among the survivors -- only such
          a row is; every other row comes from the stored lists alone."""
import numpy as np

import index_append_cases as AC
import query_index_cases as QC


def new_positions(n, removed):
    """int64 [n]: the new id of every old id, -1 for a removed one"""
    gone = np.zeros(n, dtype=bool)
    gone[np.asarray(removed, dtype=np.int64)] = True
    pos = np.cumsum(~gone) - 1
    pos[gone] = -1
    return pos.astype(np.int64)


def restate_remove_layout(layout, removed):
    """layout: restate_layout's triple of n queries; removed: their ids that leave -> the triple of the survivors:
    every band filtered in place order, ids remapped, the directory over dir_bits(n') bits"""
    sk, ids, _ = layout
    b, n = sk.shape
    pos = new_positions(n, removed)
    left = int((pos >= 0).sum())
    d = AC.dir_bits(left)
    ok = np.empty((b, left), dtype=np.uint64)
    oi = np.empty((b, left), dtype=np.uint32)
    dirw = np.empty((b, (1 << d) + 1), dtype=np.uint32)
    for t in range(b):
        stay = pos[ids[t].astype(np.int64)] >= 0
        ok[t], oi[t] = sk[t][stay], pos[ids[t][stay].astype(np.int64)]
        dirw[t] = AC._directory(ok[t], d)
    return ok, oi, dirw.reshape(-1)


def restate_remove_lists(lists, sig, removed, b, K):
    """lists: the stored (src, dst, val) of a run over sig's rows at K -> ((src, dst, val) int32 after the removal,
    picked old row ids ascending).  Unpicked rows use the stored lists alone; a picked row (exactly K stored entries, at
    least one of them removed, itself surviving) is probed again among the surviving rows."""
    src, dst, val = (np.asarray(a, dtype=np.int64) for a in lists)
    sig = np.asarray(sig)
    n = sig.shape[0]
    pos = new_positions(n, removed)
    stay = np.nonzero(pos >= 0)[0]
    rows = sig[stay]
    length = np.bincount(src, minlength=n)
    lost = np.bincount(src[pos[dst] < 0], minlength=n)
    picked = np.nonzero((length == K) & (lost > 0) & (pos >= 0))[0]
    is_picked = np.zeros(n, dtype=bool)
    is_picked[picked] = True
    keep = (pos[src] >= 0) & (pos[dst] >= 0) & ~is_picked[src]
    S, D, V = [pos[src[keep]]], [pos[dst[keep]]], [val[keep]]
    for p in picked:
        ids = QC.restate_candidates(rows, b, sig[p])
        ids = ids[ids != pos[p]]
        mi = QC.restate_scores(rows, ids, sig[p])
        order = np.lexsort((ids, -mi))[:K]
        S.append(np.full(len(order), pos[p], dtype=np.int64))
        D.append(ids[order])
        V.append(mi[order])
    S, D, V = np.concatenate(S), np.concatenate(D), np.concatenate(V)
    # rows are disjoint: ordering by new src alone, stably, keeps every row's own order
    order = np.argsort(S, kind="stable")
    return (S[order].astype(np.int32), D[order].astype(np.int32), V[order].astype(np.int32)), picked


def short_rows_that_lose(lists, n, removed, K):
    """surviving stored rows with fewer than K entries that lose at least one"""
    src, dst = (np.asarray(a, dtype=np.int64) for a in lists[:2])
    pos = new_positions(n, removed)
    length = np.bincount(src, minlength=n)
    lost = np.bincount(src[pos[dst] < 0], minlength=n)
    return int(((length < K) & (lost > 0) & (pos >= 0)).sum())


def removal_sets(n=340, seed=21):
    """name -> ids as given to remove (the random set shuffled and with duplicates)"""
    rng = np.random.default_rng(seed)
    r40 = rng.choice(n, 40, replace=False)
    given = np.concatenate((r40, r40[:7]))
    rng.shuffle(given)
    return {"first": np.array([0]), "last": np.array([n - 1]), "tail40": np.arange(n - 40, n),
            "even": np.arange(0, n, 2), "all_but_0": np.arange(1, n), "all": np.arange(n), "random40": given}


# the issue's table: (hi, set) -> picked rows, at K = 4, b = 8 on lists_update_cases.crowded(hi)
PICKED = {(3, "first"): 7, (3, "last"): 2, (3, "tail40"): 109, (3, "even"): 153,
          (40, "first"): 2, (40, "tail40"): 9, (40, "even"): 12}
SHORT_LOST = {(40, "first"): 1, (40, "tail40"): 37, (40, "even"): 82}
