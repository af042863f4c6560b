"""The replacement contract of qrlsh.QueryIndex.replace restated in numpy (test infrastructure only), and its cases.

Queries R of 0 .. n-1 take new rows and keep their ids; n, b and every other id stay.
  layout: a band is ordered by (top 32 bits of mix64(key), id).  The band after the replacement is the old band without
          the records of R, merged with the batch records sorted by (bits, id): a new record goes among the records of
          equal bits by its id, not behind them.
  lists:  from the stored lists alone, except for the rows that are probed:
            row i outside R, fewer than K stored entries: it drops its entries with dst in R, merges with the replaced
              queries that now name it and is cut at K;
            row i outside R, exactly K stored entries, none with dst in R: the same merge;
            row i outside R, exactly K stored entries, at least one with dst in R: picked -- probed again;
            row r in R: probed with its new row, itself excluded.
          Ties in the merge go by id, both ways."""
import numpy as np

import index_append_cases as AC
import lists_update_cases as LC
import query_index_cases as QC
from bucket_cases import np_mix64


def _composite(keys, ids):
    return (np_mix64(keys) >> np.uint64(32)) << np.uint64(32) | ids.astype(np.uint64)


def restate_replace_layout(layout, ids, batch_keys):
    """layout: restate_layout's triple of n queries; ids: m distinct ids in any order; batch_keys [b][m] (uint64, or
    int64 bit patterns): column x holds the new keys of ids[x] -> the triple after the replacement.  Written as the
    device does it: batch record j, in (bits, id) order, lands at (survivors that order before it) + j."""
    sk, si, _ = layout
    b, n = sk.shape
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    bk = np.ascontiguousarray(batch_keys).view(np.uint64).reshape(b, len(ids))
    by_id = np.argsort(ids, kind="stable")
    rid = ids[by_id]
    gone = np.zeros(n, dtype=bool)
    gone[rid] = True
    d = AC.dir_bits(n)
    ok = np.empty((b, n), dtype=np.uint64)
    oi = np.empty((b, n), dtype=np.uint32)
    dirw = np.empty((b, (1 << d) + 1), dtype=np.uint32)
    for t in range(b):
        stay = ~gone[si[t].astype(np.int64)]
        keys_s, ids_s = sk[t][stay], si[t][stay]
        kb = bk[t][by_id]
        cb = _composite(kb, rid)
        order = np.argsort(cb, kind="stable")
        at = np.searchsorted(_composite(keys_s, ids_s), cb[order], side="left") + np.arange(len(rid))
        new = np.zeros(n, dtype=bool)
        new[at] = True
        ok[t][new], oi[t][new] = kb[order], rid[order]
        ok[t][~new], oi[t][~new] = keys_s, ids_s
        dirw[t] = AC._directory(ok[t], d)
    return ok, oi, dirw.reshape(-1)


def overwritten(sig_old, ids, sig_new):
    rows = np.array(sig_old, dtype=np.int32, copy=True)
    rows[np.asarray(ids, dtype=np.int64)] = np.asarray(sig_new, dtype=np.int32)
    return rows


def _probe(rows, b, q, K):
    ids = QC.restate_candidates(rows, b, rows[q])
    ids = ids[ids != q]
    mi = QC.restate_scores(rows, ids, rows[q])
    return ids, mi, np.lexsort((ids, -mi))[:K]


def _row_facts(stored, n, ids, K):
    src, dst = (np.asarray(a, dtype=np.int64) for a in stored[:2])
    in_r = np.zeros(n, dtype=bool)
    in_r[np.asarray(ids, dtype=np.int64)] = True
    length = np.bincount(src, minlength=n)
    lost = np.bincount(src[in_r[dst]], minlength=n)
    return in_r, length, lost


def restate_replace_lists(stored, sig_old, ids, sig_new, b, K):
    """stored: the (src, dst, val) of a run over sig_old at K; rows ids of sig_old become sig_new -> ((src, dst, val)
    int32 afterwards, picked row ids ascending).  The four row rules, literally: only rows of R and picked rows are
    probed (among the new rows); every other row comes from its stored entries and the probes of R."""
    src, dst, val = (np.asarray(a, dtype=np.int64) for a in stored)
    n = np.asarray(sig_old).shape[0]
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    rows = overwritten(sig_old, ids, sig_new)
    in_r, length, lost = _row_facts(stored, n, ids, K)
    picked = np.nonzero((length == K) & (lost > 0) & ~in_r)[0]
    probed = in_r.copy()
    probed[picked] = True
    keep = ~probed[src] & ~in_r[dst]
    S, D, V = [src[keep]], [dst[keep]], [val[keep]]
    for q in np.nonzero(probed)[0]:
        cand, mi, best = _probe(rows, b, q, K)
        S.append(np.full(len(best), q, dtype=np.int64))
        D.append(cand[best])
        V.append(mi[best])
        if in_r[q]:      # the replaced query enters the rows that are not probed themselves
            back = ~probed[cand]
            S.append(cand[back])
            D.append(np.full(int(back.sum()), q, dtype=np.int64))
            V.append(mi[back])
    return LC.cut(np.concatenate(S), np.concatenate(D), np.concatenate(V), K), picked


def branch_counts(stored, sig_old, ids, sig_new, b, K):
    """(picked rows, short rows outside R that lose an entry, unpicked rows outside R that gain a replaced neighbour at
    a tie with a surviving stored entry of larger id)"""
    src, dst, val = (np.asarray(a, dtype=np.int64) for a in stored)
    n = np.asarray(sig_old).shape[0]
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    rows = overwritten(sig_old, ids, sig_new)
    in_r, length, lost = _row_facts(stored, n, ids, K)
    picked = (length == K) & (lost > 0) & ~in_r
    short = (length < K) & (lost > 0) & ~in_r
    tied = np.zeros(n, dtype=bool)
    for q in ids:
        cand, mi, _ = _probe(rows, b, q, K)
        for i, v in zip(cand, mi):
            if in_r[i] or picked[i]:
                continue
            mine = (src == i) & ~in_r[dst]
            if ((val[mine] == v) & (dst[mine] > q)).any():
                tied[i] = True
    return int(picked.sum()), int(short.sum()), int(tied.sum())


def replacement_sets(N, seed=23):
    """name -> (ids as given to replace, kind, source ids): kind "fresh" = new random rows, "self" = the rows the ids
    hold already, "copy" = copies of the rows `source` (indexed rows outside ids: the new record lands inside a run of
    equal keys, with smaller and larger ids on both sides of it)"""
    rng = np.random.default_rng(seed)
    r40 = rng.choice(N, 40, replace=False)      # shuffled: no order among them
    own = rng.choice(N, 30, replace=False)
    mid = np.arange(N // 3, N // 3 + 25)
    rng.shuffle(mid)
    others = np.setdiff1d(np.arange(N), mid)
    return {"first": (np.array([0]), "fresh", None), "last": (np.array([N - 1]), "fresh", None),
            "random40": (r40, "fresh", None), "even": (np.arange(0, N, 2), "fresh", None),
            "all": (np.arange(N), "fresh", None), "self": (own, "self", None),
            "copy": (mid, "copy", rng.choice(others, len(mid), replace=False))}


def new_rows(sig, case, seed=29):
    """the replacement rows of a case of replacement_sets, drawn from the value range of sig"""
    ids, kind, source = case
    sig = np.asarray(sig, dtype=np.int32)
    if kind == "self":
        return sig[ids].copy()
    if kind == "copy":
        return sig[source].copy()
    rng = np.random.default_rng(seed + len(ids))
    rows = rng.integers(0, int(sig.max()) + 1, size=(len(ids), sig.shape[1])).astype(np.int32)
    if len(ids) >= 3:
        rows[1] = -1                                  # a query without candidates
        rows[2, :2] = -1                              # an empty band
    return rows


# (hi, case) -> rows, at K = 4, b = 8 on lists_update_cases.crowded(hi); computed by branch_counts on the CPU
PICKED = {(3, "first"): 7, (3, "last"): 2, (3, "random40"): 114, (3, "even"): 153, (3, "all"): 0, (3, "self"): 81,
          (3, "copy"): 78, (40, "first"): 2, (40, "last"): 0, (40, "random40"): 5, (40, "even"): 12, (40, "all"): 0,
          (40, "self"): 6, (40, "copy"): 3}
SHORT_LOST = {(40, "first"): 1, (40, "last"): 3, (40, "random40"): 49, (40, "even"): 82, (40, "self"): 34, (40, "copy"): 25}
TIE_GAINED = {(3, "random40"): 12, (3, "copy"): 35, (40, "copy"): 13}
