"""Changing the list length of stored lists (QueryIndex.set_list_length, UserLists.set_list_length) restated in numpy
(test infrastructure only), and the counts its tests pin.

Query lists are COO src / dst / val ordered by (src, value descending, dst ascending), at most K per src.
  cut:    entry i survives a cut to K2 exactly when i < K2 or src[i - K2] != src[i] -- a predicate on src alone.
  regrow: the rows of exactly K_old entries (picked) are the only ones the cut at K_old can have shortened; they take
          their rows of the oracle's lists at K2, every other row stays as stored.
User lists are dense: idx / milli int32 [nu][K] (-1 / 0 past a row's end), len int32 [nu]."""
import numpy as np

import lists_update_cases as LC
import user_lists_cases as UC


# ---- query lists --------------------------------------------------------------------------------------------------
def cut_mask(src, K2):
    src = np.asarray(src)
    i = np.arange(len(src))
    keep = i < K2
    keep[K2:] |= src[K2:] != src[:len(src) - K2] if len(src) > K2 else False
    return keep


def restate_cut(lists, K2):
    keep = cut_mask(lists[0], K2)
    return tuple(np.asarray(a, dtype=np.int32)[keep] for a in lists)


def full_rows(src, K_old):
    """the ids of the rows of exactly K_old entries, ascending: entry i heads one iff it is a run head and
    src[i + K_old - 1] == src[i]"""
    src = np.asarray(src)
    i = np.arange(len(src))
    head = np.ones(len(src), dtype=bool)
    head[1:] = src[1:] != src[:-1]
    last = i + K_old - 1
    ok = head & (last < len(src))
    ok[ok] = src[last[ok]] == src[ok]
    return src[ok].astype(np.int64)


def restate_regrow(lists, sig, b, K_old, K2):
    """-> (lists at K2, picked rows): unpicked rows from the stored lists, picked rows from the oracle's lists at K2"""
    picked = full_rows(lists[0], K_old)
    full = LC.full_lists(sig, b, K2)
    stay = ~np.isin(lists[0], picked)
    take = np.isin(full[0], picked)
    src, dst, val = (np.concatenate((np.asarray(a)[stay], np.asarray(f)[take])) for a, f in zip(lists, full))
    return LC.cut(src, dst, val, K2), picked


# measured on LC.crowded(hi) (N = 340, P = 16, b = 8): (hi, K_old, K_new) -> (rows picked, entries before, after)
REGROWS = {
    (3, 4, 5): (323, 1292, 1615),          # every row is full at every K <= 64
    (3, 4, 256): (323, 1292, 61960),       # longest row 219: none full afterwards
    (3, 64, 256): (323, 20672, 61960),
    (40, 4, 6): (27, 521, 530),            # 236 short rows stay as stored
    (40, 2, 6): (158, 421, 530),
    (40, 1, 4): (263, 263, 521),
    (40, 64, 256): (0, 530, 530),
}
CUT_ENTRIES_40 = {4: 521, 3: 494, 2: 421, 1: 263}     # crowded(40); crowded(3): K * 323 for every K <= 64


# ---- user lists ---------------------------------------------------------------------------------------------------
def user_cut(lists, K2):
    idx, mil, ln = lists
    return idx[:, :K2].copy(), mil[:, :K2].copy(), np.minimum(ln, K2).astype(np.int32)


def user_full_rows(lists, K_old):
    return np.flatnonzero(lists[2] == K_old)


def user_regrow(lists, ratings, labels, K_old, K2):
    """-> (lists at K2, rows rescored): the stored rows at the new stride, the full rows from reference_lists at K2"""
    idx, mil, ln = lists
    nu = len(ln)
    out = UC.empty_lists(nu, K2)
    out[0][:, :K_old], out[1][:, :K_old], out[2][:] = idx, mil, ln
    full = user_full_rows(lists, K_old)
    ref = UC.reference_lists(ratings, labels, K2)
    for a, r in zip(out, ref):
        a[full] = r[full]
    return out, full


# UC.build_cases(): name -> (full rows, short rows) at the case's own K
USER_FULL = {"mixed_K19": (80, 68), "ties_at_the_cut": (9, 0), "cluster_smaller_than_K": (0, 9), "mixed_K1": (148, 0)}


def user_targets(K):
    """the lengths every case is taken to: cuts to 1 and K - 1, regrows to K + 1, K + 3 and 64"""
    return sorted({k for k in (1, K - 1) if 1 <= k < K}), sorted({k for k in (K + 1, K + 3, 64) if K < k <= 64})
