"""Numpy restatements and inputs for the live user lists (qrlsh.UserLists, csrc/userlists.hip).

reference_lists(): the lists of qrlsh.users.user_similarities from first principles -- integer-truncated centring,
exact int64 dots, float64 cosine, rint(1000 cos), positive values only, value descending then id ascending, cut at K.
restated_update(): the update rule of userlists.hip step by step (mark, rescore S = R + picked, merge the rest).
Lists are dense: idx int32 [nu][K] (-1 past the end), milli int32 [nu][K] (0 past the end), len int32 [nu]."""
import numpy as np


def centred(ratings):
    """x == 0 ? 0 : (int)((double)x - mean), mean = (double)sum / (double)count over the non-zero ratings"""
    r = np.asarray(ratings).astype(np.int64)
    out = np.zeros_like(r)
    for u in range(r.shape[0]):
        nz = r[u] != 0
        if nz.any():
            mean = float(r[u][nz].sum()) / float(nz.sum())
            out[u][nz] = (r[u][nz].astype(np.float64) - mean).astype(np.int64)   # float64 -> int truncates toward zero
    return out


def milli_matrix(c):
    """c: centred rows int64 [m][nq] -> int32 [m][m]: rint(1000 * dot / (sqrt(na) * sqrt(nb))), 0 where a norm is 0"""
    dot = c @ c.T
    n2 = np.diag(dot).copy()
    den = np.sqrt(n2.astype(np.float64))[:, None] * np.sqrt(n2.astype(np.float64))[None, :]
    ok = (n2[:, None] != 0) & (n2[None, :] != 0)
    cs = np.zeros(dot.shape, dtype=np.float64)
    cs[ok] = dot[ok].astype(np.float64) / den[ok]
    return np.rint(cs * 1000.0).astype(np.int32)


def pair_milli(ratings, pairs):
    """the scores of explicit (a, b) pairs, for the pair-kernel tests"""
    c = centred(ratings)
    n2 = (c * c).sum(axis=1)
    out = np.zeros(len(pairs), dtype=np.int32)
    for i, (a, b) in enumerate(pairs):
        if n2[a] and n2[b]:
            out[i] = np.int32(np.rint(float(c[a] @ c[b]) / (np.sqrt(float(n2[a])) * np.sqrt(float(n2[b]))) * 1000.0))
    return out


def empty_lists(nu, K):
    return (np.full((nu, K), -1, dtype=np.int32), np.zeros((nu, K), dtype=np.int32), np.zeros(nu, dtype=np.int32))


def _put(lists, u, cand, K):
    """cand: [(milli, id)] -> row u = the first K by (milli descending, id ascending) of the positive ones"""
    idx, mil, ln = lists
    best = sorted(((m, i) for m, i in cand if m > 0), key=lambda t: (-t[0], t[1]))[:K]
    idx[u], mil[u] = -1, 0
    for k, (m, i) in enumerate(best):
        idx[u, k], mil[u, k] = i, m
    ln[u] = len(best)


def ranked_candidates(ratings, labels):
    """{u: [(milli, id)] every positive neighbour of its cluster, in list order, uncut}"""
    labels = np.asarray(labels)
    c = centred(ratings)
    out = {}
    for lab in np.unique(labels):
        mem = np.flatnonzero(labels == lab)
        mm = milli_matrix(c[mem])
        for a, u in enumerate(mem):
            cand = [(int(mm[a, b]), int(v)) for b, v in enumerate(mem) if b != a and mm[a, b] > 0]
            out[int(u)] = sorted(cand, key=lambda t: (-t[0], t[1]))
    return out


def reference_lists(ratings, labels, K):
    labels = np.asarray(labels)
    nu = np.asarray(ratings).shape[0]
    idx, mil, ln = empty_lists(nu, K)
    c = centred(ratings)
    for lab in np.unique(labels):
        mem = np.flatnonzero(labels == lab)
        mm = milli_matrix(c[mem])
        np.fill_diagonal(mm, 0)
        for a, u in enumerate(mem):
            order = np.lexsort((mem, -mm[a].astype(np.int64)))      # value descending, then id ascending
            order = order[mm[a][order] > 0][:K]
            idx[u, :len(order)], mil[u, :len(order)], ln[u] = mem[order], mm[a][order], len(order)
    return idx, mil, ln


def restated_update(lists, new_ratings, labels, K, R):
    """lists: the stored lists (of the matrix before the edits); R: the rows that were edited.
    -> (the lists afterwards, the picked rows), by the rule of userlists.hip:
      picked = rows outside R with exactly K entries, one of them in R;  S = R + picked;
      a row of S: the first K of its positive scores against its whole cluster;
      another row of a touched cluster: the first K of the merge of its entries outside R with the positive
      (milli(r, v), r) of its cluster's r in R;  every other row: untouched."""
    labels = np.asarray(labels)
    idx, mil, ln = (a.copy() for a in lists)
    Rset = set(int(r) for r in R)
    nu = len(labels)
    picked = [v for v in range(nu) if v not in Rset and ln[v] == K and any(int(d) in Rset for d in idx[v, :K])]
    S = Rset | set(picked)
    c = centred(new_ratings)
    out = (idx, mil, ln)
    for lab in set(int(labels[r]) for r in Rset):
        mem = np.flatnonzero(labels == lab)
        mm = milli_matrix(c[mem])
        for a, v in enumerate(mem):
            v = int(v)
            if v in S:
                cand = [(int(mm[a, b]), int(w)) for b, w in enumerate(mem) if b != a]
            else:
                cand = [(int(mil[v, k]), int(idx[v, k])) for k in range(ln[v]) if int(idx[v, k]) not in Rset]
                cand += [(int(mm[a, b]), int(w)) for b, w in enumerate(mem) if int(w) in Rset]
            _put(out, v, cand, K)
    return out, picked


def from_coo(src, dst, val, nu, K):
    """users.user_similarities' COO (numpy) -> the dense form"""
    lists = empty_lists(nu, K)
    idx, mil, ln = lists
    for s, d, m in zip(src.tolist(), dst.tolist(), val.tolist()):
        idx[s, ln[s]], mil[s, ln[s]] = d, m
        ln[s] += 1
    return lists


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- cases
def _like_minded(rng, n, nq, noise=1, fill=0.7):
    """n users around one taste: pairwise similarities clearly positive"""
    proto = rng.integers(1, 6, size=nq) * 20
    r = proto[None, :] + rng.integers(-noise * 10, noise * 10 + 1, size=(n, nq))
    r = np.clip(r, 1, 100)
    r[rng.random((n, nq)) > fill] = 0
    return r.astype(np.int64)


def _random(rng, n, nq, fill=0.5):
    return (rng.integers(1, 101, size=(n, nq)) * (rng.random((n, nq)) < fill)).astype(np.int64)


def _case(ratings, labels, K, edits):
    u, q, v = (np.asarray(x, dtype=np.int64) for x in zip(*edits))
    new = np.array(ratings, copy=True)
    new[u, q] = v
    return {"ratings": np.asarray(ratings, dtype=np.int64), "labels": np.asarray(labels, dtype=np.int64), "K": K,
            "edits": (u, q, v), "new": new, "R": np.unique(u)}


def _flip(r, u):
    """edits that turn user u's taste upside down: every rated cell x -> 101 - x"""
    return [(u, int(q), int(101 - r[u, q])) for q in np.flatnonzero(r[u])]


def build_cases():
    """name -> {ratings, labels, K, edits (u, q, v), new, R}; test_user_lists_host pins the property each is named for"""
    rng = np.random.default_rng(20240)
    nq = 37
    cases = {}
    r = _random(rng, 1, nq)
    cases["one_user"] = _case(r, [0], 3, [(0, 4, 55), (0, 5, 0)])
    r = _like_minded(rng, 2, nq)
    cases["two_users_one_cluster"] = _case(r, [7, 7], 3, [(1, 0, 100), (1, 3, 1)])
    r = np.vstack((_like_minded(rng, 5, nq), _like_minded(rng, 4, nq)))
    cases["cluster_smaller_than_K"] = _case(r, [0] * 5 + [1] * 4, 8, [(2, 1, 90), (2, 2, 0), (2, 9, 13)])
    K = 5
    r = np.vstack((_like_minded(rng, K + 1, nq), _random(rng, 3, nq)))
    cases["cluster_of_K_plus_1"] = _case(r, [3] * (K + 1) + [9] * 3, K, [(0, 0, 5), (4, 7, 95), (4, 8, 0)])
    # equal values at the cut: users 1 .. 6 hold the same row, so everybody sees them tied
    r = _like_minded(rng, 9, nq)
    r[1:7] = r[1]
    cases["ties_at_the_cut"] = _case(r, [0] * 9, 3, [(0, 2, 77), (4, 5, 11), (4, 6, 0), (8, 1, 50)])
    r = _like_minded(rng, 8, nq)
    cases["full_row_loses_an_entry"] = _case(r, [0] * 8, 4, _flip(r, 2))
    r = np.vstack((_like_minded(rng, 3, nq), _like_minded(rng, 3, nq)))
    edits = _flip(r, 0)                                         # similarities of user 0 turn negative
    edits += [(4, int(q), 0) for q in np.flatnonzero(r[4])[1:]]  # user 4 keeps one rating: its centred row is zero
    cases["similarity_turns_zero_or_negative"] = _case(r, [0] * 3 + [1] * 3, 4, edits)
    r = _like_minded(rng, 6, nq)
    cases["row_unrated_to_zeros"] = _case(r, [0] * 6, 3, [(3, int(q), 0) for q in np.flatnonzero(r[3])])
    r = np.vstack((_like_minded(rng, 4, nq), _like_minded(rng, 7, nq)))
    cases["R_is_a_whole_cluster"] = _case(r, [0] * 4 + [1] * 7, 3, [(u, u + 1, 10 * u + 7) for u in range(4)])
    r = np.vstack((_like_minded(rng, 6, nq), _like_minded(rng, 5, nq), _random(rng, 2, nq)))
    lab = [0] * 6 + [1] * 5 + [2, 3]
    cases["R_is_all_users"] = _case(r, lab, 4, [(u, (3 * u) % nq, 1 + (17 * u) % 100) for u in range(13)])
    cases["two_clusters_at_once"] = _case(r, lab, 4, _flip(r, 1) + _flip(r, 8) + [(12, 0, 3)])
    # repeats inside one list of edits are the host layer's business; the cases keep cells distinct
    nu = 150
    r = np.vstack((_like_minded(rng, 80, nq, noise=2), _random(rng, 70, nq)))
    lab = np.concatenate((np.zeros(80, dtype=np.int64), 1 + rng.integers(0, 9, size=70)))
    perm = rng.permutation(nu)                                  # clusters interleaved in id order
    r, lab = r[perm], lab[perm]
    who = rng.choice(nu, size=10, replace=False)
    edits = [(int(u), int(rng.integers(0, nq)), int(rng.integers(0, 101))) for u in who]
    edits += _flip(r, int(np.flatnonzero(lab == 0)[3]))
    edits = list({(u, q): (u, q, v) for u, q, v in edits}.values())
    for K in (1, 19, 64):
        cases["mixed_K%d" % K] = _case(r, lab, K, edits)
    return cases


def big_cluster_case():
    """one cluster of 1 500 users at nq = 64: the selection works through 24 chunks of candidates per rescored row, and
    70 changed users reach every other row in two chunks"""
    rng = np.random.default_rng(1500)
    nu, nq = 1500, 64
    r = _like_minded(rng, nu, nq, noise=3, fill=0.5)
    who = rng.choice(nu, size=70, replace=False)
    edits = [(int(u), int(rng.integers(0, nq)), int(rng.integers(0, 101))) for u in who]
    edits += _flip(r, int(who[0]))
    edits = list({(u, q): (u, q, v) for u, q, v in edits}.values())
    return _case(r, np.zeros(nu, dtype=np.int64), 19, edits)


def no_tie_straddles_the_cut(ratings, labels, K):
    """the precondition of a comparison with an arbitrary tie order: no user's K-th and (K+1)-th positive candidates
    hold the same value"""
    return all(len(c) <= K or c[K - 1][0] != c[K][0] for c in ranked_candidates(ratings, labels).values())
