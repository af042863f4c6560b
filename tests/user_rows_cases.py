"""Numpy inputs and restated rules for the user-row operations of the live user lists (qrlsh.UserLists.add_users /
remove_users / nearest, csrc/userrows.hip).  The lists themselves come from user_lists_cases (reference_lists,
restated_update); this module holds

  nearest_rule()     the most similar existing user of a new row: rint(1000 * dot / (sqrt(na) * sqrt(nb))) over the
                     truncated centred rows, 0 where a norm is 0; the largest value, ties to the lowest id; (-1, 0) where
                     nothing is positive
  assign_labels()    add_users(labels=None): the label of that user, or -- below 1 -- a cluster of its own, labelled one
                     more than the largest label in use, counting up in row order.  This rule is the project's own: the
                     reference never admits a user after clustering.
  restated_add()     the update rule with R = the new ids over lists grown by empty rows: nothing is picked
  restated_remove()  picked = surviving rows with exactly K entries, one of which names a removed user: scored again
                     against the surviving members of their cluster; every other surviving row keeps its entries that
                     name survivors, in order; then ids are renumbered by rank

and the named cases at nq = 37.  A case holds the matrix, the labels, K, the operation, the matrix afterwards by plain
numpy indexing and the labels of all users afterwards."""
import numpy as np

import user_lists_cases as UC


# ---------------------------------------------------------------------------------------------------------------- rules
def cross_milli(ratings, rows):
    """int32 [m][nu]: the lists' score of every (new row, existing user)"""
    ratings = np.asarray(ratings)
    a, b = UC.centred(np.asarray(rows).reshape(-1, ratings.shape[1])), UC.centred(ratings)
    dot = a @ b.T
    na, nb = (a * a).sum(axis=1), (b * b).sum(axis=1)
    den = np.sqrt(na.astype(np.float64))[:, None] * np.sqrt(nb.astype(np.float64))[None, :]
    ok = (na[:, None] != 0) & (nb[None, :] != 0)
    cs = np.zeros(dot.shape, dtype=np.float64)
    cs[ok] = dot[ok].astype(np.float64) / den[ok]
    return np.rint(cs * 1000.0).astype(np.int32)


def nearest_rule(ratings, rows):
    """-> (user int32 [m], milli int32 [m], every score int32 [m][nu])"""
    mm = cross_milli(ratings, rows)
    m = mm.shape[0]
    user, milli = np.full(m, -1, dtype=np.int32), np.zeros(m, dtype=np.int32)
    for k in range(m):
        if mm.shape[1] and mm[k].max() > 0:
            user[k] = int(np.argmax(mm[k]))          # the first of the largest: the lowest id
            milli[k] = mm[k, user[k]]
    return user, milli, mm


def assign_labels(labels, user, milli):
    """the labels add_users(labels=None) gives, from nearest_rule's answer over the matrix before the batch"""
    labels = np.asarray(labels, dtype=np.int64)
    top = int(labels.max())
    out = np.empty(len(user), dtype=np.int64)
    for k in range(len(user)):
        if milli[k] >= 1:
            out[k] = labels[user[k]]
        else:
            top += 1
            out[k] = top
    return out


def restated_add(lists, new_ratings, all_labels, K, nu):
    """lists: those of the first nu users before the batch -> (the lists of all users afterwards, picked)"""
    m = len(all_labels) - nu
    grown = tuple(np.concatenate((a, e)) for a, e in zip(lists, UC.empty_lists(m, K)))
    return UC.restated_update(grown, new_ratings, all_labels, K, np.arange(nu, nu + m))


def new_positions(nu, gone):
    keep = np.ones(nu, dtype=bool)
    keep[np.asarray(gone, dtype=np.int64)] = False
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64), keep


def restated_remove(lists, ratings, labels, K, gone):
    """lists: those of the matrix before the removal -> (the lists of the survivors under their new ids, the picked
    rows by their old ids, new_pos)"""
    labels = np.asarray(labels)
    idx, mil, ln = lists
    nu = len(labels)
    new_pos, keep = new_positions(nu, gone)
    G = set(np.flatnonzero(~keep).tolist())
    picked = [v for v in range(nu) if keep[v] and ln[v] == K and any(int(d) in G for d in idx[v, :K])]
    c = UC.centred(ratings)
    out = UC.empty_lists(int(keep.sum()), K)
    for v in np.flatnonzero(keep):
        v = int(v)
        if v in picked:
            mem = np.flatnonzero((labels == labels[v]) & keep)
            mm = UC.milli_matrix(c[mem])
            a = int(np.flatnonzero(mem == v)[0])
            cand = [(int(mm[a, b]), int(new_pos[w])) for b, w in enumerate(mem) if b != a]
        else:
            cand = [(int(mil[v, k]), int(new_pos[idx[v, k]])) for k in range(ln[v]) if int(idx[v, k]) not in G]
        UC._put(out, int(new_pos[v]), cand, K)
    return out, picked, new_pos


# ---------------------------------------------------------------------------------------------------------------- cases
def _add(ratings, labels, K, rows, given):
    r, rows = np.asarray(ratings, dtype=np.int64), np.asarray(rows, dtype=np.int64).reshape(-1, np.asarray(ratings).shape[1])
    labels = np.asarray(labels, dtype=np.int64)
    if given is None:
        user, milli, _ = nearest_rule(r, rows)
        returned = assign_labels(labels, user, milli)
    else:
        returned = np.asarray(given, dtype=np.int64)
    return {"op": "add", "ratings": r, "labels": labels, "K": K, "rows": rows,
            "given": None if given is None else np.asarray(given, dtype=np.int64), "new": np.vstack((r, rows)),
            "all_labels": np.concatenate((labels, returned)), "returned": returned}


def _remove(ratings, labels, K, users):
    r, labels = np.asarray(ratings, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    new_pos, keep = new_positions(r.shape[0], users)
    return {"op": "remove", "ratings": r, "labels": labels, "K": K, "users": np.asarray(users, dtype=np.int64),
            "new": np.ascontiguousarray(r[keep]), "all_labels": labels[keep], "new_pos": new_pos}


def run(ul, c):
    """the case's operation on a qrlsh.UserLists -> its return value"""
    if c["op"] == "add":
        return ul.add_users(c["rows"], labels=c["given"])
    return ul.remove_users(c["users"])


def restated(c):
    """-> (lists before, lists after by the restated rule, picked)"""
    before = UC.reference_lists(c["ratings"], c["labels"], c["K"])
    if c["op"] == "add":
        after, picked = restated_add(before, c["new"], c["all_labels"], c["K"], c["ratings"].shape[0])
    else:
        after, picked, _ = restated_remove(before, c["ratings"], c["labels"], c["K"], c["users"])
    return before, after, picked


def _search(rng, draw, wanted, tries=2000):
    """the first draw that shows the property a case is named for"""
    for _ in range(tries):
        x = draw(rng)
        if wanted(x):
            return x
    raise AssertionError("no input with the wanted property in %d draws" % tries)


def _effect(r, lab, K, row, label):
    """how one newcomer changes the old rows: (rows that took it in and lost their last entry, rows that took it in,
    its positive scores)"""
    c = _add(r, lab, K, row, [label])
    nu = r.shape[0]
    before = UC.reference_lists(c["ratings"], c["labels"], K)
    after = UC.reference_lists(c["new"], c["all_labels"], K)
    took = [v for v in range(nu) if nu in after[0][v, :after[2][v]]]
    pushed = [v for v in took if before[2][v] == K and before[0][v, K - 1] not in after[0][v]]
    return pushed, took, int((cross_milli(r, row)[0][lab == label] > 0).sum())


PICKS = ("named_by_full_rows", "ties_at_the_cut", "mixed_K1_remove", "mixed_K19_remove")
NO_PICKS = ("nobody_names_the_user", "named_by_short_rows_only", "whole_cluster_removed")
ADDS_NOTHING = ("ranks_below_full_rows", "ties_the_Kth_entry", "unrated_newcomer")


def mixed_matrix():
    c = UC.build_cases()["mixed_K19"]
    return c["ratings"], c["labels"]


def build_cases():
    """name -> case; test_user_rows_host pins the property each is named for"""
    rng = np.random.default_rng(20262)
    nq = 37
    cases = {}
    # ---- add, labels given
    r = UC._like_minded(rng, 5, nq)
    cases["into_short_rows"] = _add(np.vstack((r[:4], UC._random(rng, 3, nq))), [0] * 4 + [1] * 3, 8, r[4], [0])
    K = 4
    r = UC._like_minded(rng, K + 3, nq, noise=2)                 # K + 2 users: every row is full
    lab = np.zeros(K + 2, dtype=np.int64)
    prototype = np.rint(np.where(r[:K + 2] > 0, r[:K + 2], np.nan).mean(axis=0, where=r[:K + 2] > 0)).astype(np.int64)
    prototype[~(r[:K + 2] > 0).any(axis=0)] = 0
    assert _effect(r[:K + 2], lab, K, prototype, 0)[0], "the cluster's own mean outranks nobody's last entry"
    cases["outranks_full_rows"] = _add(r[:K + 2], lab, K, prototype, [0])
    faint = _search(rng, lambda g: np.where(g.random(nq) < 0.2, r[0], UC._random(g, 1, nq)[0]),
                    lambda x: not _effect(r[:K + 2], lab, K, x, 0)[1] and _effect(r[:K + 2], lab, K, x, 0)[2] > 0)
    cases["ranks_below_full_rows"] = _add(r[:K + 2], lab, K, faint, [0])
    t = UC.build_cases()["ties_at_the_cut"]["ratings"]           # users 1 .. 6 hold the same row; K = 3
    cases["ties_the_Kth_entry"] = _add(t, [0] * 9, 3, t[1], [0])
    r = UC._like_minded(rng, 8, nq)
    cases["two_newcomers_one_cluster"] = _add(r[:6], [5] * 6, 8, r[6:], [5, 5])
    a, b, n = UC._like_minded(rng, 6, nq), UC._like_minded(rng, 5, nq), UC._like_minded(rng, 2, nq)
    cases["two_clusters_and_a_new_label"] = _add(np.vstack((a[:5], b[:4])), [0] * 5 + [1] * 4, 4,
                                                 np.vstack((a[5], n[0], b[4], n[1])), [0, 77, 1, 77])
    cases["unrated_newcomer"] = _add(a, [0] * 6, 3, np.zeros(nq, dtype=np.int64), [0])
    r = np.vstack((UC._like_minded(rng, 20, nq, noise=2), UC._like_minded(rng, 13, nq, noise=2)))
    who = np.r_[0:19, 20:32]                                     # 31 users; the newcomers are 31 and 32
    cases["nu_crosses_an_id_map_word"] = _add(r[who], [0] * 19 + [1] * 12, 5, r[[19, 32]], [0, 1])
    # ---- add, labels=None
    a, b = UC._like_minded(rng, 5, nq), UC._like_minded(rng, 4, nq)
    two = np.vstack((a, b))
    cases["copy_of_an_existing_user"] = _add(two, [3] * 5 + [8] * 4, 4, b[2], None)
    same = two.copy()
    same[7] = same[2]                                            # users 2 and 7 hold one row, in different clusters
    cases["identical_users_lowest_id_wins"] = _add(same, [3] * 5 + [8] * 4, 4, same[7], None)
    flipped = np.where(a[0] > 0, 101 - a[0], 0)                  # against one like-minded cluster: nothing positive
    cases["nothing_positive_own_cluster"] = _add(a, [3] * 5, 4, flipped, None)
    lone = np.zeros(nq, dtype=np.int64)
    lone[4] = 60                                                 # one rating: the centred row is zero
    cases["two_own_clusters_in_one_batch"] = _add(a, [3] * 5, 4, np.vstack((lone, a[1], np.zeros(nq, dtype=np.int64))), None)
    # ---- remove
    r = np.vstack((UC._like_minded(rng, 5, nq), UC._like_minded(rng, 4, nq), UC._random(rng, 1, nq)))
    lab = [0] * 5 + [1] * 4 + [2]
    cases["nobody_names_the_user"] = _remove(r, lab, 3, [9])
    cases["named_by_short_rows_only"] = _remove(r, lab, 6, [1])
    r7 = UC._like_minded(rng, 7, nq)
    cases["named_by_full_rows"] = _remove(r7, [0] * 7, 4, [2])
    cases["whole_cluster_removed"] = _remove(r, lab, 3, [5, 6, 7, 8])
    cases["first_and_last_user"] = _remove(r, lab, 3, [9, 0])
    cases["duplicates_in_the_ids"] = _remove(r, lab, 3, [6, 2, 6, 6, 2])
    cases["all_users_but_one"] = _remove(r, lab, 3, [u for u in range(10) if u != 6])
    cases["cluster_left_with_one_member"] = _remove(r, lab, 3, [5, 7, 8])
    cases["ties_at_the_cut"] = _remove(t, [0] * 9, 3, [2])
    # ---- the nu = 150 matrix (its id map spans five words), both operations at every K
    r, lab = mixed_matrix()
    nu = r.shape[0]
    taste = r[np.flatnonzero(lab == 0)[:3]]
    rows = np.vstack((np.where(rng.random((3, nq)) < 0.8, taste, 0), UC._random(rng, 3, nq)))
    gone = rng.choice(nu, size=14, replace=False)
    for K in (1, 19, 64):
        cases["mixed_K%d_add" % K] = _add(r, lab, K, rows, [0, 0, 4, 4, 1000, 1000])
        cases["mixed_K%d_add_nearest" % K] = _add(r, lab, K, rows, None)
        cases["mixed_K%d_remove" % K] = _remove(r, lab, K, gone)
    return cases
