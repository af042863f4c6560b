"""Numpy inputs for the column operations of the live user lists (qrlsh.UserLists.add_columns / remove_columns /
set_columns, csrc/usercolumns.hip).  A case holds the matrix, the labels, K, the operation, the matrix afterwards by
plain numpy indexing, and R by the rule: a row is changed exactly when, in some affected column, its old value (0 for
an appended column) differs from its new one (0 for a removed column).  The lists themselves come from
user_lists_cases (reference_lists, restated_update)."""
import numpy as np

import user_lists_cases as UC


def apply_op(ratings, op, cols=None, block=None):
    """-> (new matrix, R).  op "add": block = int m (unrated columns) or [nu][m]; "remove": cols, any order, repeats
    allowed; "set": cols distinct, block [nu][len(cols)]"""
    r = np.asarray(ratings, dtype=np.int64)
    nu, nq = r.shape
    if op == "add":
        now = np.zeros((nu, block), dtype=np.int64) if isinstance(block, int) else np.asarray(block, dtype=np.int64)
        old = np.zeros_like(now)
        new = np.hstack((r, now))
    elif op == "remove":
        c = np.asarray(cols, dtype=np.int64).reshape(-1)
        keep = np.ones(nq, dtype=bool)
        keep[c] = False
        old = r[:, c]
        now = np.zeros_like(old)
        new = np.ascontiguousarray(r[:, keep])
    elif op == "set":
        c = np.asarray(cols, dtype=np.int64).reshape(-1)
        assert len(set(c.tolist())) == c.size
        now = np.asarray(block, dtype=np.int64)
        old = r[:, c]
        new = r.copy()
        new[:, c] = now
    else:
        raise ValueError(op)
    return new, np.flatnonzero((old != now).any(axis=1).reshape(nu))


def _case(ratings, labels, K, op, cols=None, block=None):
    r = np.asarray(ratings, dtype=np.int64)
    new, R = apply_op(r, op, cols, block)
    return {"ratings": r, "labels": np.asarray(labels, dtype=np.int64), "K": K, "op": op,
            "cols": None if cols is None else np.asarray(cols, dtype=np.int64),
            "block": block if block is None or isinstance(block, int) else np.asarray(block, dtype=np.int64),
            "new": new, "R": R}


def run(ul, c):
    """the case's operation on a qrlsh.UserLists (or anything with the three methods) -> its return value"""
    if c["op"] == "add":
        return ul.add_columns(c["block"])
    if c["op"] == "remove":
        return ul.remove_columns(c["cols"])
    return ul.set_columns(c["cols"], c["block"])


R_EMPTY = ("unrated_columns_appended", "never_rated_column_removed", "equal_values_overwritten")
PICKS = ("agreed_columns_removed", "ties_at_the_cut", "mixed_K19_remove")


def mixed_matrix():
    """user_lists_cases' nu = 150 matrix: a cluster of 80 like-minded users and 9 random ones, interleaved in id order"""
    c = UC.build_cases()["mixed_K19"]
    return c["ratings"], c["labels"]


def build_cases():
    """name -> {ratings, labels, K, op, cols, block, new, R}; test_user_columns_host pins the property each is named for"""
    rng = np.random.default_rng(20251)
    nq = 37
    cases = {}
    two = [0] * 6 + [1] * 5
    r = np.vstack((UC._like_minded(rng, 6, nq), UC._like_minded(rng, 5, nq)))
    cases["unrated_columns_appended"] = _case(r, two, 4, "add", block=3)
    b = np.zeros((11, 2), dtype=np.int64)
    b[1] = (80, 0)
    b[7] = (15, 95)
    cases["block_appended_two_users_rated"] = _case(r, two, 4, "add", block=b)
    r0 = r.copy()
    r0[:, 5] = 0
    cases["never_rated_column_removed"] = _case(r0, two, 4, "remove", cols=[5])
    cases["rated_column_removed"] = _case(r, two, 4, "remove", cols=[7])
    cases["first_and_last_column_removed"] = _case(r, two, 4, "remove", cols=[nq - 1, 0])
    cases["duplicates_in_cols"] = _case(r, two, 4, "remove", cols=[3, 9, 3, 20, 9, 3])
    cases["every_column_but_one_removed"] = _case(r, two, 4, "remove", cols=[q for q in range(nq) if q != 11])
    cases["every_column_removed"] = _case(r, two, 4, "remove", cols=list(range(nq))[::-1])
    cases["equal_values_overwritten"] = _case(r, two, 4, "set", cols=[8, 2], block=r[:, [8, 2]])
    r1 = r.copy()
    r1[1, 4], r1[2, 30], r1[3, 17], r1[9, 17] = 40, 0, 60, 0
    b = r1[:, [30, 4, 17]].copy()
    b[1, 1] = 0        # x -> 0
    b[2, 0] = 55       # 0 -> x
    b[3, 2] = 61       # x -> y
    cases["overwrites_to_zero_from_zero_and_between"] = _case(r1, two, 4, "set", cols=[30, 4, 17], block=b)
    # users 0 and 1 alone rated five columns, and agree there: without them the two drift apart from each other, and
    # the full rows of the others that name one of them are picked
    r = UC._like_minded(rng, 8, nq)
    agreed = [2, 11, 12, 25, 33]
    r[:, agreed] = 0
    r[0, agreed] = r[1, agreed] = (100, 1, 100, 1, 100)
    cases["agreed_columns_removed"] = _case(r, [0] * 8, 4, "remove", cols=agreed)
    r = np.vstack((UC._like_minded(rng, 4, nq), UC._like_minded(rng, 7, nq)))
    r[:4, 19], r[4:, 19] = (10, 35, 60, 85), 0
    cases["R_is_a_whole_cluster"] = _case(r, [0] * 4 + [1] * 7, 3, "remove", cols=[19])
    r = np.vstack((UC._like_minded(rng, 6, nq), UC._like_minded(rng, 5, nq), UC._random(rng, 2, nq)))
    lab = [0] * 6 + [1] * 5 + [2, 3]
    b = r[:, [6, 21]].copy()
    b[1], b[8], b[12] = (100 - b[1, 0], 3), (0, 99), (7, 7)
    cases["two_clusters_at_once"] = _case(r, lab, 4, "set", cols=[6, 21], block=b)
    r = UC.build_cases()["ties_at_the_cut"]["ratings"]          # users 1 .. 6 hold the same row
    b = np.zeros((9, 2), dtype=np.int64)
    b[0], b[4], b[8] = (77, 0), (11, 30), (0, 50)
    cases["ties_at_the_cut"] = _case(r, [0] * 9, 3, "add", block=b)
    # the nu = 150 matrix (its id map spans five words), every operation at every K
    r, lab = mixed_matrix()
    nu = r.shape[0]
    who = rng.choice(nu, size=12, replace=False)
    add = np.zeros((nu, 3), dtype=np.int64)
    add[who, rng.integers(0, 3, size=12)] = rng.integers(1, 101, size=12)
    st = r[:, [35, 0, 18]].copy()
    st[who[:4], 0], st[who[4:8], 1], st[who[8:], 2] = 0, rng.integers(1, 101, size=4), 101 - st[who[8:], 2]
    for K in (1, 19, 64):
        cases["mixed_K%d_add" % K] = _case(r, lab, K, "add", block=add)
        cases["mixed_K%d_remove" % K] = _case(r, lab, K, "remove", cols=[29, 4])
        cases["mixed_K%d_set" % K] = _case(r, lab, K, "set", cols=[35, 0, 18], block=st)
    return cases
