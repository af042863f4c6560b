"""Serving chosen queries (qrlsh.predict_queries / for_queries / query_utility): numpy restatements and seeded cases
(test infrastructure only).

The restatements are defined from the oracle's FULL prediction matrix (oracle.predict_scores, or a golden `final`), never
from the code under test:
  * the completed column of query j = column j of the matrix, transposed (request-major);
  * the top-k users = test_recommend_host.restate over the transposed columns: eligible = unrated and prediction != 0,
    value descending, then user ascending;
  * the 8 utility words from ratings[:, j], the matrix column and the zero / non-zero pattern of the two sides
    (oracle.weighted_average of the row over j's list and of the column over the user's list).
The case builders sit on predict_cases.build_case (knife cells on a rounding half, which tell the sum orders apart) and on
plain random data; each asserts what makes its case worth running."""
import numpy as np

from oracle import oracle as O
import predict_cases as PC
from test_recommend_host import restate

ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}


# ------------------------------------------------------------------------------------------------- the restatements
def restate_columns(final, queries):
    """(m, nu): row x = column queries[x] of the full matrix"""
    return np.asarray(final)[:, np.asarray(queries, dtype=np.int64)].T.astype(np.int64)


def restate_top_users(ratings, final, queries, k):
    """(users, val, avail) int64: restate() with the roles swapped, one row per request"""
    q = np.asarray(queries, dtype=np.int64)
    return restate(np.asarray(ratings)[:, q].T, np.asarray(final)[:, q].T, k)


def sides_nonzero(ratings, qs, us, j, summation=O.np_sum_order):
    """(query side != 0, user side != 0) bool [nu] for column j (meaningful at the unrated cells)"""
    ratings = np.asarray(ratings)
    nu = ratings.shape[0]
    qnz, unz = np.zeros(nu, dtype=bool), np.zeros(nu, dtype=bool)
    for u in range(nu):
        if j in qs:
            qnz[u] = O.weighted_average(ratings[u], qs[j]["indexes"], qs[j]["values"], summation) != 0
        if u in us:
            unz[u] = O.weighted_average(ratings[:, j], us[u]["indexes"], us[u]["values"], summation) != 0
    return qnz, unz


def restate_words(ratings, final, qs, us, queries, summation=O.np_sum_order):
    """int64 (m, 8): rated users, the sum of their ratings, unrated users with a non-zero prediction, the sum of those
    predictions, unrated users with prediction 0, unrated users with only the query side / only the user side / both
    sides non-zero"""
    ratings, final = np.asarray(ratings), np.asarray(final)
    words = np.zeros((len(queries), 8), dtype=np.int64)
    memo = {}
    for x, j in enumerate(int(q) for q in queries):
        if j not in memo:
            col, pred = ratings[:, j].astype(np.int64), final[:, j].astype(np.int64)
            rated, unrated = col != 0, col == 0
            qnz, unz = sides_nonzero(ratings, qs, us, j, summation)
            hit = unrated & (pred != 0)
            memo[j] = [rated.sum(), col[rated].sum(), hit.sum(), pred[hit].sum(), (unrated & (pred == 0)).sum(),
                       (unrated & qnz & ~unz).sum(), (unrated & ~qnz & unz).sum(), (unrated & qnz & unz).sum()]
        words[x] = memo[j]
    return words


def golden_case(name):
    """(ratings, final, qs, us) of a golden score set, lists in the oracle's dict form"""
    from test_recommend_users_host import golden_lists
    g, qs, us = golden_lists(name)
    return g["ratings"], g["final"], qs, us


# ------------------------------------------------------------------------------------------------------- the cases
class Case:
    """ratings int32 [nu][nq]; coo = (src, dst, milli) int64 numpy arrays sorted by source; qs / us the oracle's dicts"""

    def __init__(self, ratings, coo, qs, us):
        self.ratings, self.coo, self.qs, self.us = ratings, coo, qs, us
        self.nu, self.nq = ratings.shape

    def torch_coo(self):
        import torch
        return tuple(torch.tensor(x, dtype=torch.int32) for x in self.coo)


def coo_to_dict(src, dst, mil):
    qs = {}
    for j in np.unique(src):
        sel = src == j
        qs[int(j)] = {"indexes": dst[sel].astype(np.int64), "values": mil[sel] / 1000.0}
    return qs


def random_case(seed, nu, nq, longest_q, ku, fill=0.5):
    """random ratings 1..100, query lists of 0..longest_q distinct neighbours (never the query itself), user lists of
    exactly min(ku, nu - 1) other users"""
    rng = np.random.default_rng(seed)
    ratings = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < fill)).astype(np.int32)
    src, dst, mil = [], [], []
    for j in range(nq):
        n = int(rng.integers(0, min(longest_q, nq - 1) + 1))
        ix = rng.choice(nq - 1, size=n, replace=False)
        src += [j] * n
        dst += (ix + (ix >= j)).tolist()   # the ids from j on shifted past j
        mil += np.sort(rng.integers(0, 1001, size=n))[::-1].tolist()
    coo = tuple(np.asarray(x, dtype=np.int64) for x in (src, dst, mil))
    us = {}
    n = min(ku, nu - 1)
    for u in range(nu):
        if n > 0:
            ix = rng.choice(nu - 1, size=n, replace=False).astype(np.int64)
            us[u] = {"indexes": ix + (ix >= u), "values": np.round(rng.random(n), 3)}
    return Case(ratings, coo, coo_to_dict(*coo), us)


def knife_case():
    """A predict_cases knife matrix, 48 users x 300 queries, with the chosen columns: every target query (knife cells),
    some ordinary ones (one twice, out of order) and the spare one no list names.  -> (case c, queries, finals per sum
    order).  Asserts that the sum orders part inside the chosen columns, and that some unrated user has an unrated
    neighbour user with a non-zero prediction in the same column whose value would CHANGE the user side: a sweep whose
    user side read cells it had already written would show."""
    c = PC.build_case(21, nu=48, nq=300, tu=6, tq=12, user_longest=32)
    queries = [7, 0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 200, 57, c.spare, 200, 13]
    finals = {o: O.predict_scores(c.ratings, c.qs, c.us, summation=s) for o, s in ORDERS.items()}
    cols = {o: restate_columns(finals[o], queries) for o in ORDERS}
    assert (cols["pairwise"] != cols["sequential"]).any(), "the sum orders agree on every chosen cell"
    final = finals["pairwise"]
    written = 0
    for j in set(queries):
        for u in range(c.nu):
            if c.ratings[u, j] == 0:
                ix, v = c.us[u]["indexes"], c.us[u]["values"]
                if O.weighted_average(final[:, j], ix, v) != O.weighted_average(c.ratings[:, j], ix, v):
                    written += 1
    assert written > 0, "no user side would change by reading predicted cells"
    return c, queries, finals


def mixed_forms_case():
    """2000 users x 40 queries.  Column 3 holds a 256, column 5 a negative rating (both: the memory form inside their
    workgroups), column 7 is all zero, column 9 fully rated; the others are narrow (LDS form) -- both forms in one launch.
    -> (case, queries)."""
    c = random_case(77, 2000, 40, 12, 6)
    r = c.ratings
    r[1234, 3] = 256
    r[17, 5] = -3
    r[:, 7] = 0
    r[:, 9] = np.where(r[:, 9] == 0, 41, r[:, 9])
    queries = [0, 3, 5, 7, 9, 12, 39, 3]
    assert r[:, 3].max() > 255 and r[:, 5].min() < 0 and not r[:, 7].any() and r[:, 9].all()
    narrow = [j for j in queries if j not in (3, 5)]
    assert all(0 <= r[:, j].min() and r[:, j].max() <= 255 for j in narrow)
    # the wide value is read by some user side: user 1234 is some unrated user's neighbour
    assert any(1234 in c.us[u]["indexes"] for u in range(c.nu) if r[u, 3] == 0)
    assert any(17 in c.us[u]["indexes"] for u in range(c.nu) if r[u, 5] == 0)
    return c, queries
