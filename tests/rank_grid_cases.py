"""The numpy restatement of the ranking grid (qrlsh_evaluate_ranking_grid) and seeded cases for it (test infrastructure
only).  Per setting the predictions at the test cells come from tune_cases.sides + tune_cases.blend (the oracle's
weighted_average and sum orders) and are handed to rank_eval_cases.rank_eval_ref(candidates="heldout", pred=...): never
the code under test.  test_rank_grid_host pins this restatement against rank_eval_ref over host-cut lists."""
import numpy as np

from oracle import oracle as O
import rank_eval_cases as REC
import tune_cases as TC


def sides_of_test_cells(train, truth, qs, us, rows, q_cuts, u_cuts, summation=O.np_sum_order):
    """{user: (columns, [qp per query cut][cell], [up per user cut][cell])} for the rows named: the two sides of every
    test cell (train == 0 and truth != 0), once per cut -- the expensive part, shared by every setting"""
    train, truth = np.asarray(train), np.asarray(truth)
    out = {}
    for u in sorted(set(int(r) for r in rows)):
        cols = np.flatnonzero((train[u] == 0) & (truth[u] != 0))
        qp = np.zeros((len(q_cuts), len(cols)))
        up = np.zeros((len(u_cuts), len(cols)))
        for c, j in enumerate(cols.tolist()):
            a, b = TC.sides(train, qs, us, u, j, q_cuts, u_cuts, summation)
            qp[:, c], up[:, c] = a, b
        out[u] = (cols, qp, up)
    return out


def setting_predictions(sides, rows, nq, cq, cu, triple):
    """int64 [m][nq]: the prediction of every test cell of each request's row under one setting, 0 elsewhere"""
    pred = np.zeros((len(rows), nq), dtype=np.int64)
    done = {}
    for x, u in enumerate(rows):
        if u not in done:
            cols, qp, up = sides[u]
            line = np.zeros(nq, dtype=np.int64)
            for c, j in enumerate(cols.tolist()):
                line[j] = TC.blend(qp[cq, c], up[cu, c], *triple)[0]
            done[u] = line
        pred[x] = done[u]
    return pred


def rank_grid_ref(train, truth, qs, us, users, k, relevant, gains, q_cuts, u_cuts, weights, summation=O.np_sum_order,
                  sides=None):
    """-> (per int64 [m][CQ][CU][W][8], totals int64 [CQ][CU][W][16], idx int64 [m][CQ][CU][W][k]).
    sides: sides_of_test_cells(...) of the same matrices, lists, cuts and summation, when several k share them"""
    train = np.asarray(train)
    nu, nq = train.shape
    rows = list(range(nu)) if users is None else [int(u) for u in users]
    weights = [tuple(float(x) for x in w) for w in np.asarray(weights, dtype=np.float64).reshape(-1, 3)]
    shape = (len(q_cuts), len(u_cuts), len(weights))
    if sides is None:
        sides = sides_of_test_cells(train, truth, qs, us, rows, q_cuts, u_cuts, summation)
    per = np.zeros((len(rows),) + shape + (8,), dtype=np.int64)
    totals = np.zeros(shape + (16,), dtype=np.int64)
    idx = np.zeros((len(rows),) + shape + (k,), dtype=np.int64)
    for a in range(shape[0]):
        for b in range(shape[1]):
            for w, triple in enumerate(weights):
                pred = setting_predictions(sides, rows, nq, a, b, triple)
                i, _, _, p, t = REC.rank_eval_ref(train, truth, None, None, rows, k, relevant, "heldout", gains, pred=pred)
                per[:, a, b, w], totals[a, b, w], idx[:, a, b, w] = p, t, i
    return per, totals, idx


def host_cut_lists(qs, us, q_cut, u_cut):
    """the lists a caller cuts on the host for one setting"""
    return TC.cut_lists(qs, q_cut), TC.cut_lists(us, u_cut)


# ------------------------------------------------------------------------------------------------------------ cases
MAIN_Q_CUTS, MAIN_U_CUTS = [0, 7, 8, 64], [0, 1, 8, 9]
MAIN_K, MAIN_RELEVANT = 10, 60
QUERY_ONLY, USER_ONLY = (1.0, 0.0, 50.0), (0.0, 1.0, 50.0)


def main_weights():
    """8 triples: the default, the two one-sided ones (they order the same cells differently), seeded ones"""
    w = [TC.DEFAULT, QUERY_ONLY, USER_ONLY] + [tuple(x) for x in TC.weight_grid(8, seed=3)[3:].tolist()]
    return np.array(w[:8], dtype=np.float64)


def main_case(seed=33, nu=24, nq=700, held=0.3):
    """tune_cases.planted_case (query lists of 0, 1, 7, 8, 9, 15, 16, 17 and 64 entries at both ends, user lists of 9)
    with about `held` of the rated cells held out; the requests name every user, three of them twice.
    -> (train, truth, coo, qs, us, users)"""
    truth, coo, qs, us = TC.planted_case(seed, nu, nq, 9)
    rng = np.random.default_rng(seed + 1000003)
    gone = (truth != 0) & (rng.random(truth.shape) < held)
    train = np.where(gone, 0, truth).astype(np.int32)
    users = list(range(nu)) + [3, 3, nu - 1]
    return train, truth, coo, qs, us, users


def main_expected(case, summation=O.np_sum_order):
    """rank_grid_ref of the main case's 128 settings.  Asserted here: under the whole lists the query-only and the
    user-only triple list different cells in a different order for some request, so a kernel that ranks once and
    reuses the order for every setting cannot pass."""
    train, truth, _, qs, us, users = case
    per, totals, idx = rank_grid_ref(train, truth, qs, us, users, MAIN_K, MAIN_RELEVANT, REC.dcg_gains_ref(MAIN_K),
                                     MAIN_Q_CUTS, MAIN_U_CUTS, main_weights(), summation)
    q_only, u_only = idx[:, 3, 3, 1], idx[:, 3, 3, 2]
    differ = sum(a.tolist() != b.tolist() for a, b in zip(q_only, u_only))
    assert differ > len(users) // 2, differ
    return per, totals, idx


def avail_case(k, seed=0):
    """Three users with exactly k - 1, k and k + 1 candidates (test cells with a non-zero prediction) and nothing else,
    in rank_eval_cases.cut_case's construction: user lists are empty and target query j has one neighbour, source C + j,
    at similarity 1.0, so under the default blend cell (u, j) predicts round(0.8 train[u][C + j] + 12) != 0.
    -> (train, truth, coo, qs, us)"""
    import evaluate_cases as EC
    C = k + 8
    rng = np.random.default_rng(seed + k)
    train = np.zeros((3, 2 * C), dtype=np.int32)
    truth = np.zeros((3, 2 * C), dtype=np.int32)
    for u, n in enumerate((k - 1, k, k + 1)):
        cols = rng.choice(C, size=n, replace=False)
        train[u, C + cols] = rng.integers(1, 101, size=n)
        truth[u, cols] = rng.integers(1, 101, size=n)
    truth[:, C:] = train[:, C:]
    qs = {j: {"indexes": np.array([C + j], dtype=np.int64), "values": np.array([1.0])} for j in range(C)}
    return train, truth, EC.coo_of(qs), qs, {}
