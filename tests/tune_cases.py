"""The numpy restatement of the grid evaluation (qrlsh_evaluate_grid) and seeded cases for it (test infrastructure only).
Built on evaluate_cases (the oracle's weighted_average and sum orders, the sample rule), never on the code under test.

A setting is (query-list cut, user-list cut, (query_weight, user_weight, default_mean)).  The restatement cuts the lists
on the host -- the first min(len, cut) entries as stored -- and then does evaluate_cases.evaluate_ref's arithmetic with
the weights as parameters.  Per setting 8 int64 words: n, sum err, sum |err|, sum err^2 over the non-zero predictions,
missed, cells evaluated, n from the query side only, n from the user side only."""
import numpy as np

from oracle import oracle as O
import evaluate_cases as EC

DEFAULT = (EC.QW, EC.UW, float(EC.DM))
WHOLE = 64


def words8(e16):
    """evaluate's 16 words (last axis) -> the grid's 8"""
    e = np.asarray(e16, dtype=np.int64)
    out = np.zeros(e.shape[:-1] + (8,), dtype=np.int64)
    for k in range(4):
        out[..., k] = e[..., k] + e[..., 4 + k] + e[..., 8 + k]
    out[..., 4], out[..., 5], out[..., 6], out[..., 7] = e[..., 12], e[..., 13], e[..., 0], e[..., 4]
    return out


def cut_lists(lists, cut):
    """every list's first min(len, cut) entries; a list cut to nothing is left out"""
    out = {}
    for k, v in lists.items():
        if cut > 0 and len(v["indexes"]):
            out[k] = {"indexes": np.asarray(v["indexes"])[:cut], "values": np.asarray(v["values"])[:cut]}
    return out


def blend(qp, up, qw, uw, dm):
    """recommender.py:324-331 with the weights as parameters -> (prediction, branch 0 / 1 / 2)"""
    if up == 0 and qp == 0:
        return 0, 0
    if up == 0:
        return int(round(qp * (qw + (uw * 0.5)) + dm * (uw * 0.5))), 0
    if qp == 0:
        return int(round(up * (uw + (qw * 0.5)) + dm * (qw * 0.5))), 1
    return int(round(qp * qw + up * uw)), 2


def sides(ratings, qs, us, i, j, q_cuts, u_cuts, summation):
    """([qp per query cut], [up per user cut]) of cell (i, j) as if ratings[i][j] were 0"""
    def per_cut(values_at, own, lists, key, cuts):
        done = {}   # by the length left: two cuts that leave the same prefix are one list
        for c in cuts:
            n = min(c, len(lists[key]["indexes"])) if key in lists else 0
            if n not in done:
                done[n] = EC._side(values_at, own, cut_lists({key: lists[key]}, c).get(key) if n else None, summation)
        return [done[min(c, len(lists[key]["indexes"])) if key in lists else 0] for c in cuts]
    return per_cut(ratings[i], j, qs, j, q_cuts), per_cut(ratings[:, j], i, us, i, u_cuts)


def grid_ref(ratings, qs, us, cells, values, q_cuts, u_cuts, weights, nu=None, summation=O.np_sum_order):
    """cells int [n][2], values [n] (their truth) -> (pred int64 [n][CQ][CU][W], per_user int64 [nu][CQ][CU][W][8],
    totals int64 [CQ][CU][W][8])"""
    ratings = np.asarray(ratings)
    nu = ratings.shape[0] if nu is None else nu
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    weights = [tuple(float(x) for x in w) for w in np.asarray(weights, dtype=np.float64).reshape(-1, 3)]
    shape = (len(q_cuts), len(u_cuts), len(weights))
    pred = np.zeros((len(cells),) + shape, dtype=np.int64)
    per = np.zeros((nu,) + shape + (8,), dtype=np.int64)
    for c, ((i, j), tv) in enumerate(zip(cells.tolist(), np.asarray(values).tolist())):
        qp, up = sides(ratings, qs, us, i, j, q_cuts, u_cuts, summation)
        for a in range(shape[0]):
            for b in range(shape[1]):
                for w, (qw, uw, dm) in enumerate(weights):
                    p, branch = blend(qp[a], up[b], qw, uw, dm)
                    pred[c, a, b, w] = p
                    line = per[i, a, b, w]
                    line[5] += 1
                    if p == 0:
                        line[4] += 1
                        continue
                    e = p - int(tv)
                    line[0] += 1
                    line[1] += e
                    line[2] += abs(e)
                    line[3] += e * e
                    if branch == 0:
                        line[6] += 1
                    elif branch == 1:
                        line[7] += 1
    return pred, per, per.sum(axis=0)


def weight_grid(n, seed=0):
    """n weight triples: the default first, then seeded ones (weights in 0 .. 1.2, means in 0 .. 100), among them a
    zero query weight and a zero user weight"""
    rng = np.random.default_rng(seed)
    w = [DEFAULT, (0.0, 1.0, 50.0), (1.0, 0.0, 50.0)]
    while len(w) < n:
        w.append((float(rng.integers(0, 13)) / 10.0, float(rng.integers(0, 13)) / 10.0, float(rng.integers(0, 101))))
    return np.array(w[:n], dtype=np.float64)


def planted_case(seed, nu, nq, ku, lengths=(0, 1, 7, 8, 9, 15, 16, 17, 64), fill=0.5):
    """evaluate_cases.random_case with query lists of exactly `lengths` entries planted on the first queries and on the
    last ones (both ends of the matrix), values descending as stored lists have them.  Where ku > nu the user lists are
    drawn with repeats (random_case wants ku distinct users): ku entries each, naming their own user among others.
    -> (ratings, coo, qs, us)"""
    ratings, _, qs, us = EC.random_case(seed, nu, nq, 12, min(ku, nu), fill=fill)
    rng = np.random.default_rng(seed + 1)
    if ku > nu:
        us = {u: {"indexes": rng.integers(0, nu, size=ku).astype(np.int64),
                  "values": np.sort(rng.integers(0, 1001, size=ku))[::-1] / 1000.0} for u in range(nu)}
    for base in (0, nq - len(lengths)):
        for k, n in enumerate(lengths):
            j = base + k
            qs.pop(j, None)
            if n:
                qs[j] = {"indexes": rng.integers(0, nq, size=n).astype(np.int64),
                         "values": np.sort(rng.integers(0, 1001, size=n))[::-1] / 1000.0}
    return ratings, EC.coo_of(qs), qs, us
