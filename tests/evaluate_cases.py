"""The numpy restatement of the evaluation (qrlsh_ratings_holdout / qrlsh_evaluate / qrlsh_evaluate_cells) and seeded
cases for it (test infrastructure only).  Built on the oracle's weighted_average and sum orders and on the library's
host mixer qrlsh_mix64_host, never on the code under test.

A cell (i, j) is EVALUATED iff truth[i][j] != 0 and the sample rule keeps it; its prediction is the blend of
recommender.py:313-331 computed from `ratings` as if ratings[i][j] were 0; err = prediction - truth.  Per user, 16
int64 words: 0-3, 4-7, 8-11 = n, sum err, sum |err|, sum err^2 of the cells predicted from the query side only, the user
side only and both; 12 = evaluated cells whose prediction is 0; 13 = evaluated cells; 14-15 = 0."""
import numpy as np

from oracle import oracle as O

QW, UW, DM = 0.6, 0.4, 60     # recommender.py:32-34
ALL = 1 << 32                 # keep: every cell


def np_mix64(z):
    """qr_mix64 (csrc/common.h) on a uint64 array; test_evaluate_host pins it to qrlsh_mix64_host"""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keep_of(fraction):
    return int(round(fraction * 2.0**32))


def kept_mask(nu, nq, seed, keep):
    """bool [nu][nq]: the sample rule mix64(seed ^ (i << 32 | j)) >> 32 < keep"""
    i = np.arange(nu, dtype=np.uint64).reshape(-1, 1) << np.uint64(32)
    j = np.arange(nq, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        top = np_mix64(np.uint64(seed) ^ (i | j)) >> np.uint64(32)
    return top < np.uint64(keep) if keep < ALL else np.ones((nu, nq), dtype=bool)


def kept_cells(cells, seed, keep):
    """the same rule for listed cells [n][2]"""
    c = np.asarray(cells, dtype=np.uint64).reshape(-1, 2)
    with np.errstate(over="ignore"):
        top = np_mix64(np.uint64(seed) ^ ((c[:, 0] << np.uint64(32)) | c[:, 1])) >> np.uint64(32)
    return top < np.uint64(keep) if keep < ALL else np.ones(len(c), dtype=bool)


def holdout_ref(ratings, seed, keep):
    """(train matrix, cells zeroed)"""
    ratings = np.asarray(ratings)
    gone = (ratings != 0) & kept_mask(*ratings.shape, seed, keep)
    return np.where(gone, 0, ratings).astype(ratings.dtype), int(gone.sum())


def _side(values_at, own, lst, summation):
    """weighted_average over a list with the entries that name the cell's own row / column reading 0"""
    if lst is None or len(lst["indexes"]) == 0:
        return 0.0
    idx = np.asarray(lst["indexes"], dtype=np.int64)
    ur = np.where(idx == own, 0, values_at[idx])
    # oracle.weighted_average gathers ratings_row[indexes]: hand it the gathered values under the identity index
    return O.weighted_average(ur, np.arange(len(idx)), lst["values"], summation)


def predict_unrated(ratings, qs, us, i, j, summation=O.np_sum_order):
    """(prediction, branch) of cell (i, j) as if ratings[i][j] were 0; branch 0 / 1 / 2 = query side only / user side
    only / both, -1 = no prediction (0)"""
    qp = _side(ratings[i], j, qs.get(j), summation)
    up = _side(ratings[:, j], i, us.get(i), summation)
    if up == 0 and qp == 0:
        return 0, -1
    if up == 0:
        p, b = round(qp * (QW + (UW * 0.5)) + DM * (UW * 0.5)), 0
    elif qp == 0:
        p, b = round(up * (UW + (QW * 0.5)) + DM * (QW * 0.5)), 1
    else:
        p, b = round(qp * QW + up * UW), 2
    return int(p), (b if p != 0 else -1)


def evaluate_ref(ratings, qs, us, cells, values, nu=None, summation=O.np_sum_order):
    """cells int [n][2], values [n] (their truth) -> (pred int64 [n], per_user int64 [nu][16], totals int64 [16]);
    repeated cells count once each"""
    ratings = np.asarray(ratings)
    nu = ratings.shape[0] if nu is None else nu
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    pred = np.zeros(len(cells), dtype=np.int64)
    per = [[0] * 16 for _ in range(nu)]
    for c, ((i, j), tv) in enumerate(zip(cells.tolist(), np.asarray(values).tolist())):
        p, b = predict_unrated(ratings, qs, us, i, j, summation)
        pred[c] = p
        line = per[i]
        line[13] += 1
        if p == 0:
            line[12] += 1
            continue
        e = p - int(tv)
        line[4 * b] += 1
        line[4 * b + 1] += e
        line[4 * b + 2] += abs(e)
        line[4 * b + 3] += e * e
    per = np.array(per, dtype=np.int64).reshape(nu, 16)
    return pred, per, per.sum(axis=0)


def evaluated_cells(truth, seed, keep):
    """the cells qrlsh_evaluate evaluates, row-major: (cells int64 [n][2], their truth)"""
    truth = np.asarray(truth)
    m = (truth != 0) & kept_mask(*truth.shape, seed, keep)
    cells = np.argwhere(m)
    return cells, truth[m]


def pred_matrix(shape, cells, pred):
    """pred_out: the prediction at evaluated cells, -1 elsewhere"""
    out = np.full(shape, -1, dtype=np.int64)
    out[cells[:, 0], cells[:, 1]] = pred
    return out


def sums_from_predictions(pred_out, truth):
    """per user (n covered, sum err, sum |err|, sum err^2, missed, evaluated) from a pred_out matrix: the three
    branches' words added up -- what can be said about EVERY cell without the branch"""
    pred_out, truth = np.asarray(pred_out, dtype=np.int64), np.asarray(truth, dtype=np.int64)
    hit = pred_out > 0
    e = np.where(hit, pred_out - truth, 0)
    return np.stack([hit.sum(1), e.sum(1), np.abs(e).sum(1), (e * e).sum(1), (pred_out == 0).sum(1),
                     (pred_out >= 0).sum(1)], axis=1)


def branch_sums(per_user):
    per_user = np.asarray(per_user)
    return np.concatenate([per_user[:, 0:4] + per_user[:, 4:8] + per_user[:, 8:12], per_user[:, 12:14]], axis=1)


def random_case(seed, nu, nq, longest_q, ku, fill=0.5):
    """random ratings 1..100; query lists of 0..longest_q neighbours (a list may name its own query, or one query
    twice); user lists of exactly ku distinct users (a list may name its own user).
    -> (ratings int32, (src, dst, milli) int32 arrays sorted by src, qs dict, us dict)"""
    rng = np.random.default_rng(seed)
    ratings = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < fill)).astype(np.int32)
    deg = rng.integers(0, longest_q + 1, size=nq)
    src = np.repeat(np.arange(nq), deg)
    dst = rng.integers(0, nq, size=len(src))
    mil = rng.integers(0, 1001, size=len(src))
    off = np.concatenate(([0], np.cumsum(deg)))
    qs = {j: {"indexes": dst[off[j]:off[j + 1]].astype(np.int64), "values": mil[off[j]:off[j + 1]] / 1000.0}
          for j in range(nq) if deg[j]}
    us = {}
    for u in range(nu):
        if ku:
            us[u] = {"indexes": rng.choice(nu, size=ku, replace=False).astype(np.int64),
                     "values": rng.integers(0, 1001, size=ku) / 1000.0}
    return ratings, tuple(x.astype(np.int32) for x in (src, dst, mil)), qs, us


QUEUE_EDGES = (1, 1023, 1024, 1025, 2047, 2048)   # rated cells of a row: around one drain of the sweeps' queue and its ring


def rows_with_exact_counts(truth, rows, counts, seed):
    """truth[row] = values 1..100 in exactly `count` columns (a seeded permutation's first ones), 0 elsewhere, for every
    (row, count); the rows' counts are asserted, so a case cannot stop covering them"""
    rng = np.random.default_rng(seed)
    nq = truth.shape[1]
    for row, count in zip(rows, counts):
        truth[row] = 0
        cols = rng.permutation(nq)[:count]
        truth[row, cols] = rng.integers(1, 101, size=count)
    assert [int((truth[r] != 0).sum()) for r in rows] == list(counts)
    return truth


def coo_of(qs):
    """(src, dst, milli) int32 arrays sorted by source of a {j: {'indexes', 'values'}} dict"""
    src, dst, mil = [], [], []
    for j in sorted(qs):
        idx = np.asarray(qs[j]["indexes"])
        src += [j] * len(idx)
        dst += idx.tolist()
        mil += np.rint(np.asarray(qs[j]["values"]) * 1000).astype(np.int64).tolist()
    return tuple(np.array(x, dtype=np.int32) for x in (src, dst, mil))
