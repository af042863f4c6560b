"""Recommendations on the device (qrlsh.top_k / Recommender.recommend) against the numpy restatement of
tests/test_recommend_host.py: exact (idx, val, avail) on the golden fixtures, end to end through the drop-in
Recommender, on random shapes with heavy ties, and across every form (slices, window / radix refinement, rows form)."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load
from test_recommend_host import SCORES, reference_topk, restate

pytestmark = pytest.mark.gpu

DEV = "cuda"
GENERATOR_SETS = ["cfg1", "cfg1b", "cfg2"]


def restate_all(ratings, pred, k):
    """restate() for every row at once (one lexsort over the eligible cells): (idx, val, avail)"""
    ratings, pred = np.asarray(ratings), np.asarray(pred)
    nu = ratings.shape[0]
    rows, cols = np.nonzero((ratings == 0) & (pred != 0))
    v = pred[rows, cols].astype(np.int64)
    o = np.lexsort((cols, -v, rows))
    rows, cols, v = rows[o], cols[o], v[o]
    avail = np.bincount(rows, minlength=nu).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(avail)[:-1]))
    rank = np.arange(len(rows)) - start[rows]
    keep = rank < k
    idx = np.full((nu, k), -1, dtype=np.int64)
    val = np.zeros((nu, k), dtype=np.int64)
    idx[rows[keep], rank[keep]] = cols[keep]
    val[rows[keep], rank[keep]] = v[keep]
    return idx, val, avail


def dev_topk(ratings, pred, k, **kw):
    import qrlsh
    idx, val, avail = qrlsh.top_k(ratings, pred, k, device=DEV, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), avail.cpu().numpy()


def assert_exact(got, want, what=""):
    for name, g, w in zip(("idx", "val", "avail"), got, want):
        assert g.shape == w.shape, "%s %s shape %s != %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:5]
            raise AssertionError("%s %s differs at %s" % (what, name, bad.tolist()))


def test_restate_all_matches_restate():
    rng = np.random.RandomState(3)
    r = rng.randint(0, 3, size=(40, 57)) * (rng.rand(40, 57) < 0.5)
    p = rng.randint(-5, 6, size=(40, 57))
    for k in (1, 4, 57, 100):
        assert_exact(restate_all(r, p, k), restate(r, p, k), "k=%d" % k)


# ---------------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("name", SCORES)
def test_golden_exact_and_tie_aware_against_reference(name):
    g = load(name)
    ratings, final = g["ratings"], g["final"]
    to_predict = [tuple(x) for x in g["to_predict"]]
    for k in (1, 5, 11, 1024):
        got = dev_topk(ratings, final, k)
        assert_exact(got, restate(ratings, final, k), "%s k=%d" % (name, k))
        idx, val, avail = got
        for u in range(ratings.shape[0]):
            just_scored, ref_cols = reference_topk(to_predict, final, u, k)
            n = min(k, len(just_scored))
            assert avail[u] == len(just_scored)
            assert np.array_equal(val[u, :n], final[u][ref_cols])
            assert all(final[u][c] == v for c, v in zip(idx[u, :n], val[u, :n]))


# ---------------------------------------------------------------------------------------------------- 2. end to end
def _recommender_on(sub):
    import pandas as pd
    import recommender as R
    g = load(sub + "_scores")
    gdir = os.path.join(GOLDEN, sub)
    rec = R.Recommender()
    rec.verbose = False
    dataset = pd.read_csv(os.path.join(gdir, "dataset.csv"))
    rec.datasetFeatures = list(dataset.columns)[1:]
    users = pd.read_csv(os.path.join(gdir, "users.csv"), header=None)
    queries, qids = rec.parse_queries(os.path.join(gdir, "queries.csv"))
    ratings = pd.read_csv(os.path.join(gdir, "utility_matrix.csv"))
    ratings.insert(0, "user", users[0].to_numpy())
    ratings.columns = ["user"] + qids
    rec.init(users, queries, qids, dataset, ratings)
    R.PERM = int(g["P"])
    np.random.seed(int(g["seed"]))
    return rec, g


@pytest.mark.parametrize("sub", GENERATOR_SETS)
def test_recommender_recommend_end_to_end(sub):
    import qrlsh
    import recommender as R
    from qrlsh import predict
    rec, g = _recommender_on(sub)
    to_predict, final, missed = rec.compute_scores()
    assert np.array_equal(final.to_numpy(), g["final"])
    fin = final.to_numpy()
    for k in (1, 7, 1024):
        out = rec.recommend(final, k)
        idx, val, avail = restate(rec.ratings, fin, k)
        assert sorted(out) == list(range(fin.shape[0]))
        for u, e in out.items():
            n = min(k, int(avail[u]))
            assert e["available"] == avail[u]
            assert e["indexes"].dtype == np.int64 and e["values"].dtype == np.int64
            assert np.array_equal(e["indexes"], idx[u, :n]) and np.array_equal(e["values"], val[u, :n])
    # the device-resident path: fill_predictions' tensor and the ratings on the device, nothing copied in between
    res = rec.last_result
    usim = rec.compute_userSimilarities()
    pt = predict.fill_predictions(rec.ratings, res.src, res.dst, res.val, usim, R.QUERY_WEIGHT, R.USER_WEIGHT,
                                  R.DEFAULT_MEAN, DEV, sum_order=rec.sum_order)
    rt = torch.from_numpy(rec.ratings.astype(np.int32)).to(DEV)
    assert np.array_equal(pt.cpu().numpy(), fin)
    for k in (3, 1024):
        idx, val, avail = qrlsh.top_k(rt, pt, k)
        out = rec.recommend(final, k)
        for u, e in out.items():
            n = e["available"] if e["available"] < k else k
            assert np.array_equal(idx[u, :n].cpu().numpy(), e["indexes"])
            assert np.array_equal(val[u, :n].cpu().numpy(), e["values"])
        assert np.array_equal(avail.cpu().numpy(), [out[u]["available"] for u in range(fin.shape[0])])


# ---------------------------------------------------------------------------------------------------- 3. shapes
def _heavy_ties(nu, nq, seed):
    """bench.py's N1 ratings (1..100, 75 % unrated) and predictions 1..100 on every cell, 2 % of them 0"""
    rng = np.random.RandomState(seed)
    r = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    r[rng.rand(nu, nq) < 0.75] = 0
    p = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    p[rng.rand(nu, nq) < 0.02] = 0
    return r, p


def test_n1_shape_heavy_ties():
    nu, nq = 2000, 100_000
    rng = np.random.RandomState(11)
    r = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    r[rng.rand(nu, nq) < 0.75] = 0
    p = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    rt, pt = torch.from_numpy(r).to(DEV), torch.from_numpy(p).to(DEV)
    mask = r == 0
    avail = mask.sum(axis=1)
    srt = np.sort(np.where(mask, p, np.iinfo(np.int32).min), axis=1)   # ascending; the top k are at the end
    sample = np.random.RandomState(5).choice(nu, 128, replace=False)
    for k in (1, 28, 1024):
        idx, val, av = dev_topk(rt, pt, k)
        assert np.array_equal(av, avail)
        assert np.array_equal(val, srt[:, ::-1][:, :k])
        want = restate(r, p, k, users=sample)
        assert_exact((idx[sample], val[sample], av[sample]), want, "k=%d sample" % k)


def test_long_rows_multi_slice():
    r, p = _heavy_ties(8, 3_000_000, 12)
    rt, pt = torch.from_numpy(r).to(DEV), torch.from_numpy(p).to(DEV)
    for k in (1, 1024):
        assert_exact(dev_topk(rt, pt, k), restate(r, p, k), "8x3M k=%d" % k)


def test_short_rows_unaligned():
    r, p = _heavy_ties(100_000, 37, 13)
    want = restate_all(r, p, 10)
    assert_exact(dev_topk(r, p, 10), want, "rows form")
    assert_exact(dev_topk(r[:3000], p[:3000], 10, slices=1), restate_all(r[:3000], p[:3000], 10), "slice form nq=37")
    assert_exact(dev_topk(r[:3000], p[:3000], 10, slices=7), restate_all(r[:3000], p[:3000], 10), "7 slices nq=37")
    r2, p2 = _heavy_ties(300, 10_007, 14)
    for s in (0, 1, 5):
        assert_exact(dev_topk(r2, p2, 50, slices=s), restate_all(r2, p2, 50), "nq=10007 slices=%d" % s)


def test_edge_shapes():
    # nq = 1, both forms
    r, p = _heavy_ties(50, 1, 15)
    for s in (0, 1, 3):
        assert_exact(dev_topk(r, p, 4, slices=s), restate_all(r, p, 4), "nq=1 slices=%d" % s)
    # a row with no eligible cell, a fully rated row, rows with fewer than k eligible cells
    r, p = _heavy_ties(6, 5000, 16)
    p[0] = 0                      # nothing predicted
    r[1] = 7                      # fully rated
    r[2, :] = 3
    r[2, [10, 4000, 4999]] = 0    # three eligible cells
    for s in (0, 1, 4):
        for k in (1, 3, 1024):
            got = dev_topk(r, p, k, slices=s)
            assert_exact(got, restate_all(r, p, k), "edge rows slices=%d k=%d" % (s, k))
            assert got[2][0] == 0 and got[2][1] == 0 and np.all(got[0][:2] == -1)
    # a fully rated matrix, both forms
    full = np.ones((9, 3000), dtype=np.int32)
    for s in (0, 2):
        idx, val, av = dev_topk(full, full, 5, slices=s)
        assert np.all(idx == -1) and np.all(val == 0) and np.all(av == 0)
    # no columns at all
    idx, val, av = dev_topk(np.zeros((4, 0), np.int32), np.zeros((4, 0), np.int32), 2)
    assert np.all(idx == -1) and np.all(val == 0) and np.all(av == 0)


# ---------------------------------------------------------------------------------------------------- 4. forms
def _forms_agree(r, p, k, what):
    want = restate_all(r, p, k)
    rt, pt = torch.from_numpy(r).to(DEV), torch.from_numpy(p).to(DEV)
    for s in (1, 2, 7, 0):
        for lo in (0, 10**6, -2**31):
            assert_exact(dev_topk(rt, pt, k, slices=s, lo=lo), want, "%s slices=%d lo=%d k=%d" % (what, s, lo, k))


def test_forms_agree_window_and_refinement():
    r, p = _heavy_ties(64, 200_000, 17)
    for k in (1, 37, 1024):
        _forms_agree(r, p, k, "ties")


def test_forms_agree_full_int32_range():
    rng = np.random.RandomState(18)
    r = (rng.rand(48, 70_001) < 0.3).astype(np.int32) * 5
    p = rng.randint(-2**31, 2**31, size=r.shape, dtype=np.int64).astype(np.int32)
    p[:, ::97] = 2**31 - 1
    p[:, 5::101] = -2**31 + 1
    p[:, 7::103] = -2**31
    p[:, 9::89] = -1
    p[3] = rng.randint(-50, 0, size=p.shape[1])      # an all-negative row
    for k in (1, 300, 1024):
        _forms_agree(r, p, k, "int32 range")


def test_forms_agree_one_coarse_digit():
    # distinct values inside one 12-bit top digit of the key and a few inside one 20-bit digit: rounds 2 and 3 decide
    rng = np.random.RandomState(19)
    r = np.zeros((16, 150_000), dtype=np.int32)
    p = (5_000_000 + rng.randint(0, 1 << 20, size=r.shape)).astype(np.int32)
    p[:, ::7] = 5_000_000 + rng.randint(0, 256, size=p[:, ::7].shape)
    for k in (1, 500, 1024):
        _forms_agree(r, p, k, "coarse digit")


# ---------------------------------------------------------------------------------------------------- 5. users
def test_user_subsets_match_all_users():
    r, p = _heavy_ties(300, 20_000, 20)
    rt, pt = torch.from_numpy(r).to(DEV), torch.from_numpy(p).to(DEV)
    for k in (5, 1024):
        all_ = dev_topk(rt, pt, k)
        for users in ([299, 3, 150, 0], [7, 7, 7, 2, 7], [42], list(range(299, -1, -1))):
            for form in (list, np.asarray, lambda x: torch.tensor(x, device=DEV)):
                got = dev_topk(rt, pt, k, users=form(users))
                sel = np.asarray(users)
                assert_exact(got, tuple(a[sel] for a in all_), "users %s" % users[:5])


def test_out_of_range_user_raises_from_flag_and_leaves_no_fault():
    import qrlsh
    r, p = _heavy_ties(30, 5000, 21)
    for s in (0, 1):
        for bad in ([3, 30], [-1], [2**40, 0]):
            with pytest.raises(ValueError):
                qrlsh.top_k(r, p, 4, users=torch.tensor(bad, dtype=torch.int64, device=DEV), slices=s)
    short = _heavy_ties(30, 40, 22)
    with pytest.raises(ValueError):
        qrlsh.top_k(*short, 4, users=torch.tensor([0, 31], device=DEV))
    torch.cuda.synchronize()
    assert_exact(dev_topk(r, p, 4), restate_all(r, p, 4), "after the flagged calls")


# ---------------------------------------------------------------------------------------------------- 6. row blocks
def test_all_users_split_into_row_blocks_match_the_single_call(monkeypatch):
    """37 rows under a budget that admits 10 per call (slices=1: the rows form has no workspace, so nothing would
    split): 37 -> 19 -> 10, four library calls, the last of 7 rows, served by the ids the split had to make"""
    from qrlsh import _lib, recommend
    lib = _lib.load()
    r, p = _heavy_ties(37, 40, 23)
    want = dev_topk(r, p, 5, slices=1)
    assert_exact(want, restate_all(r, p, 5), "one call")
    calls = []
    real = lib.qrlsh_recommend_topk

    def counted(*args):
        calls.append(args[5])
        return real(*args)
    monkeypatch.setattr(lib, "qrlsh_recommend_topk", counted)
    monkeypatch.setattr(recommend, "WORKSPACE_BUDGET", int(lib.qrlsh_recommend_workspace_bytes(10, 40, 5, 1)))
    assert_exact(dev_topk(r, p, 5, slices=1), want, "row blocks")
    assert calls == [10, 10, 10, 7]
