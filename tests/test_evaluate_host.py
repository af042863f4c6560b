"""Evaluation (qrlsh.holdout / evaluate / evaluate_cells, Recommender.evaluate): what needs no device.  The restatement
the GPU tests hold the device to (tests/evaluate_cases.py) checked against the oracle's predict_cells and a direct loop
over the sample rule; Evaluation's figures; the host layer's argument checks (before the library touches a device) and
the C ABI's (fake pointers: each call fails a check before anything is dereferenced)."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
import evaluate_cases as EC
import predict_cases as PC

from qrlsh import _lib
from qrlsh.evaluate import Evaluation, is_kept, keep_word, mix64
import qrlsh


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("summation", [O.np_sum_order, PC.sequential_sum])
def test_restated_cell_equals_predict_cells_on_a_copy_with_the_cell_zeroed(summation):
    c = PC.build_case(7, nu=160, nq=400, tu=6, tq=12)
    rng = np.random.default_rng(3)
    rated = np.argwhere(c.ratings != 0)
    cells = np.concatenate([rated[rng.choice(len(rated), size=150, replace=False)], c.knife[:40]])
    for i, j in cells.tolist():
        z = c.ratings.copy()
        z[i, j] = 0
        want = int(O.predict_cells(z, c.qs, c.us, [[i, j]], summation=summation)[0])
        got, branch = EC.predict_unrated(c.ratings, c.qs, c.us, i, j, summation)
        assert got == want, (i, j)
        assert (branch == -1) == (want == 0)


def test_restatement_masks_a_list_entry_that_names_the_cell_itself():
    ratings, _, qs, us = EC.random_case(5, 12, 40, 6, 4)
    qs[3] = {"indexes": np.array([3, 7, 3, 9]), "values": np.array([0.9, 0.5, 0.4, 0.1])}
    us[2] = {"indexes": np.array([2, 5, 6, 1]), "values": np.array([0.9, 0.5, 0.4, 0.1])}
    ratings[2, [3, 7, 9]] = (80, 20, 40)
    ratings[[5, 6, 1], 3] = (10, 0, 30)
    z = ratings.copy()
    z[2, 3] = 0
    assert EC.predict_unrated(ratings, qs, us, 2, 3)[0] == int(O.predict_cells(z, qs, us, [[2, 3]])[0])
    assert EC.predict_unrated(ratings, qs, us, 2, 3) == EC.predict_unrated(z, qs, us, 2, 3)


def test_sample_rule_matches_a_direct_loop_over_the_library_mixer():
    lib = _lib.load()
    xs = [0, 1, 2**32, 2**63 + 12345, 2**64 - 1, 0x9E3779B97F4A7C15]
    assert [int(v) for v in EC.np_mix64(np.array(xs, dtype=np.uint64))] == [lib.qrlsh_mix64_host(x) for x in xs]
    assert [mix64(x) for x in xs] == [lib.qrlsh_mix64_host(x) for x in xs]
    nu, nq = 9, 37
    for seed, fraction in ((0, 0.3), (12345678901234567, 0.5), (2**64 - 1, 0.01)):
        keep = EC.keep_of(fraction)
        assert keep == keep_word(fraction)
        direct = np.array([[(lib.qrlsh_mix64_host(seed ^ (i << 32 | j)) >> 32) < keep for j in range(nq)]
                           for i in range(nu)])
        assert np.array_equal(EC.kept_mask(nu, nq, seed, keep), direct)
        assert np.array_equal(np.array([[is_kept(seed, keep, i, j) for j in range(nq)] for i in range(nu)]), direct)
        cells = np.argwhere(np.ones((nu, nq), dtype=bool))
        assert np.array_equal(EC.kept_cells(cells, seed, keep), direct.reshape(-1))
        # membership does not depend on nq
        assert np.array_equal(EC.kept_mask(nu, nq + 11, seed, keep)[:, :nq], direct)
    assert EC.kept_mask(4, 5, 7, EC.ALL).all() and not EC.kept_mask(4, 5, 7, 0).any()
    assert keep_word(1.0) == 2**32 and keep_word(0) == 0
    big = EC.kept_mask(300, 400, 9, EC.keep_of(0.25)).mean()
    assert abs(big - 0.25) < 0.01, big


def test_holdout_restatement_and_totals_are_column_sums():
    ratings, _, qs, us = EC.random_case(11, 20, 60, 6, 4)
    seed, keep = 5, EC.keep_of(0.3)
    train, n = EC.holdout_ref(ratings, seed, keep)
    gone = (train == 0) & (ratings != 0)
    assert n == gone.sum() and 0 < n < (ratings != 0).sum()
    assert np.array_equal(train[~gone], ratings[~gone])
    cells, values = EC.evaluated_cells(ratings, seed, keep)
    assert np.array_equal(cells, np.argwhere(gone)) and np.array_equal(values, ratings[gone])
    pred, per, totals = EC.evaluate_ref(train, qs, us, cells, values)
    assert np.array_equal(totals, per.sum(axis=0)) and totals[13] == n and not per[:, 14:].any()
    assert totals[0] + totals[4] + totals[8] + totals[12] == totals[13]
    # a hold-out cell is 0 in the train matrix: forcing it to 0 changes nothing
    assert np.array_equal(pred, O.predict_cells(train, qs, us, cells))
    # the sums that need no branch follow from the prediction matrix
    assert np.array_equal(EC.branch_sums(per), EC.sums_from_predictions(EC.pred_matrix(ratings.shape, cells, pred), ratings))
    # repeats count once each
    twice = EC.evaluate_ref(train, qs, us, np.concatenate([cells, cells[:5]]), np.concatenate([values, values[:5]]))
    assert twice[2][13] == n + 5


# ------------------------------------------------------------------------------------------------- Evaluation
def test_evaluation_figures_follow_from_the_integers():
    t = np.zeros(16, dtype=np.int64)
    t[0:4] = (3, -6, 10, 50)
    t[4:8] = (0, 0, 0, 0)
    t[8:12] = (5, 9, 11, 31)
    t[12], t[13] = 2, 10
    e = Evaluation(t)
    assert (e.n, e.covered, e.coverage) == (10, 8, 0.8)
    assert e.mae == 21 / 8 and e.bias == 3 / 8 and e.rmse == math.sqrt(81 / 8)
    assert e.by_branch["query"] == {"n": 3, "mae": 10 / 3, "rmse": math.sqrt(50 / 3), "bias": -2.0}
    assert e.by_branch["user"]["n"] == 0 and all(math.isnan(e.by_branch["user"][k]) for k in ("mae", "rmse", "bias"))
    assert e.by_branch["both"]["bias"] == 9 / 5
    assert isinstance(e.mae, float) and e.per_user is None and e.predictions is None and e.totals.dtype == np.int64
    none = Evaluation(np.zeros(16, dtype=np.int64))
    assert none.n == 0 and all(math.isnan(x) for x in (none.mae, none.rmse, none.bias, none.coverage))
    # sums beyond float64's integers stay exact up to the final division
    t = np.zeros(16, dtype=np.int64)
    t[0:4] = (2**40, 0, 2**40, 2**62)
    t[13] = 2**40
    assert Evaluation(t).rmse == math.sqrt(2**62 / 2**40)


# ------------------------------------------------------------------------------------------------- host layer
def test_host_layer_checks_its_arguments_before_any_device_work():
    ratings, coo, qs, us = EC.random_case(2, 6, 30, 4, 3)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="fraction"):
            qrlsh.holdout(ratings, bad)
        with pytest.raises(ValueError, match="fraction"):
            qrlsh.evaluate(ratings, *coo, us, fraction=bad)
    with pytest.raises(ValueError, match="truth has shape"):
        qrlsh.evaluate(ratings, *coo, us, truth=ratings[:, :-1])
    with pytest.raises(ValueError, match="truth"):
        qrlsh.evaluate(ratings, *coo, us, truth=ratings.astype(np.float64))
    with pytest.raises(ValueError, match="sum_order"):
        qrlsh.evaluate(ratings, *coo, us, sum_order="tree")
    with pytest.raises(ValueError, match="seed"):
        qrlsh.evaluate(ratings, *coo, us, seed=-1)
    with pytest.raises(ValueError, match="user id"):
        qrlsh.evaluate_cells(ratings, *coo, us, [0, 6], [1, 1], [5, 5])
    with pytest.raises(ValueError, match="query id"):
        qrlsh.evaluate_cells(ratings, *coo, us, [0, 5], [1, 30], [5, 5])
    with pytest.raises(ValueError, match="differ in length"):
        qrlsh.evaluate_cells(ratings, *coo, us, [0, 5], [1], [5, 5])
    assert set(("holdout", "evaluate", "evaluate_cells", "Evaluation")) <= set(qrlsh.__all__)


def test_recommender_evaluate_checks_before_it_needs_a_run():
    import recommender as R
    rec = R.Recommender()
    with pytest.raises(ValueError, match="fraction"):
        rec.evaluate(fraction=2)
    with pytest.raises(ValueError, match="cells"):
        rec.evaluate(holdout=True, cells=([0], [0], [1]))
    rec.ratings, rec.queriesIDs = np.zeros((2, 3), dtype=np.int64), np.arange(3)
    for kw in ({}, {"holdout": True}):
        with pytest.raises(ValueError, match="no live lists"):
            rec.evaluate(**kw)


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def test_c_abi_refuses_bad_arguments_before_any_device_work():
    lib = _lib.load()
    for name in ("qrlsh_ratings_holdout", "qrlsh_evaluate_workspace_bytes", "qrlsh_evaluate", "qrlsh_evaluate_cells"):
        assert name in _lib.SIGNATURES
    r, t, qo, qi, qm, ui, uv, pu, to, fl, ws = _fake(11)

    def ev(nu=4, nq=1000, ku=8, order=0, keep=2**32, flags=fl, totals=to, work=ws, nbytes=1 << 20, truth=t):
        return lib.qrlsh_evaluate(r, truth, nu, nq, qo, qi, qm, ui, uv, ku, 0.6, 0.4, 60.0, order, 0, keep, pu, totals, None,
                                  flags, work, nbytes, None)

    for kw in (dict(nu=-1), dict(nq=2**31), dict(nu=2**31), dict(ku=65), dict(order=2), dict(keep=2**32 + 1),
               dict(flags=None), dict(totals=None), dict(truth=None), dict(work=None), dict(nbytes=8),
               dict(work=ctypes.c_void_p(0x100004))):
        assert ev(**kw) == _lib.QRLSH_EINVAL, kw
        assert lib.qrlsh_last_error()

    cu, cq, cv = _fake(3)

    def cells(nu=4, nq=1000, ku=8, order=0, m=5, users=cu, flags=fl, totals=to):
        return lib.qrlsh_evaluate_cells(r, nu, nq, qo, qi, qm, ui, uv, ku, 0.6, 0.4, 60.0, order, users, cq, cv, m, None,
                                        totals, flags, None)

    for kw in (dict(nu=-1), dict(ku=65), dict(order=-1), dict(m=-1), dict(users=None), dict(flags=None), dict(totals=None)):
        assert cells(**kw) == _lib.QRLSH_EINVAL, kw

    def hold(nu=4, nq=10, keep=5, inp=r, out=t, count=to):
        return lib.qrlsh_ratings_holdout(inp, nu, nq, 0, keep, out, count, None)

    for kw in (dict(nu=-1), dict(nq=2**31), dict(keep=2**32 + 1), dict(inp=None), dict(out=r), dict(count=None)):
        assert hold(**kw) == _lib.QRLSH_EINVAL, kw


def test_workspace_size():
    lib = _lib.load()
    size = lib.qrlsh_evaluate_workspace_bytes
    assert size(0, 10) == 0 and size(10, 0) == 0
    # [users x slices x 16 int64][ceil(users / 64) x 16 int64]; about 4096 workgroups, at least 1024 columns a slice
    assert size(8, 131072) == (8 * 128 + 1) * 128
    assert size(8, 1025) == (8 * 2 + 1) * 128
    assert size(333, 5003) == (333 * 5 + 6) * 128
    assert size(2000, 100000) == (2000 * 3 + 32) * 128
    assert size(5000, 100000) == (5000 + 79) * 128
