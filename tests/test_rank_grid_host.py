"""The ranking grid without a device: the restatement of tests/rank_grid_cases.py against rank_eval_ref over host-cut
lists, what the weights do to the order of a list, RankingGridEvaluation's figures, index order and best(), the
stitching of a long weight list, and every argument check.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import predict_cases as PC
import rank_eval_cases as REC
import rank_grid_cases as RGC
import tune_cases as TC

from qrlsh import rankgrid, tune
from qrlsh.ranking import RankingEvaluation


@pytest.fixture(scope="module")
def tiny():
    train, truth, coo, qs, us, users = RGC.main_case(seed=5, nu=8, nq=120, held=0.4)
    return train, truth, coo, qs, us, users[:8] + [2, 2]


def test_the_restatement_is_rank_eval_ref_over_host_cut_lists(tiny):
    """at the default weights rank_eval_ref predicts through oracle.predict_cells: cutting the lists on the host and
    calling it once per pair of cuts is the existing route; the grid's restatement must give the same words"""
    train, truth, _, qs, us, users = tiny
    k, relevant, gains = 5, 50, REC.primes(5)
    q_cuts, u_cuts = [0, 7, 64], [0, 3, 9]
    for summation in (O.np_sum_order, PC.sequential_sum):
        per, totals, idx = RGC.rank_grid_ref(train, truth, qs, us, users, k, relevant, gains, q_cuts, u_cuts,
                                             [TC.DEFAULT], summation)
        assert totals[2, 2, 0, 1] > 0 and totals[2, 2, 0, 6] > 100
        for a, cq in enumerate(q_cuts):
            for b, cu in enumerate(u_cuts):
                cqs, cus = RGC.host_cut_lists(qs, us, cq, cu)
                i, _, _, p, t = REC.rank_eval_ref(train, truth, cqs, cus, users, k, relevant, "heldout", gains,
                                                  summation=summation)
                assert np.array_equal(per[:, a, b, 0], p) and np.array_equal(totals[a, b, 0], t), (cq, cu)
                assert np.array_equal(idx[:, a, b, 0], i)
        assert not totals[0, 0, 0, :5].any() and totals[0, 0, 0, 8] == len(users)      # both sides off: nothing listed
        assert np.array_equal(per[8], per[2]) and np.array_equal(per[9], per[2])       # a user named three times


def test_the_weights_change_the_order_not_only_the_values(tiny):
    train, truth, _, qs, us, users = tiny
    per, totals, idx = RGC.rank_grid_ref(train, truth, qs, us, users, 5, 50, REC.primes(5), [64], [64],
                                         [RGC.QUERY_ONLY, RGC.USER_ONLY, (0.0, 0.0, 60.0), (0.6, -0.4, 60.0)])
    assert sum(a.tolist() != b.tolist() for a, b in zip(idx[:, 0, 0, 0], idx[:, 0, 0, 1])) > 4
    assert not np.array_equal(totals[0, 0, 0, :5], totals[0, 0, 1, :5])
    # every word but the list's is the same for every setting: relevant and test cells, requests
    assert (totals[0, 0, :, 5] == totals[0, 0, 0, 5]).all() and (totals[0, 0, :, 6] == totals[0, 0, 0, 6]).all()
    assert (totals[0, 0, :, 11] == totals[0, 0, 0, 11]).all()
    # both weights 0 with both sides present predicts 0: such cells are not listed
    assert totals[0, 0, 2, 7] < totals[0, 0, 0, 7]


def _grid(hits, listed, relevant, dcg, ideal, with_hit=None, with_rel=None, q_cuts=(64,), u_cuts=(64,)):
    n = len(hits)
    t = np.zeros((n, 16), dtype=np.int64)
    t[:, 0], t[:, 1], t[:, 2], t[:, 4], t[:, 5], t[:, 11] = listed, hits, listed, dcg, relevant, ideal
    t[:, 8] = 10
    t[:, 9] = 10 if with_rel is None else with_rel
    t[:, 10] = hits if with_hit is None else with_hit
    w = n // (len(q_cuts) * len(u_cuts))
    return rankgrid.RankingGridEvaluation(list(q_cuts), list(u_cuts), [(0.1 * k, 0.5, 60.0) for k in range(w)], t)


def test_figures_are_ranking_evaluations_divisions():
    g = _grid([3, 0, 5], [10, 0, 10], [6, 6, 0], [70, 0, 90], [100, 100, 0], with_rel=[10, 10, 0])
    for w in range(3):
        one = RankingEvaluation(g.totals[0, 0, w])
        for name in ("precision", "recall", "ndcg", "hit_rate"):
            a, b = getattr(g, name)[0, 0, w], getattr(one, name)
            assert (np.isnan(a) and np.isnan(b)) or a == b, (w, name)
    assert g.precision[0, 0, 0] == 0.3 and np.isnan(g.precision[0, 0, 1]) and np.isnan(g.ndcg[0, 0, 2])
    assert g.totals.shape == (1, 1, 3, 16) and g.totals.dtype == np.int64 and g.per_request is None


def test_best_takes_the_highest_figure_the_lowest_index_on_ties_and_never_nan():
    g = _grid([2, 4, 4, 0, 9], [10, 10, 10, 0, 10], [8, 8, 8, 8, 0], [50, 80, 80, 0, 99], [100, 100, 100, 100, 0])
    assert g.best() == (64, 64, (0.1, 0.5, 60.0), 1)              # settings 1 and 2 tie on 0.8: the lower index
    assert np.isnan(g.ndcg[0, 0, 4]) and np.isnan(g.precision[0, 0, 3])
    assert g.best("precision")[3] == 4                            # 0.9; its ndcg and recall are nan, its precision is not
    assert g.best("precision", min_recall=0.1)[3] == 1            # a recall of nan does not clear a bar above 0
    assert g.best("recall")[3] == 1 and g.best("hit_rate")[3] == 4
    assert g.best("ndcg", min_recall=0.5) == (64, 64, (0.1, 0.5, 60.0), 1)
    with pytest.raises(ValueError, match="no setting"):
        g.best(min_recall=0.6)
    for bad in ("rmse", "mrr", None):
        with pytest.raises(ValueError, match="metric"):
            g.best(bad)
    empty = _grid([0, 0], [0, 0], [0, 0], [0, 0], [0, 0], with_rel=[0, 0])
    assert all(np.isnan(getattr(empty, m)).all() for m in rankgrid.METRICS)
    with pytest.raises(ValueError, match="no setting"):
        empty.best()
    # the index runs (cq * CU + cu) * W + w
    dcg = [9, 9, 9, 9, 9, 9, 9, 50, 9, 9, 9, 9]
    g = _grid(np.full(12, 1), np.full(12, 10), np.full(12, 5), dcg, np.full(12, 100), q_cuts=(0, 8), u_cuts=(1, 5, 9))
    assert g.best() == (8, 1, (0.1, 0.5, 60.0), 7) and g.setting(7) == g.best()[:3]
    assert g.setting(0) == (0, 1, (0.0, 0.5, 60.0)) and g.setting(11) == (8, 9, (0.1, 0.5, 60.0))
    # tune's result class and metrics are as they were
    assert tune.METRICS == ("rmse", "mae", "bias") and rankgrid.METRICS == ("ndcg", "precision", "recall", "hit_rate")


def test_a_long_weight_list_is_stitched_along_the_weights_with_sixteen_words():
    calls = []

    def stub(lo, hi):
        calls.append((lo, hi))
        w = torch.arange(lo, hi, dtype=torch.int64)
        totals = (torch.arange(2).view(2, 1, 1, 1) * 1000000 + torch.arange(2).view(1, 2, 1, 1) * 10000
                  + w.view(1, 1, -1, 1) * 100 + torch.arange(16).view(1, 1, 1, 16))
        per = totals[..., :8].unsqueeze(0).repeat(3, 1, 1, 1, 1)
        return totals, per, torch.tensor([0], dtype=torch.int64)

    totals, per, flags = tune.sweep(40, 2, 2, stub)
    assert calls == [(0, 32), (32, 40)] and tuple(totals.shape) == (2, 2, 40, 16) and tuple(per.shape) == (3, 2, 2, 40, 8)
    g = rankgrid.RankingGridEvaluation([1, 2], [3, 4], np.zeros((40, 3)), totals.numpy(), per)
    for index in (0, 39, 40, 159):
        cq, cu, w = index // 80, (index // 40) % 2, index % 40
        assert g.totals.reshape(-1, 16)[index].tolist() == [cq * 1000000 + cu * 10000 + w * 100 + k for k in range(16)]
        assert g.setting(index)[:2] == ([1, 2][cq], [3, 4][cu])


def test_arguments_are_checked_before_anything_is_uploaded(tiny):
    train, truth, coo, qs, us, users = tiny
    w = [TC.DEFAULT]

    def call(**kw):
        args = dict(k=5, relevant=50, weights=w, device="none")
        args.update(kw)
        k, relevant, weights = args.pop("k"), args.pop("relevant"), args.pop("weights")
        tr, tt = args.pop("train", train), args.pop("truth", truth)
        return rankgrid.evaluate_ranking_grid(tr, tt, *coo, us, k, relevant, weights, **args)

    for bad in (0, 1025, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must"):
            call(k=bad)
    for bad in (0, -3, 2**31, 1.5, True):
        with pytest.raises(ValueError, match="relevant"):
            call(relevant=bad)
    for bad in ([], [-1], [1, 2, 3, 4, 5], [1.5], [True]):
        with pytest.raises(ValueError, match="q_cuts"):
            call(q_cuts=bad)
        with pytest.raises(ValueError, match="u_cuts"):
            call(u_cuts=bad)
    for bad in ([], [0.6, 0.4, 60], [[0.6, 0.4]], [[0.6, 0.4, float("inf")]]):
        with pytest.raises(ValueError, match="weights"):
            call(weights=bad)
    with pytest.raises(ValueError, match="sum_order"):
        call(sum_order="tree")
    with pytest.raises(ValueError, match="truth"):
        call(truth=truth[:, :5])
    with pytest.raises(ValueError, match="user id"):
        call(users=[0, train.shape[0]])
    with pytest.raises(ValueError, match="users"):
        call(users=[0.5])
    for bad in ([1, 2, 3], [5, 4, 3, 2, -1], [1.0] * 5):
        with pytest.raises(ValueError, match="gains"):
            call(gains=bad)
    with pytest.raises(ValueError, match="int64"):
        call(gains=[2**62] * 5)
