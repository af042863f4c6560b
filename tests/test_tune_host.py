"""The grid evaluation without a device: the restatement of tests/tune_cases.py against evaluate_cases', the prefix
property the feature rests on, what a cut and a sum order change, GridEvaluation.best and the splitting of a long
weight list into library calls.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import evaluate_cases as EC
import predict_cases as PC
import tune_cases as TC

from qrlsh import tune


def test_default_setting_is_evaluate_ref_through_the_word_mapping():
    ratings, _, qs, us = EC.random_case(5, 12, 300, 20, 9)
    cells, values = EC.evaluated_cells(ratings, 3, EC.keep_of(0.4))
    assert len(cells) > 400
    for summation in (O.np_sum_order, PC.sequential_sum):
        pred, per, totals = EC.evaluate_ref(ratings, qs, us, cells, values, summation=summation)
        gpred, gper, gtotals = TC.grid_ref(ratings, qs, us, cells, values, [TC.WHOLE], [TC.WHOLE], [TC.DEFAULT],
                                           summation=summation)
        assert np.array_equal(gpred[:, 0, 0, 0], pred)
        assert np.array_equal(gper[:, 0, 0, 0], TC.words8(per)) and np.array_equal(gtotals[0, 0, 0], TC.words8(totals))
        assert gtotals[0, 0, 0, 0] > 0 and gtotals[0, 0, 0, 6] > 0 and gtotals[0, 0, 0, 4] + gtotals[0, 0, 0, 0] == len(cells)


def test_a_stored_list_cut_short_is_the_list_a_smaller_k_stores():
    """oracle.topk orders (value descending, id ascending): its rows at K' are the first K' entries of its rows at K,
    with ties in value across the cut; the same for the reference's user cut argsort[::-1][:K]"""
    rng = np.random.default_rng(11)
    n = 60
    i, j = np.triu_indices(n, 1)
    pick = rng.random(len(i)) < 0.6
    pairs = (i[pick].astype(np.uint64) << np.uint64(32)) | j[pick].astype(np.uint64)
    milli = rng.integers(0, 6, size=len(pairs)).astype(np.int32) * 100      # six values: ties everywhere
    K = 28
    src, dst, val = O.topk(pairs, milli, K)
    rows = {q: (dst[src == q], val[src == q]) for q in range(n)}
    assert max(len(r[0]) for r in rows.values()) == K
    for k2 in (1, 7, 8, 9, 19):
        s2, d2, v2 = O.topk(pairs, milli, k2)
        tied = 0
        for q in range(n):
            want_d, want_v = rows[q][0][:k2], rows[q][1][:k2]
            assert np.array_equal(d2[s2 == q], want_d) and np.array_equal(v2[s2 == q], want_v), (k2, q)
            tied += len(rows[q][1]) > k2 and rows[q][1][k2 - 1] == rows[q][1][k2]
        assert tied > 10                                                      # the cut falls inside a run of ties
    # the reference's user cut: one argsort, reversed, cut at K
    sim = rng.integers(0, 5, size=(40, 40)) / 4.0
    for row in sim:
        full = np.argsort(row)[::-1]
        for k2 in (1, 5, 9):
            assert np.array_equal(np.argsort(row)[::-1][:k2], full[:19][:k2])


@pytest.fixture(scope="module")
def knife():
    return PC.build_case(16, nu=60, nq=700, tu=6, tq=60, user_longest=32)


def test_a_cut_and_the_sum_order_move_knife_edge_cells(knife):
    """between the cuts 8 and 9 (the pairwise order changes shape at 8) and between the two orders some knife-edge cell
    changes its prediction: a sweep that reused one accumulation for two cuts, or one order for both, would show"""
    c = knife
    assert len(c.knife) > 100
    values = np.full(len(c.knife), 50)
    got = {name: TC.grid_ref(c.ratings, c.qs, c.us, c.knife, values, [8, 9, 64], [8, 9, 64], [TC.DEFAULT],
                             summation=s)[0][:, :, :, 0]
           for name, s in (("pairwise", O.np_sum_order), ("sequential", PC.sequential_sum))}
    pw = got["pairwise"]
    assert (pw[:, 0, 2] != pw[:, 1, 2]).any() and (pw[:, 2, 0] != pw[:, 2, 1]).any()      # cut 8 against cut 9
    assert (pw[:, 2, 2] != got["sequential"][:, 2, 2]).any()                              # the whole lists, both orders
    # and a cut past every list is the whole list
    whole = TC.grid_ref(c.ratings, c.qs, c.us, c.knife, values, [1000], [1000], [TC.DEFAULT])[0][:, 0, 0, 0]
    assert np.array_equal(whole, pw[:, 2, 2])


def _grid(n, sq, cells=None, q_cuts=(64,), u_cuts=(64,)):
    """a GridEvaluation over W weight triples from per-setting n and sum err^2 (sum |err| = n, sum err = 0)"""
    n, sq = np.asarray(n, dtype=np.int64).reshape(-1), np.asarray(sq, dtype=np.int64).reshape(-1)
    cells = np.full(len(n), 100) if cells is None else np.asarray(cells)
    t = np.zeros((len(n), 8), dtype=np.int64)
    t[:, 0], t[:, 2], t[:, 3], t[:, 5] = n, n, sq, cells
    t[:, 4] = t[:, 5] - t[:, 0]
    w = len(n) // (len(q_cuts) * len(u_cuts))
    return tune.GridEvaluation(list(q_cuts), list(u_cuts), [(0.1 * k, 0.5, 60.0) for k in range(w)], t)


def test_best_takes_the_lowest_figure_the_lowest_index_on_ties_and_never_nan():
    g = _grid([50, 50, 50, 0, 10], [200, 100, 100, 0, 10])
    assert g.n.shape == (1, 1, 5) and np.isnan(g.rmse[0, 0, 3]) and g.rmse[0, 0, 1] == np.sqrt(2.0)
    assert g.coverage[0, 0, 4] == 0.1 and g.mae[0, 0, 0] == 1.0 and g.bias[0, 0, 0] == 0.0
    assert g.best() == (64, 64, (0.4, 0.5, 60.0), 4)
    q, u, w, index = g.best(min_coverage=0.5)          # settings 1 and 2 tie: the lower index
    assert index == 1 and w == (0.1, 0.5, 60.0)
    assert g.best("mae", min_coverage=0.5)[3] == 0       # every mae is 1: the first
    with pytest.raises(ValueError, match="no setting"):
        g.best(min_coverage=0.6)
    with pytest.raises(ValueError, match="metric"):
        g.best("ndcg")
    # nothing evaluated at all: nan everywhere, nothing qualifies
    empty = _grid([0, 0], [0, 0], cells=[0, 0])
    assert np.isnan(empty.coverage).all() and np.isnan(empty.rmse).all()
    with pytest.raises(ValueError, match="no setting"):
        empty.best()
    # the index runs (cq * CU + cu) * W + w
    g = _grid(np.full(12, 10), [9, 9, 9, 9, 9, 9, 9, 1, 9, 9, 9, 9], q_cuts=(0, 8), u_cuts=(1, 5, 9))
    assert g.best() == (8, 1, (0.1, 0.5, 60.0), 7) and g.setting(7) == g.best()[:3]


def test_a_long_weight_list_runs_as_successive_calls_and_is_stitched():
    assert tune.chunks_of(8, 4, 4) == [(0, 8)]
    assert tune.chunks_of(40, 2, 2) == [(0, 32), (32, 40)]
    assert tune.chunks_of(129, 1, 1) == [(0, 128), (128, 129)]
    assert tune.chunks_of(5, 4, 4, limit=16) == [(k, k + 1) for k in range(5)]
    calls = []

    def stub(lo, hi):
        """totals word = 1000 * setting-in-grid coordinates, so a misplaced chunk shows"""
        calls.append((lo, hi))
        w = torch.arange(lo, hi, dtype=torch.int64)
        totals = (torch.arange(2).view(2, 1, 1, 1) * 1000000 + torch.arange(2).view(1, 2, 1, 1) * 10000
                  + w.view(1, 1, -1, 1) * 10 + torch.arange(8).view(1, 1, 1, 8))
        return totals, totals.unsqueeze(0).repeat(3, 1, 1, 1, 1), torch.tensor([len(calls) - 1], dtype=torch.int64)

    totals, per_user, flags = tune.sweep(40, 2, 2, stub)
    assert calls == [(0, 32), (32, 40)] and flags.tolist() == [0, 1]
    assert tuple(totals.shape) == (2, 2, 40, 8) and tuple(per_user.shape) == (3, 2, 2, 40, 8)
    for a in range(2):
        for b in range(2):
            for w in range(40):
                assert totals[a, b, w].tolist() == [a * 1000000 + b * 10000 + w * 10 + k for k in range(8)]
    assert torch.equal(per_user[2], totals)
    # one call: nothing to stitch, no per-user lines
    calls.clear()
    one = tune.sweep(3, 2, 2, lambda lo, hi: stub(lo, hi)[:1] + (None, torch.zeros(1, dtype=torch.int64)))
    assert calls == [(0, 3)] and one[1] is None and tuple(one[0].shape) == (2, 2, 3, 8)


def test_arguments_are_checked_before_anything_is_uploaded():
    ratings, coo, qs, us = EC.random_case(1, 4, 10, 3, 2)
    w = [TC.DEFAULT]
    for bad in ([], [-1], [1, 2, 3, 4, 5], [1.5], [True]):
        with pytest.raises(ValueError, match="q_cuts"):
            tune.evaluate_grid(ratings, *coo, us, w, q_cuts=bad, device="none")
        with pytest.raises(ValueError, match="u_cuts"):
            tune.evaluate_grid(ratings, *coo, us, w, u_cuts=bad, device="none")
    for bad in ([], [0.6, 0.4, 60], [[0.6, 0.4]], [[0.6, 0.4, float("nan")]]):
        with pytest.raises(ValueError, match="weights"):
            tune.evaluate_grid(ratings, *coo, us, bad, device="none")
    with pytest.raises(ValueError, match="fraction"):
        tune.evaluate_grid(ratings, *coo, us, w, fraction=1.5, device="none")
    with pytest.raises(ValueError, match="sum_order"):
        tune.evaluate_grid(ratings, *coo, us, w, sum_order="tree", device="none")
    with pytest.raises(ValueError, match="truth"):
        tune.evaluate_grid(ratings, *coo, us, w, truth=ratings[:, :5], device="none")
