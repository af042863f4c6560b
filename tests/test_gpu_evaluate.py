"""Hold-out and leave-one-out evaluation on the device (qrlsh.holdout / evaluate / evaluate_cells,
Recommender.evaluate).  Expected values come from the numpy restatement of tests/evaluate_cases.py (the oracle's
weighted_average and sum orders, the library's host mixer), never from the code under test; every comparison is exact."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
import evaluate_cases as EC
import predict_cases as PC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib  # noqa: E402
from qrlsh.ops import _ptr, _stream  # noqa: E402

DEV = "cuda"
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def tensors(coo):
    return tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo)


def assert_evaluation(ev, want, shape, cells, what):
    """ev: the device's Evaluation (with predictions); want: evaluate_ref's (pred, per_user, totals)"""
    pred, per, totals = want
    got_pred = host(ev.predictions)
    want_pred = EC.pred_matrix(shape, cells, pred)
    bad = np.argwhere(got_pred != want_pred)
    assert len(bad) == 0, "%s: %d cells of pred_out differ, first %s: %s != %s" % (
        what, len(bad), bad[0].tolist(), got_pred[tuple(bad[0])], want_pred[tuple(bad[0])])
    got_per = host(ev.per_user)
    assert got_per.shape == per.shape and got_per.dtype == np.int64
    bad = np.argwhere(got_per != per)
    assert len(bad) == 0, "%s: per_user differs at (user, word) %s" % (what, bad[:5].tolist())
    assert np.array_equal(ev.totals, totals), "%s: totals %s != %s" % (what, ev.totals.tolist(), totals.tolist())


def check_against_restatement(ratings, truth, coo, qs, us, what, seed=0, fraction=1.0, orders=ORDERS):
    """evaluate() on the device against evaluate_ref over the cells the sample rule keeps; -> the evaluated count"""
    truth_ = ratings if truth is None else truth
    cells, values = EC.evaluated_cells(truth_, seed, EC.keep_of(fraction))
    for o, s in orders.items():
        want = EC.evaluate_ref(ratings, qs, us, cells, values, summation=s)
        ev = qrlsh.evaluate(ratings, *tensors(coo), us, truth=truth, fraction=fraction, seed=seed, sum_order=o,
                            want_predictions=True, device=DEV)
        assert_evaluation(ev, want, ratings.shape, cells, "%s %s" % (what, o))
        assert ev.n == len(cells) and ev.covered == int((want[0] != 0).sum())
    return len(cells)


# ----------------------------------------------------------------------------------------------------- 1. knife edges
class Knife:
    """The serving tests' knife case.  truth = its matrix plus seeded values in 1..100 at the knife cells (unrated in
    `ratings`: a hold-out), ratings = its matrix (every rated cell: leave-one-out).  The oracle gets a seeded sample of
    4000 rated cells plus all knife cells."""

    def __init__(self):
        c = self.c = PC.build_case(16, nu=333, nq=5003, tu=10, tq=100, user_longest=32)
        rng = np.random.default_rng(160)
        self.coo = c.coo()
        self.truth = c.ratings.copy()
        self.truth[c.knife[:, 0], c.knife[:, 1]] = rng.integers(1, 101, size=len(c.knife))
        rated = np.argwhere(c.ratings != 0)
        pick = rated[np.sort(rng.choice(len(rated), size=4000, replace=False))]
        cells = np.concatenate([pick, c.knife])
        self.cells = cells[np.lexsort((cells[:, 1], cells[:, 0]))]          # row-major, as the sweep's
        self.values = self.truth[self.cells[:, 0], self.cells[:, 1]]
        self.sample_truth = np.zeros_like(self.truth)
        self.sample_truth[self.cells[:, 0], self.cells[:, 1]] = self.values
        self.want = {o: EC.evaluate_ref(c.ratings, c.qs, c.us, self.cells, self.values, summation=s)
                     for o, s in ORDERS.items()}


@pytest.fixture(scope="module")
def knife():
    return Knife()


def test_knife_cells_and_rated_cells_in_both_orders(knife):
    c = knife.c
    sq = {o: int(knife.want[o][2][[3, 7, 11]].sum()) for o in ORDERS}
    print("sum err^2 of the sample per order:", sq, "knife cells:", len(c.knife))
    assert sq["pairwise"] != sq["sequential"]          # the restatement alone: a wrong order shows
    assert len(c.knife) > 500 and all(knife.want[o][2][w] > 0 for o in ORDERS for w in (0, 4, 8))
    rt, tt = torch.from_numpy(c.ratings).to(DEV), torch.from_numpy(knife.truth).to(DEV)
    rated = int((knife.truth != 0).sum())
    for o in ORDERS:
        # the sample alone: every word of every line
        ev = qrlsh.evaluate(rt, *knife.coo, c.us, truth=knife.sample_truth, sum_order=o, want_predictions=True, device=DEV)
        assert_evaluation(ev, knife.want[o], c.ratings.shape, knife.cells, "sample " + o)
        # every rated cell and every knife cell in one call
        ev = qrlsh.evaluate(rt, *knife.coo, c.us, truth=tt, sum_order=o, want_predictions=True, device=DEV)
        pred = host(ev.predictions)
        assert np.array_equal(pred == -1, knife.truth == 0)
        assert np.array_equal(pred[knife.cells[:, 0], knife.cells[:, 1]], knife.want[o][0])
        per = host(ev.per_user)
        assert np.array_equal(EC.branch_sums(per), EC.sums_from_predictions(pred, knife.truth))
        assert np.array_equal(ev.totals, per.sum(axis=0)) and not per[:, 14:].any()
        assert ev.n == rated and ev.n == ev.totals[13] and 0 < ev.covered <= ev.n
        t = [int(x) for x in ev.totals]
        assert ev.rmse == math.sqrt((t[3] + t[7] + t[11]) / ev.covered) and ev.mae == (t[2] + t[6] + t[10]) / ev.covered
        # without pred_out, and with truth left out where truth is the matrix itself
        again = qrlsh.evaluate(tt, *knife.coo, c.us, sum_order=o, device=DEV)
        same = qrlsh.evaluate(tt, *knife.coo, c.us, truth=tt, sum_order=o, device=DEV)
        assert again.predictions is None and np.array_equal(again.totals, same.totals)
        assert np.array_equal(host(again.per_user), host(same.per_user))


# ----------------------------------------------------------------------------------------------------- 2. forms
@pytest.mark.parametrize("nq", [131072, 131073])
def test_forms_on_both_sides_of_the_lds_row_limit(nq):
    """nq = 131072 is the longest row the LDS holds, 131073 takes the global form; about 2000 cells are evaluated"""
    ratings, coo, qs, us = EC.random_case(nq, 8, nq, 12, 6)
    n = check_against_restatement(ratings, None, coo, qs, us, "nq=%d" % nq, seed=nq, fraction=2000 / (4 * nq))
    assert 1500 < n < 2500


def test_a_wide_value_beside_rows_that_stage_in_lds():
    ratings, coo, qs, us = EC.random_case(25, 6, 2500, 12, 4)
    ratings[2, 17] = 300
    ratings[4, 2499] = -3
    n = check_against_restatement(ratings, None, coo, qs, us, "wide", seed=1, fraction=0.3)
    assert 1500 < n < 3500


def test_the_queue_drains_inside_the_loop():
    """4096 users -> one slice of 2500 columns per user, so a workgroup queues a whole row of truth.  Rows with exactly
    1, 1023, 1024, 1025, 2047 and 2048 rated cells stand on both sides of one drain inside the loop (1024 waiting) and
    of the ring's wrap (2048 slots); one row is 90 % rated (two drains inside the loop and the rest after it).  They sit
    at the first user, in the middle and at the last user; every other workgroup evaluates nothing."""
    nu, nq = 4096, 2500
    ratings, coo, qs, us = EC.random_case(71, nu, nq, 10, 5, fill=0.3)
    rng = np.random.default_rng(72)
    truth = np.zeros_like(ratings)
    rows = [0, 513, 1777, 2048, 3000, nu - 1]
    EC.rows_with_exact_counts(truth, rows, [1024, 1, 2047, 1023, 1025, 2048], seed=73)
    dense = 1024
    truth[dense] = (rng.integers(1, 101, size=nq) * (rng.random(nq) < 0.9)).astype(np.int32)
    counts = {r: int((truth[r] != 0).sum()) for r in rows + [dense]}
    assert sorted(counts[r] for r in rows) == list(EC.QUEUE_EDGES) and counts[0] == 1024 and counts[nu - 1] == 2048
    assert counts[dense] > 2048 and int((truth != 0).sum()) == sum(counts.values())
    n = check_against_restatement(ratings, truth, coo, qs, us, "drain in the loop")
    assert n == sum(counts.values())


@pytest.mark.parametrize("nq", [1, 1025])
def test_one_column_and_a_partly_filled_last_slice(nq):
    ratings, coo, qs, us = EC.random_case(nq + 40, 5, nq, 6, 3, fill=0.6)
    ratings[3] = 0                       # a user with no rated cell
    ratings[1] = 0                       # and one with exactly one
    ratings[1, nq - 1] = 77
    n = check_against_restatement(ratings, None, coo, qs, us, "nq=%d" % nq, seed=2)
    assert n == int((ratings != 0).sum()) and n > 0


def test_no_user_lists_full_lists_and_empty_query_lists():
    nu, nq = 70, 1500
    ratings, coo, qs, _ = EC.random_case(31, nu, nq, 12, 0)
    assert any(j not in qs for j in range(nq))                      # queries with empty lists
    check_against_restatement(ratings, None, coo, qs, {}, "ku=0", seed=3, fraction=0.04)
    # lists of 64 on both sides
    _, _, _, us = EC.random_case(33, nu, nq, 12, 64)
    rng = np.random.default_rng(34)
    qs[7] = {"indexes": rng.choice(nq, size=64, replace=False).astype(np.int64),
             "values": np.sort(rng.integers(1, 1001, size=64))[::-1] / 1000.0}
    check_against_restatement(ratings, None, EC.coo_of(qs), qs, us, "ku=64", seed=4, fraction=0.04)
    cells = np.stack([np.arange(nu), np.full(nu, 7)], axis=1)
    want = EC.evaluate_ref(ratings, qs, us, cells, np.full(nu, 50))
    ev = qrlsh.evaluate_cells(ratings, *tensors(EC.coo_of(qs)), us, cells[:, 0], cells[:, 1], np.full(nu, 50),
                              want_predictions=True, device=DEV)
    assert np.array_equal(host(ev.predictions), want[0]) and np.array_equal(ev.totals, want[2])


# ----------------------------------------------------------------------------------------------------- 3. sampling
@pytest.fixture(scope="module")
def middle():
    """60 x 1203 (two slices, the second partly filled; 1203 % 4 != 0)"""
    return EC.random_case(77, 60, 1203, 10, 5)


def test_keep_nothing_and_keep_everything(middle):
    ratings, coo, qs, us = middle
    ev = qrlsh.evaluate(ratings, *tensors(coo), us, fraction=0.0, want_predictions=True, device=DEV)
    assert ev.n == 0 and not ev.totals.any() and not host(ev.per_user).any() and (host(ev.predictions) == -1).all()
    assert np.isnan(ev.rmse) and np.isnan(ev.coverage)
    ev = qrlsh.evaluate(ratings, *tensors(coo), us, fraction=1.0, want_predictions=True, device=DEV)
    assert ev.n == int((ratings != 0).sum()) and np.array_equal(host(ev.predictions) >= 0, ratings != 0)
    # any seed keeps everything at fraction 1
    other = qrlsh.evaluate(ratings, *tensors(coo), us, fraction=1.0, seed=99, device=DEV)
    assert np.array_equal(other.totals, ev.totals)


def test_holdout_zeroes_exactly_the_cells_the_evaluation_then_reports(middle):
    ratings, coo, qs, us = middle
    seed, fraction = 1234567890123, 0.3
    rt = torch.from_numpy(ratings).to(DEV)
    train, count = qrlsh.holdout(rt, fraction, seed=seed, device=DEV)
    want_train, want_count = EC.holdout_ref(ratings, seed, EC.keep_of(fraction))
    assert train.dtype == torch.int32 and train.data_ptr() != rt.data_ptr()
    assert np.array_equal(host(train), want_train) and count == want_count and 0 < count < (ratings != 0).sum()
    assert np.array_equal(host(rt), ratings)                            # the input is unchanged
    # host data in, same result; fraction 0 copies, fraction 1 empties
    again, n2 = qrlsh.holdout(ratings, fraction, seed=seed, device=DEV)
    assert n2 == count and torch.equal(again, train)
    assert torch.equal(qrlsh.holdout(rt, 0.0, device=DEV)[0], rt)
    gone, n3 = qrlsh.holdout(rt, 1.0, device=DEV)
    assert n3 == int((ratings != 0).sum()) and not host(gone).any()
    # the hold-out: the cells zeroed are exactly the cells evaluated
    for o, s in ORDERS.items():
        ev = qrlsh.evaluate(train, *tensors(coo), us, truth=rt, fraction=fraction, seed=seed, sum_order=o,
                            want_predictions=True, device=DEV)
        zeroed = (want_train == 0) & (ratings != 0)
        assert np.array_equal(host(ev.predictions) >= 0, zeroed) and ev.n == count
        cells, values = EC.evaluated_cells(ratings, seed, EC.keep_of(fraction))
        assert_evaluation(ev, EC.evaluate_ref(want_train, qs, us, cells, values, summation=s), ratings.shape, cells,
                          "hold-out " + o)


def test_holdout_where_a_thread_takes_several_vectors():
    """70 x 131 073 = 2.3 M vectors of four cells for the 1 M threads of the largest grid: threads take two or three,
    stepping (row, column) from one to the next across row ends (131 073 % 4 != 0)"""
    rng = np.random.default_rng(70)
    ratings = (rng.integers(1, 101, size=(70, 131073)) * (rng.random((70, 131073)) < 0.25)).astype(np.int32)
    train, count = qrlsh.holdout(ratings, 0.4, seed=11, device=DEV)
    want, n = EC.holdout_ref(ratings, 11, EC.keep_of(0.4))
    assert count == n and np.array_equal(host(train), want)


def test_holdout_through_pointers_that_are_not_16_byte_aligned(middle):
    ratings = middle[0]
    nu, nq = ratings.shape
    lib = _lib.load()
    big_in = torch.zeros((nu * nq + 8,), dtype=torch.int32, device=DEV)
    big_out = torch.full((nu * nq + 8,), -7, dtype=torch.int32, device=DEV)
    big_in[1:1 + nu * nq] = torch.from_numpy(ratings).to(DEV).reshape(-1)
    count = torch.zeros((1,), dtype=torch.int64, device=DEV)
    seed, keep = 5, EC.keep_of(0.5)
    _lib.check(lib.qrlsh_ratings_holdout(_ptr(big_in[1:]), nu, nq, seed, keep, _ptr(big_out[3:]), _ptr(count), _stream()))
    want, n = EC.holdout_ref(ratings, seed, keep)
    out = host(big_out)
    assert np.array_equal(out[3:3 + nu * nq].reshape(nu, nq), want) and int(count.item()) == n
    assert (out[:3] == -7).all() and (out[3 + nu * nq:] == -7).all()


# ----------------------------------------------------------------------------------------------------- 4. cells form
def test_cells_form_equals_the_sweep_and_the_restatement(middle):
    ratings, coo, qs, us = middle
    nu, nq = ratings.shape
    rng = np.random.default_rng(41)
    users, queries = rng.integers(0, nu, size=1000), rng.integers(0, nq, size=1000)
    users[900:], queries[900:] = users[:100], queries[:100]           # repeats
    values = rng.integers(1, 101, size=1000)
    values[900:] = values[:100]
    unrated = int((ratings[users, queries] == 0).sum())
    assert 300 < unrated < 700
    truth = ratings.copy()
    truth[users, queries] = values
    for o, s in ORDERS.items():
        sweep = qrlsh.evaluate(ratings, *tensors(coo), us, truth=truth, sum_order=o, want_predictions=True, device=DEV)
        ev = qrlsh.evaluate_cells(ratings, *tensors(coo), us, users, queries, values, sum_order=o,
                                  want_predictions=True, device=DEV)
        pred = host(ev.predictions)
        assert np.array_equal(pred, host(sweep.predictions)[users, queries]), o
        want = EC.evaluate_ref(ratings, qs, us, np.stack([users, queries], axis=1), values, summation=s)
        assert np.array_equal(pred, want[0]) and np.array_equal(ev.totals, want[2]), o
        assert ev.n == 1000 and ev.per_user is None
        # device tensors in, the same answer
        dev = qrlsh.evaluate_cells(torch.from_numpy(ratings).to(DEV), *tensors(coo), us, torch.from_numpy(users).to(DEV),
                                   torch.from_numpy(queries).to(DEV), torch.from_numpy(values).to(DEV), sum_order=o,
                                   device=DEV)
        assert np.array_equal(dev.totals, ev.totals) and dev.predictions is None
    none = qrlsh.evaluate_cells(ratings, *tensors(coo), us, [], [], [], device=DEV)
    assert none.n == 0 and not none.totals.any()


# ----------------------------------------------------------------------------------------------------- 5. flags
def test_flagged_inputs_raise_and_leave_no_fault(middle):
    ratings, coo, qs, us = middle
    nu, nq = ratings.shape
    rt = torch.from_numpy(ratings).to(DEV)
    src, dst, mil = tensors(coo)
    keep = src != 600
    long_ = tuple(torch.cat([t[keep], extra]) for t, extra in (
        (src, torch.full((65,), 600, dtype=torch.int32)), (dst, torch.arange(65, dtype=torch.int32)),
        (mil, torch.full((65,), 500, dtype=torch.int32))))
    order = torch.argsort(long_[0].to(torch.int64), stable=True)
    long_ = tuple(t[order] for t in long_)
    outside = dst.clone()
    outside[len(outside) // 2] = nq
    cu, cq, cv = (torch.tensor(x, device=DEV) for x in ([3, 5], [7, 9], [50, 60]))
    for call in (lambda *a: qrlsh.evaluate(rt, *a, us, device=DEV),
                 lambda *a: qrlsh.evaluate_cells(rt, *a, us, cu, cq, cv, device=DEV)):
        with pytest.raises(ValueError, match="more than 64"):
            call(*long_)
        with pytest.raises(ValueError, match="neighbour index"):
            call(src, outside, mil)
    with pytest.raises(ValueError, match="user id"):
        qrlsh.evaluate_cells(rt, src, dst, mil, us, torch.tensor([3, nu], device=DEV), cq, cv, device=DEV)
    with pytest.raises(ValueError, match="query id"):
        qrlsh.evaluate_cells(rt, src, dst, mil, us, cu, torch.tensor([-1, 9], device=DEV), cv, device=DEV)
    torch.cuda.synchronize()
    check_against_restatement(ratings, None, coo, qs, us, "after the flagged calls", seed=8, fraction=0.02,
                              orders={"pairwise": O.np_sum_order})


# ----------------------------------------------------------------------------------------------------- 6. Recommender
def _index_lists(ui):
    idx, milli, n = (host(t) for t in (ui.idx, ui.milli, ui.len))
    return {u: {"indexes": idx[u, :n[u]].astype(np.int64), "values": milli[u, :n[u]] / 1000.0} for u in range(ui.nu)}


def test_recommender_evaluates_the_model_it_serves():
    from test_gpu_recommend import _recommender_on
    from qrlsh import users
    from qrlsh.userlists import UserLists
    rec, g = _recommender_on("cfg1")
    nu, nq = rec.ratings.shape
    rec.compute_querySimilarities()
    labels = users.cluster_labels(rec.ratings)
    rec.live_user_similarities(labels=labels)
    ui = rec.user_index

    def raises():
        raise AssertionError("compute_userSimilarities ran: the user index did not serve")
    rec.compute_userSimilarities = raises
    summation = ORDERS[rec.sum_order]

    def leave_one_out(what):
        qs, us = rec.current_query_similarities(), _index_lists(ui)
        cells, values = EC.evaluated_cells(rec.ratings, 0, EC.ALL)
        want = EC.evaluate_ref(rec.ratings, qs, us, cells, values, summation=summation)
        ev = rec.evaluate()
        assert np.array_equal(ev.totals, want[2]) and np.array_equal(host(ev.per_user), want[1]), what
        assert ev.n == len(cells) > 2000 and 0 < ev.covered and ev.rmse > 0
        return qs

    leave_one_out("after the run")
    rng = np.random.default_rng(7)
    us_, qs_, vs_ = rng.integers(0, nu, size=40), rng.integers(0, nq, size=40), rng.integers(0, 101, size=40)
    rec.rate(us_, qs_, vs_)
    qs = leave_one_out("after rate")
    # a sample, the other order, an explicit test set
    cells, values = EC.evaluated_cells(rec.ratings, 5, EC.keep_of(0.25))
    want = EC.evaluate_ref(rec.ratings, qs, _index_lists(ui), cells, values, summation=O.np_sum_order)
    assert np.array_equal(rec.evaluate(fraction=0.25, seed=5, sum_order="pairwise").totals, want[2])
    got = rec.evaluate(cells=(cells[:, 0], cells[:, 1], values), sum_order="pairwise")
    assert np.array_equal(got.totals, want[2])
    # hold-out: the user side is rebuilt over the train matrix, nothing of the served state moves
    before = rec.ratings.copy()
    held = [t.clone() for t in (ui.ratings, ui.idx, ui.milli, ui.len)]
    ev = rec.evaluate(holdout=True, fraction=0.2, seed=3)
    train, count = EC.holdout_ref(before, 3, EC.keep_of(0.2))
    fresh = UserLists.build(train, ui.user_labels(), K=ui.K, device=DEV)
    cells, values = EC.evaluated_cells(before, 3, EC.keep_of(0.2))
    want = EC.evaluate_ref(train, qs, _index_lists(fresh), cells, values, summation=summation)
    assert np.array_equal(ev.totals, want[2]) and np.array_equal(host(ev.per_user), want[1])
    assert ev.n == count > 300
    assert np.array_equal(rec.ratings, before) and rec.user_index is ui
    assert all(torch.equal(a, b) for a, b in zip(held, (ui.ratings, ui.idx, ui.milli, ui.len)))
    # without a user index: the compute_userSimilarities route over the train matrix
    del rec.compute_userSimilarities
    del rec.user_index
    usim = rec._user_similarities_over(train)
    want = EC.evaluate_ref(train, qs, usim, cells, values, summation=summation)
    assert np.array_equal(rec.evaluate(holdout=True, fraction=0.2, seed=3).totals, want[2])
