"""Serving chosen users on the device (qrlsh.predict_users / qrlsh.for_users / Recommender.recommend_users).
Expected values come from the oracle (predict_cells in numpy's or the sequential sum order, then the restatement of
tests/test_recommend_users_host.py) or from the two-step device path that existed before (fill_predictions + top_k),
never from the code under test."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import predict_cases as PC
from test_recommend_host import restate
from test_recommend_users_host import oracle_rows, restate_users

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import predict  # noqa: E402

DEV = "cuda"
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}
USERS = [0, 3, 9, 200, 332, 3]


def host(*ts):
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def assert_same(got, want, what=""):
    for name, g, w in zip(("idx", "val", "avail"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s %s shape %s != %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            raise AssertionError("%s %s differs at %s" % (what, name, np.argwhere(g != w)[:5].tolist()))


# ----------------------------------------------------------------------------------------------------- 1. knife case
class Knife:
    def __init__(self):
        c = self.c = PC.build_case(16, nu=333, nq=5003, tu=10, tq=100, user_longest=32)
        self.coo = c.coo()
        self.rows = {o: oracle_rows(c.ratings, c.qs, c.us, USERS, summation=s) for o, s in ORDERS.items()}


@pytest.fixture(scope="module")
def knife():
    return Knife()


def test_knife_rows_equal_the_oracle_in_both_orders(knife):
    c = knife.c
    differ = (knife.rows["pairwise"] != knife.rows["sequential"]).sum(axis=1)
    print("cells that differ between the orders, per requested row:", differ.tolist())
    assert differ.sum() > 0
    for o in ORDERS:
        got = host(qrlsh.predict_users(c.ratings, *knife.coo, c.us, USERS, device=DEV, sum_order=o))
        bad = np.argwhere(got != knife.rows[o])
        assert len(bad) == 0, "%s: %d cells differ, first (request, column) %s" % (o, len(bad), bad[0].tolist())
    # a device ratings tensor, prepared user lists and device ids give the same rows
    rt = torch.from_numpy(c.ratings).to(DEV)
    prepared = predict.user_lists(c.us, c.nu, DEV)
    got = host(qrlsh.predict_users(rt, *knife.coo, prepared, torch.tensor(USERS, device=DEV), device=DEV))
    assert np.array_equal(got, knife.rows["pairwise"])
    # users = None: every row, in order
    every = host(qrlsh.predict_users(rt, *knife.coo, prepared, None, device=DEV))
    assert every.shape == (c.nu, c.nq) and np.array_equal(every[USERS], knife.rows["pairwise"])


def test_knife_top_k_equals_the_restated_oracle_rows(knife):
    c = knife.c
    tops = {}
    for o in ORDERS:
        for k in (5, 28, 1024):
            want = restate_users(c.ratings, knife.rows[o], USERS, k)
            got = host(*qrlsh.for_users(c.ratings, *knife.coo, c.us, USERS, k, sum_order=o, device=DEV))
            assert_same(got, want, "%s k=%d" % (o, k))
            tops[o, k] = want
    # the orders already part at k = 5, and in every row cells tie with the 28th value across the cut: a wrong order
    # or tie rule shows
    assert any(not np.array_equal(tops["pairwise", 5][n], tops["sequential", 5][n]) for n in (0, 1))
    _, val, _ = tops["pairwise", 28]
    for x, u in enumerate(USERS):
        row = knife.rows["pairwise"][x]
        tied = int(((c.ratings[u] == 0) & (row == val[x, 27])).sum())
        assert tied > int((val[x] == val[x, 27]).sum()), (u, tied)


# ----------------------------------------------------------------------------------------------------- 2. two-step path
def test_two_step_path_agrees_for_every_slicing_and_window(knife):
    c = knife.c
    rt = torch.from_numpy(c.ratings).to(DEV)
    prepared = predict.user_lists(c.us, c.nu, DEV)
    for o in ORDERS:
        full = predict.fill_predictions(rt, *knife.coo, c.us, device=DEV, sum_order=o)
        assert np.array_equal(host(full)[USERS], knife.rows[o])
        for k in (5, 28):
            want = host(*qrlsh.top_k(rt, full, k, users=USERS, device=DEV))
            assert_same(want, restate_users(c.ratings, knife.rows[o], USERS, k), "two-step %s k=%d" % (o, k))
            for slices in (0, 1, 3, 256):
                for lo in (0, 70, -5000):
                    got = host(*qrlsh.for_users(rt, *knife.coo, prepared, USERS, k, lo=lo, slices=slices, sum_order=o,
                                                device=DEV))
                    assert_same(got, want, "%s k=%d slices=%d lo=%d" % (o, k, slices, lo))


# ----------------------------------------------------------------------------------------------------- 3. forms
def _random_case(seed, nu, nq, longest_q, ku, fill=0.5):
    """random ratings 1..100, query lists of 0..longest_q distinct neighbours, user lists of exactly ku"""
    rng = np.random.default_rng(seed)
    ratings = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < fill)).astype(np.int32)
    deg = rng.integers(0, longest_q + 1, size=nq)
    src = np.repeat(np.arange(nq), deg)
    dst = rng.integers(0, nq, size=len(src))
    mil = rng.integers(0, 1001, size=len(src))
    us = {}
    for u in range(nu):
        if ku:
            us[u] = {"indexes": rng.choice(nu, size=ku, replace=False).astype(np.int64),
                     "values": np.round(rng.random(ku), 3)}
    coo = tuple(torch.tensor(x, dtype=torch.int32) for x in (src, dst, mil))
    return ratings, coo, us


def _rows_match_fill_predictions(ratings, coo, us, users, what):
    rt = torch.from_numpy(ratings).to(DEV)
    for o in ORDERS:
        full = predict.fill_predictions(rt, *coo, us, device=DEV, sum_order=o)
        got = qrlsh.predict_users(rt, *coo, us, users, device=DEV, sum_order=o)
        torch.cuda.synchronize()
        assert torch.equal(got, full[torch.tensor(users, device=DEV)]), "%s %s" % (what, o)
        idx, val, avail = host(*qrlsh.for_users(rt, *coo, us, users, 28, sum_order=o, device=DEV))
        assert_same((idx, val, avail), host(*qrlsh.top_k(rt, full, 28, users=users, device=DEV)), "%s %s" % (what, o))


@pytest.mark.parametrize("nq", [131072, 131073])
def test_forms_on_both_sides_of_the_lds_row_limit(nq):
    """nq = 131072 is the longest row the LDS holds, 131073 takes the global form; in each, user 5 holds a 256 and
    user 11 a -1 (at 131072: the fallback inside the workgroup), user 20 is an ordinary row"""
    ratings, coo, us = _random_case(nq, 40, nq, 12, 6)
    ratings[5, nq // 3] = 256
    ratings[11, nq - 2] = -1
    _rows_match_fill_predictions(ratings, coo, us, [5, 11, 20], "nq=%d" % nq)


def test_no_user_lists_full_user_lists_and_a_query_list_of_64():
    nu, nq = 80, 3001
    ratings, coo, _ = _random_case(31, nu, nq, 12, 0)
    # query 7 gets a list of exactly 64
    src, dst, mil = (t.numpy() for t in coo)
    keep = src != 7
    rng = np.random.default_rng(32)
    src = np.concatenate([src[keep], np.full(64, 7)])
    dst = np.concatenate([dst[keep], rng.choice(nq, size=64, replace=False)])
    mil = np.concatenate([mil[keep], np.sort(rng.integers(1, 1001, size=64))[::-1]])
    o = np.argsort(src, kind="stable")
    coo = tuple(torch.tensor(x[o], dtype=torch.int32) for x in (src, dst, mil))
    ratings[:, 7] = 0
    _rows_match_fill_predictions(ratings, coo, {}, [0, 79, 40], "ku=0")
    _, _, us = _random_case(33, nu, nq, 12, 64)
    _rows_match_fill_predictions(ratings, coo, us, [0, 79, 40], "ku=64")
    # and against the oracle on the column whose list is full
    qs = {7: {"indexes": dst[o][src[o] == 7].astype(np.int64), "values": mil[o][src[o] == 7] / 1000.0}}
    cells = np.stack([np.arange(nu), np.full(nu, 7)], axis=1)
    for order, s in ORDERS.items():
        want = O.predict_cells(ratings, qs, us, cells, summation=s)
        got = host(qrlsh.predict_users(ratings, *coo, us, None, device=DEV, sum_order=order))[:, 7]
        assert np.array_equal(got, want), order


# ----------------------------------------------------------------------------------------------------- 4. rows form
@pytest.mark.parametrize("nq", [2048, 2049])
def test_selection_rows_form_and_its_neighbour(nq):
    """nq = 2048 is the last size of the selection's one-workgroup-per-row form; user 2 has every query rated
    (avail 0), user 4 three unrated ones (k > avail)"""
    ratings, coo, us = _random_case(nq, 12, nq, 12, 5)
    ratings[2] = np.where(ratings[2] == 0, 7, ratings[2])
    ratings[4] = np.where(ratings[4] == 0, 9, ratings[4])
    ratings[4, [1, nq // 2, nq - 1]] = 0
    users = [4, 2, 0, 11]
    rt = torch.from_numpy(ratings).to(DEV)
    full = predict.fill_predictions(rt, *coo, us, device=DEV)
    for k in (1, 28, 1024):
        want = restate(ratings, host(full), k, users=users)
        got = host(*qrlsh.for_users(rt, *coo, us, users, k, device=DEV))
        assert_same(got, want, "nq=%d k=%d" % (nq, k))
        assert got[2][1] == 0 and got[2][0] <= 3 and np.all(got[0][1] == -1)


def test_no_queries_at_all():
    ratings = np.zeros((4, 0), dtype=np.int32)
    empty = tuple(torch.zeros((0,), dtype=torch.int32) for _ in range(3))
    us = {0: {"indexes": np.array([1]), "values": np.array([0.5])}}
    idx, val, avail = host(*qrlsh.for_users(ratings, *empty, us, [3, 0], 2, device=DEV))
    assert idx.shape == (2, 2) and np.all(idx == -1) and np.all(val == 0) and np.all(avail == 0)
    assert host(qrlsh.predict_users(ratings, *empty, us, [3, 0], device=DEV)).shape == (2, 0)
    idx, val, avail = qrlsh.for_users(np.zeros((4, 9), dtype=np.int32), *empty, us, [], 2, device=DEV)
    assert idx.shape == (0, 2) and avail.shape == (0,)


# ----------------------------------------------------------------------------------------------------- 5. flags
def test_flagged_inputs_raise_and_leave_no_fault(knife):
    c = knife.c
    rt = torch.from_numpy(c.ratings).to(DEV)
    src, dst, mil = (t.clone() for t in knife.coo)
    # a 65-entry list for query 4000 (its own entries replaced)
    keep = src != 4000
    long_ = tuple(torch.cat([t[keep], extra]) for t, extra in (
        (src, torch.full((65,), 4000, dtype=torch.int32)), (dst, torch.arange(65, dtype=torch.int32)),
        (mil, torch.full((65,), 500, dtype=torch.int32))))
    order = torch.argsort(long_[0].to(torch.int64), stable=True)
    long_ = tuple(t[order] for t in long_)
    # an index = nq
    outside = dst.clone()
    outside[len(outside) // 2] = c.nq
    for call in (lambda *a: qrlsh.predict_users(rt, *a, device=DEV),
                 lambda *a: qrlsh.for_users(rt, *a, 5, device=DEV)):
        with pytest.raises(ValueError, match="more than 64"):
            call(*long_, c.us, USERS)
        with pytest.raises(ValueError, match="neighbour index"):
            call(src, outside, mil, c.us, USERS)
        with pytest.raises(ValueError, match="user id"):
            call(src, dst, mil, c.us, torch.tensor([3, c.nu], device=DEV))
        with pytest.raises(ValueError, match="user id"):
            call(src, dst, mil, c.us, torch.tensor([-1], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    got = host(qrlsh.predict_users(rt, *knife.coo, c.us, USERS, device=DEV))
    assert np.array_equal(got, knife.rows["pairwise"])
    assert_same(host(*qrlsh.for_users(rt, *knife.coo, c.us, USERS, 5, device=DEV)),
                restate_users(c.ratings, knife.rows["pairwise"], USERS, 5), "after the flagged calls")


# ----------------------------------------------------------------------------------------------------- 6. Recommender
def _same_answers(got, want):
    assert sorted(got) == sorted(want)
    for u in want:
        assert got[u]["available"] == want[u]["available"], u
        assert got[u]["indexes"].dtype == np.int64 and got[u]["values"].dtype == np.int64
        assert np.array_equal(got[u]["indexes"], want[u]["indexes"]), u
        assert np.array_equal(got[u]["values"], want[u]["values"]), u


@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_serves_chosen_users_in_every_state(sub):
    """recommend_users / predict_users against recommend(compute_scores(...)[1]) after the run, after
    add_queries(update_lists=True) and after remove_queries(update_lists=True); both sides of a state get the same
    user similarities (the clustering runs once per state)"""
    from test_gpu_recommend import _recommender_on
    from qrlsh import pipeline
    rec, g = _recommender_on(sub)
    N, nu = rec.queriesIDs.size, rec.usersIDs.size
    n0 = N - 9
    block = rec.ratings[:, n0:].copy()
    rest, ids = np.asarray(rec.queries, dtype=object)[n0:], rec.queriesIDs[n0:]
    rec.queries, rec.queriesIDs, rec.ratings = rec.queries[:n0], rec.queriesIDs[:n0], rec.ratings[:, :n0]
    rec.max_candidates = pipeline.max_candidates(N)
    np.random.seed(int(g["seed"]))
    users = [0, nu - 1, 7, 7, 3]
    with pytest.raises(ValueError, match="no live lists"):
        rec.recommend_users(users, 5)
    method = type(rec).compute_userSimilarities

    def scores(**kw):
        """(finalPredictions, user similarities) of the current state: compute_scores gets the similarities computed
        here, so the clustering runs once per state"""
        usim = method(rec)
        rec.compute_userSimilarities = lambda: usim
        return rec.compute_scores(**kw)[1], usim

    def check(final, usim, what):
        fin = final.to_numpy()
        for k in (1, 7, 1024):
            _same_answers(rec.recommend_users(users, k, user_sim=usim), rec.recommend(final, k, users))
        _same_answers(rec.recommend_users(None, 7, user_sim=usim), rec.recommend(final, 7))
        rt = torch.from_numpy(np.ascontiguousarray(rec.ratings, dtype=np.int32)).to(DEV)
        prepared = predict.user_lists(usim, nu, DEV)
        _same_answers(rec.recommend_users(torch.tensor(users, device=DEV), 7, user_sim=prepared, ratings=rt),
                      rec.recommend(final, 7, users))
        rows = rec.predict_users(users, user_sim=usim)
        assert np.array_equal(rows.to_numpy(), fin[users]), what
        assert list(rows.columns) == list(final.columns) and list(rows.index) == list(final.index[users])
        assert sum(e["available"] for e in rec.recommend(final, 7, users).values()) > 0, what

    check(*scores(), "after the run")
    rec.add_queries(rest, ratings=block, ids=ids, update_lists=True)
    assert rec.queriesIDs.size == N
    check(*scores(reuse_lists=True), "after add_queries")
    rec.remove_queries([0, N // 2, N - 1], update_lists=True)
    assert rec.queriesIDs.size == N - 3
    check(*scores(reuse_lists=True), "after remove_queries")
    # without an argument the user similarities are computed here
    del rec.compute_userSimilarities
    final = rec.compute_scores(reuse_lists=True)[1]
    _same_answers(rec.recommend_users(users, 7), rec.recommend(final, 7, users))


# ----------------------------------------------------------------------------------------------------- 7. row blocks
def test_row_blocks_match_the_single_call_and_name_a_bad_id_of_the_last_block(monkeypatch):
    """37 rows under a budget that admits 10 per call: 37 -> 19 -> 10, four library calls, the last of 7 rows"""
    from qrlsh import _lib, recommend
    lib = _lib.load()
    ratings, coo, us = _random_case(41, 37, 40, 12, 5)
    want = host(*qrlsh.for_users(ratings, *coo, us, None, 5, device=DEV))
    full = predict.fill_predictions(ratings, *coo, us, device=DEV)
    assert_same(want, restate(ratings, host(full), 5), "one call")
    calls = []
    real = lib.qrlsh_recommend_users

    def counted(*args):
        calls.append(args[14])
        return real(*args)
    monkeypatch.setattr(lib, "qrlsh_recommend_users", counted)
    monkeypatch.setattr(recommend, "WORKSPACE_BUDGET", int(lib.qrlsh_recommend_users_workspace_bytes(10, 40, 5, 0)))
    assert_same(host(*qrlsh.for_users(ratings, *coo, us, None, 5, device=DEV)), want, "row blocks")
    assert calls == [10, 10, 10, 7]
    users = list(range(36, -1, -1))
    got = host(*qrlsh.for_users(ratings, *coo, us, torch.tensor(users, device=DEV), 5, device=DEV))
    assert_same(got, tuple(w[users] for w in want), "row blocks, device ids")
    users[33] = 37                                        # the only bad id, in the block of the last 7
    with pytest.raises(ValueError, match=r"user id 37 \(position 33\) outside \[0, 37\)"):
        qrlsh.for_users(ratings, *coo, us, torch.tensor(users, device=DEV), 5, device=DEV)
    torch.cuda.synchronize()
