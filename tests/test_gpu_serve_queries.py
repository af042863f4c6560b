"""Serving chosen queries on the device (qrlsh.predict_queries / for_queries / query_utility, Recommender.recommend_queries
/ predict_queries / query_utility).  Expected values come from the restatements of tests/serve_queries_cases.py over the
oracle's matrix, or -- for the larger shapes -- from the route that existed before (fill_predictions, the strided
columns, top_k over the transposes), never from the code under test.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import serve_queries_cases as SQ

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import predict  # noqa: E402
from qrlsh import servequeries  # noqa: E402

DEV = "cuda"
ORDERS = SQ.ORDERS


def host(*ts):
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def assert_same(got, want, what=""):
    for name, g, w in zip(("users", "val", "avail"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s %s shape %s != %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            raise AssertionError("%s %s differs at %s" % (what, name, np.argwhere(g != w)[:5].tolist()))


def old_route(rt, coo, us, queries, k, order="pairwise", full=None):
    """what a caller had before: the whole matrix, the strided columns and their transposes, top_k over them.
    -> (columns (m, nu) device, (users, val, avail) host, the matrix)"""
    if full is None:
        full = predict.fill_predictions(rt, *coo, us, device=DEV, sum_order=order)
    q = torch.as_tensor(np.asarray(queries, dtype=np.int64), device=DEV)
    cols = full[:, q].T.contiguous()
    top = host(*qrlsh.top_k(rt[:, q].T.contiguous(), cols, k, device=DEV)) if len(queries) and rt.shape[0] else None
    return cols, top, full


def words_from(rt, cols):
    """words 0 .. 4 from the raw and the completed columns (m, nu) alone"""
    r, c = host(rt).astype(np.int64), host(cols).astype(np.int64)
    hit = (r == 0) & (c != 0)
    return np.stack([(r != 0).sum(1), r.sum(1), hit.sum(1), (c * hit).sum(1), ((r == 0) & (c == 0)).sum(1)], axis=1)


# ----------------------------------------------------------------------------------------------------- 1. knife case
@pytest.fixture(scope="module")
def knife():
    return SQ.knife_case()


def test_knife_columns_top_users_and_words_in_both_orders(knife):
    c, queries, finals = knife
    coo = c.coo()
    tops = {}
    for o, s in ORDERS.items():
        want = SQ.restate_columns(finals[o], queries)
        got = host(qrlsh.predict_queries(c.ratings, *coo, c.us, queries, device=DEV, sum_order=o))
        bad = np.argwhere(got != want)
        assert got.dtype == np.int32 and got.shape == want.shape
        assert len(bad) == 0, "%s: %d cells differ, first (request, user) %s" % (o, len(bad), bad[0].tolist())
        for k in (1, 5, 1024):
            tops[o, k] = SQ.restate_top_users(c.ratings, finals[o], queries, k)
            assert_same(host(*qrlsh.for_queries(c.ratings, *coo, c.us, queries, k, sum_order=o, device=DEV)), tops[o, k],
                        "%s k=%d" % (o, k))
        words = qrlsh.query_utility(c.ratings, *coo, c.us, queries, device=DEV, sum_order=o).words
        assert np.array_equal(words, SQ.restate_words(c.ratings, finals[o], c.qs, c.us, queries, s)), o
    assert any(not np.array_equal(a, b) for a, b in zip(tops["pairwise", 5], tops["sequential", 5]))
    # a device matrix, prepared user lists and device ids give the same
    rt = torch.from_numpy(c.ratings).to(DEV)
    prepared = predict.user_lists(c.us, c.nu, DEV)
    got = host(qrlsh.predict_queries(rt, *coo, prepared, torch.tensor(queries, device=DEV), device=DEV))
    assert np.array_equal(got, SQ.restate_columns(finals["pairwise"], queries))


def test_utility_of_every_column_and_beside_the_other_calls(knife):
    c, queries, finals = knife
    coo = c.coo()
    every = qrlsh.query_utility(c.ratings, *coo, c.us, device=DEV)
    want = SQ.restate_words(c.ratings, finals["pairwise"], c.qs, c.us, range(c.nq))
    assert every.words.shape == (c.nq, 8) and np.array_equal(every.words, want)
    assert np.array_equal(every.rated + every.predicted + every.missed, np.full(c.nq, c.nu))
    alone = qrlsh.query_utility(c.ratings, *coo, c.us, queries, device=DEV).words
    assert np.array_equal(alone, want[queries])
    cols, u1 = qrlsh.predict_queries(c.ratings, *coo, c.us, queries, device=DEV, utility=True)
    users, val, avail, u2 = qrlsh.for_queries(c.ratings, *coo, c.us, queries, 5, device=DEV, utility=True)
    assert np.array_equal(u1.words, alone) and np.array_equal(u2.words, alone)
    assert np.array_equal(host(cols), SQ.restate_columns(finals["pairwise"], queries))
    assert np.array_equal(host(avail), alone[:, 2])          # the eligible users are the predicted ones


# ----------------------------------------------------------------------------------------------------- 2. slice edges
@pytest.mark.parametrize("nu", [1, 1023, 1024, 1025, 2049])
def test_slice_edges_many_slices_one_slice_and_unsorted_ids(nu):
    c = SQ.random_case(nu, nu, 96, 12, 6)
    coo = c.torch_coo()
    rt = torch.from_numpy(c.ratings).to(DEV)
    prepared = predict.user_lists(c.us, c.nu, DEV)
    rng = np.random.default_rng(nu)
    distinct = rng.permutation(96)[:64]
    many = distinct[rng.integers(0, 64, size=4100)]        # 4100 > PU_AUTO_GROUPS requests: one slice per request
    full = None
    for o in ORDERS:
        for queries in ([41], many.tolist(), [95, 0, 41, 17, 41, 3]):
            cols, top, full = old_route(rt, coo, c.us, queries, 10, o, full)
            got = qrlsh.predict_queries(rt, *coo, prepared, queries, device=DEV, sum_order=o)
            assert torch.equal(got, cols), (o, len(queries))
            assert_same(host(*qrlsh.for_queries(rt, *coo, prepared, queries, 10, sum_order=o, device=DEV)), top,
                        "%s m=%d" % (o, len(queries)))
            words = qrlsh.query_utility(rt, *coo, prepared, queries, device=DEV, sum_order=o).words
            q = torch.as_tensor(queries, device=DEV)
            assert np.array_equal(words[:, :5], words_from(rt[:, q].T, cols)), (o, len(queries))
        full = None
    # unsorted ids as a device tensor
    queries = [95, 0, 41, 17, 41, 3]
    cols, top, _ = old_route(rt, coo, c.us, queries, 10)
    qt = torch.tensor(queries, dtype=torch.int64, device=DEV)
    assert torch.equal(qrlsh.predict_queries(rt, *coo, prepared, qt, device=DEV), cols)
    assert_same(host(*qrlsh.for_queries(rt, *coo, prepared, qt, 10, device=DEV)), top, "device ids")


# ----------------------------------------------------------------------------------------------------- 3. forms
@pytest.mark.parametrize("nu", [131072, 131073])
def test_forms_on_both_sides_of_the_lds_column_limit(nu):
    """nu = 131072 is the longest column the LDS holds, 131073 takes the memory form; column 5 holds a 256 (at 131072: the
    fallback inside the workgroup), the others are narrow"""
    c = SQ.random_case(nu, nu, 48, 12, 6)
    c.ratings[nu // 3, 5] = 256
    assert any(nu // 3 in c.us[u]["indexes"] for u in range(nu) if c.ratings[u, 5] == 0)
    coo = c.torch_coo()
    rt = torch.from_numpy(c.ratings).to(DEV)
    prepared = predict.user_lists(c.us, nu, DEV)
    queries = [5, 11, 47, 0]
    cols, top, _ = old_route(rt, coo, c.us, queries, 28)
    assert torch.equal(qrlsh.predict_queries(rt, *coo, prepared, queries, device=DEV), cols)
    users, val, avail, util = qrlsh.for_queries(rt, *coo, prepared, queries, 28, device=DEV, utility=True)
    assert_same(host(users, val, avail), top, "nu=%d" % nu)
    q = torch.as_tensor(queries, device=DEV)
    assert np.array_equal(util.words[:, :5], words_from(rt[:, q].T, cols))


def test_both_forms_in_one_launch():
    c, queries = SQ.mixed_forms_case()
    coo = c.torch_coo()
    rt = torch.from_numpy(c.ratings).to(DEV)
    prepared = predict.user_lists(c.us, c.nu, DEV)
    for o in ORDERS:
        cols, top, _ = old_route(rt, coo, c.us, queries, 28, o)
        got = qrlsh.predict_queries(rt, *coo, prepared, queries, device=DEV, sum_order=o)
        bad = torch.nonzero(got != cols)
        assert bad.numel() == 0, "%s: first (request, user) %s" % (o, bad[0].tolist())
        users, val, avail, util = qrlsh.for_queries(rt, *coo, prepared, queries, 28, sum_order=o, device=DEV, utility=True)
        assert_same(host(users, val, avail), top, o)
        q = torch.as_tensor(queries, device=DEV)
        assert np.array_equal(util.words[:, :5], words_from(rt[:, q].T, cols))
        assert avail[4].item() == 0 and util.words[4, 0] == c.nu        # the fully rated column
        assert util.words[3, 0] == 0 and util.words[3, 6] == util.words[3, 7] == 0   # the all-zero one has no user side
    # the small oracle: the wide columns cell by cell on a sample of users
    from oracle import oracle as O
    sample = [u for u in range(0, c.nu, 97)] + [1234, 17]
    for x, j in ((1, 3), (2, 5)):
        cells = np.stack([np.asarray(sample), np.full(len(sample), j)], axis=1)
        want = O.predict_cells(c.ratings, c.qs, c.us, cells)
        assert np.array_equal(host(got)[x][sample], want), j


# ----------------------------------------------------------------------------------------------------- 4. list edges
def test_list_edges():
    nu, nq = 80, 96
    c = SQ.random_case(31, nu, nq, 12, 0)
    src, dst, mil = c.coo
    absent = [j for j in range(nq) if j not in c.qs]
    assert absent, "every query has a list"
    rng = np.random.default_rng(32)
    # query 7 gets a list of exactly 64; query 9 names only the neighbours of its neighbours
    second = np.unique(np.concatenate([c.qs[int(b)]["indexes"] for b in c.qs[9]["indexes"] if int(b) in c.qs]))
    second = second[(second != 9) & ~np.isin(second, c.qs[9]["indexes"])][:40]
    assert len(c.qs[9]["indexes"]) > 0 and len(second) > 0
    keep = (src != 7) & (src != 9)
    src = np.concatenate([src[keep], np.full(64, 7), np.full(len(second), 9)])
    dst = np.concatenate([dst[keep], rng.choice(np.delete(np.arange(nq), 7), size=64, replace=False), second])
    mil = np.concatenate([mil[keep], np.sort(rng.integers(1, 1001, size=64))[::-1],
                          np.sort(rng.integers(1, 1001, size=len(second)))[::-1]])
    o = np.argsort(src, kind="stable")
    coo = tuple(torch.tensor(x[o], dtype=torch.int32) for x in (src, dst, mil))
    c.ratings[:, 7] = 0
    rt = torch.from_numpy(c.ratings).to(DEV)
    queries = [7, 9, absent[0], 0, 95]
    full64 = SQ.random_case(33, nu, nq, 12, 64).us
    assert all(len(v["indexes"]) == 64 for v in full64.values())
    for us, what in (({}, "ku=0"), (full64, "ku=64")):
        for order in ORDERS:
            cols, top, _ = old_route(rt, coo, us, queries, 10, order)
            assert torch.equal(qrlsh.predict_queries(rt, *coo, us, queries, device=DEV, sum_order=order), cols), what
            users, val, avail, util = qrlsh.for_queries(rt, *coo, us, queries, 10, sum_order=order, device=DEV, utility=True)
            assert_same(host(users, val, avail), top, what)
            # the absent query has no query side; without user lists nobody has a user side
            assert util.words[2, 5] == util.words[2, 7] == 0, what
            if not us:
                assert not util.words[:, 6:].any() and util.words[2, 2] == 0
            else:
                assert util.words[2, 6] > 0
    # and against the oracle on the column whose list is full
    from oracle import oracle as O
    qs = {7: {"indexes": dst[o][src[o] == 7].astype(np.int64), "values": mil[o][src[o] == 7] / 1000.0}}
    cells = np.stack([np.arange(nu), np.full(nu, 7)], axis=1)
    for order, s in ORDERS.items():
        want = O.predict_cells(c.ratings, qs, full64, cells, summation=s)
        got = host(qrlsh.predict_queries(rt, *coo, full64, [7], device=DEV, sum_order=order))[0]
        assert np.array_equal(got, want), order


# ----------------------------------------------------------------------------------------------------- 5. selection
@pytest.mark.parametrize("nu", [2048, 2049])
def test_selection_rows_form_and_its_neighbour(nu):
    """nu = 2048 is the last size of the selection's one-workgroup-per-row form.  Column 2 is fully rated (avail 0),
    column 4 has three unrated users (k > eligible); the users come in 8 kinds with identical rows and no user lists, so
    that a column holds at most 8 distinct predictions: the cut at k goes through equal values, ordered by user id"""
    rng = np.random.default_rng(nu)
    base = SQ.random_case(nu, 8, 64, 12, 0)
    kind = rng.integers(0, 8, size=nu)
    ratings = np.ascontiguousarray(base.ratings[kind])
    ratings[:, 2] = np.where(ratings[:, 2] == 0, 7, ratings[:, 2])
    ratings[:, 4] = np.where(ratings[:, 4] == 0, 9, ratings[:, 4])
    ratings[[1, nu // 2, nu - 1], 4] = 0
    coo = base.torch_coo()
    rt = torch.from_numpy(ratings).to(DEV)
    queries = [4, 2, 0, 63, 17]
    full = host(predict.fill_predictions(rt, *coo, {}, device=DEV))
    for k in (1, 28, 1024):
        want = SQ.restate_top_users(ratings, full, queries, k)
        for slices, lo in ((0, 0), (1, 0), (2, 0), (0, -5000), (2, 70), (1, 100000)):
            got = host(*qrlsh.for_queries(rt, *coo, {}, queries, k, lo=lo, slices=slices, device=DEV))
            assert_same(got, want, "nu=%d k=%d slices=%d lo=%d" % (nu, k, slices, lo))
        assert want[2][1] == 0 and want[2][0] <= 3 and np.all(want[0][1] == -1)
    users, val, avail = SQ.restate_top_users(ratings, full, queries, 28)
    x = 4                                                    # query 17: about half of the users are eligible
    assert avail[x] > 100
    j = queries[x]
    tied = int(((ratings[:, j] == 0) & (full[:, j] == val[x, 27])).sum())
    assert tied > int((val[x] == val[x, 27]).sum()), "no tie across the cut"
    assert (np.diff(users[x][val[x] == val[x, 27]]) > 0).all()


# ----------------------------------------------------------------------------------------------------- 6. empty shapes
def test_empty_shapes_every_column_and_blocks(monkeypatch):
    c = SQ.random_case(5, 40, 30, 8, 4)
    coo = c.torch_coo()
    rt = torch.from_numpy(c.ratings).to(DEV)
    # m = 0
    users, val, avail = qrlsh.for_queries(rt, *coo, c.us, [], 3, device=DEV)
    assert users.shape == (0, 3) and val.shape == (0, 3) and avail.shape == (0,)
    assert qrlsh.predict_queries(rt, *coo, c.us, [], device=DEV).shape == (0, 40)
    assert qrlsh.query_utility(rt, *coo, c.us, [], device=DEV).words.shape == (0, 8)
    # nu = 0
    none = np.zeros((0, 30), dtype=np.int32)
    users, val, avail = host(*qrlsh.for_queries(none, *coo, {}, [3, 0], 2, device=DEV))
    assert users.shape == (2, 2) and np.all(users == -1) and np.all(val == 0) and np.all(avail == 0)
    assert qrlsh.predict_queries(none, *coo, {}, [3, 0], device=DEV).shape == (2, 0)
    assert not qrlsh.query_utility(none, *coo, {}, None, device=DEV).words.any()
    # queries = None: every column in order; the same in blocks of a few requests
    cols, top, _ = old_route(rt, coo, c.us, list(range(30)), 5)
    assert torch.equal(qrlsh.predict_queries(rt, *coo, c.us, None, device=DEV), cols)
    assert_same(host(*qrlsh.for_queries(rt, *coo, c.us, None, 5, device=DEV)), top, "every column")
    whole = qrlsh.query_utility(rt, *coo, c.us, None, device=DEV).words
    monkeypatch.setattr(servequeries, "WORKSPACE_BUDGET", 7 * 40 * 4 + 7 * 40 * 4)
    assert torch.equal(qrlsh.predict_queries(rt, *coo, c.us, None, device=DEV), cols)
    users, val, avail, util = qrlsh.for_queries(rt, *coo, c.us, None, 5, device=DEV, utility=True)
    assert_same(host(users, val, avail), top, "every column in blocks")
    assert np.array_equal(util.words, whole)
    assert np.array_equal(qrlsh.query_utility(rt, *coo, c.us, [29, 3, 3, 0, 12, 7, 7, 1, 2], device=DEV).words,
                          whole[[29, 3, 3, 0, 12, 7, 7, 1, 2]])


# ----------------------------------------------------------------------------------------------------- 7. flags
def test_flagged_inputs_raise_and_the_next_call_is_right(knife):
    """the refusals the contract promises; nothing here is built to make the device fault"""
    c, queries, finals = knife
    rt = torch.from_numpy(c.ratings).to(DEV)
    src, dst, mil = (t.clone() for t in c.coo())
    # a 65-entry list for query 200 (its own entries replaced)
    keep = src != 200
    long_ = tuple(torch.cat([t[keep], extra]) for t, extra in (
        (src, torch.full((65,), 200, dtype=torch.int32)), (dst, torch.arange(65, dtype=torch.int32)),
        (mil, torch.full((65,), 500, dtype=torch.int32))))
    order = torch.argsort(long_[0].to(torch.int64), stable=True)
    long_ = tuple(t[order] for t in long_)
    outside = dst.clone()
    outside[len(outside) // 2] = c.nq
    for call in (lambda *a: qrlsh.predict_queries(rt, *a, device=DEV),
                 lambda *a: qrlsh.for_queries(rt, *a, 5, device=DEV),
                 lambda *a: qrlsh.query_utility(rt, *a, device=DEV)):
        with pytest.raises(ValueError, match="more than 64"):
            call(*long_, c.us, queries)
        with pytest.raises(ValueError, match="neighbour index"):
            call(src, outside, mil, c.us, queries)
        with pytest.raises(ValueError, match="query id %d" % c.nq):
            call(src, dst, mil, c.us, torch.tensor([3, c.nq], device=DEV))
        with pytest.raises(ValueError, match="query id -1"):
            call(src, dst, mil, c.us, torch.tensor([-1], dtype=torch.int64, device=DEV))
        with pytest.raises(ValueError, match="query id"):
            call(src, dst, mil, c.us, torch.tensor([2**32 + 1], dtype=torch.int64, device=DEV))   # clamped, not wrapped
        with pytest.raises(ValueError, match="query id"):
            call(src, dst, mil, c.us, [2**32 + 1])                                        # a host id past int32
    torch.cuda.synchronize()
    got = host(qrlsh.predict_queries(rt, src, dst, mil, c.us, queries, device=DEV))
    assert np.array_equal(got, SQ.restate_columns(finals["pairwise"], queries))
    assert_same(host(*qrlsh.for_queries(rt, src, dst, mil, c.us, queries, 5, device=DEV)),
                SQ.restate_top_users(c.ratings, finals["pairwise"], queries, 5), "after the flagged calls")


# ----------------------------------------------------------------------------------------------------- 8. Recommender
@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_serves_chosen_queries_in_every_state(sub):
    """recommend_queries / predict_queries / query_utility against compute_scores(reuse_lists=True)'s matrix, given the
    user lists of the live user index, after every live operation"""
    from test_gpu_recommend import _recommender_on
    from qrlsh import pipeline, users as U
    import users_cases as UC
    rec, g = _recommender_on(sub)
    N, nu = rec.queriesIDs.size, rec.usersIDs.size
    n0 = N - 9
    block = rec.ratings[:, n0:].copy()
    rest, ids = np.asarray(rec.queries, dtype=object)[n0:], rec.queriesIDs[n0:]
    rec.queries, rec.queriesIDs, rec.ratings = rec.queries[:n0], rec.queriesIDs[:n0], rec.ratings[:, :n0]
    rec.max_candidates = pipeline.max_candidates(N)
    np.random.seed(int(g["seed"]))
    with pytest.raises(ValueError, match="no live lists"):
        rec.recommend_queries([0], 5)
    rec.compute_querySimilarities()
    rec.live_user_similarities(labels=U.cluster_labels(rec.ratings))
    rng = np.random.default_rng(3)
    summation = ORDERS[rec.sum_order]

    def check(what):
        ui = rec.user_index
        assert (ui.nu, ui.nq) == rec.ratings.shape, what
        torch.cuda.synchronize()
        usim = UC.lists_to_dict((ui.idx.cpu().numpy(), ui.milli.cpu().numpy(), ui.len.cpu().numpy()))
        rec.compute_userSimilarities = lambda: usim
        try:
            final = rec.compute_scores(reuse_lists=True)[1]
        finally:
            del rec.compute_userSimilarities
        fin = final.to_numpy()
        nq = fin.shape[1]
        positions = [0, nq - 1, 7, 7, 3, nq // 2]
        cols = rec.predict_queries(positions)
        assert np.array_equal(cols.to_numpy(), fin[:, positions]), what
        assert list(cols.index) == list(final.index) and list(cols.columns) == list(final.columns[positions]), what
        assert np.array_equal(rec.predict_queries(None).to_numpy(), fin), what
        for k in (1, 7, 1024):
            users, val, avail = SQ.restate_top_users(rec.ratings, fin, positions, k)
            got = rec.recommend_queries(positions, k)
            assert sorted(got) == sorted(set(positions)), what
            for x, j in enumerate(positions):
                n = min(k, int(avail[x]))
                assert got[j]["available"] == int(avail[x]), (what, j)
                assert got[j]["users"].dtype == np.int64 and got[j]["values"].dtype == np.int64
                assert np.array_equal(got[j]["users"], users[x, :n]) and np.array_equal(got[j]["values"], val[x, :n]), (what, j)
        assert sum(e["available"] for e in rec.recommend_queries(torch.tensor(positions, device=DEV), 7).values()) > 0, what
        qs = rec.current_query_similarities()
        util = rec.query_utility(positions)
        assert np.array_equal(util.words, SQ.restate_words(rec.ratings, fin, qs, usim, positions, summation)), what
        every = rec.query_utility()
        assert np.array_equal(every.words[positions], util.words) and every.words.shape == (nq, 8), what

    check("after the run")
    rec.add_queries(rest, ratings=block, ids=ids, update_lists=True)
    assert rec.queriesIDs.size == N
    check("after add_queries")
    rec.remove_queries([0, N // 2, N - 1], update_lists=True)
    check("after remove_queries")
    newb = rng.integers(0, 101, size=(nu, 2)) * (rng.random((nu, 2)) < 0.3)
    rec.replace_queries([5, 1], np.asarray(rec.queries, dtype=object)[[8, 9]], ratings=newb, update_lists=True)
    check("after replace_queries")
    nq = rec.ratings.shape[1]
    us, qs_, vs = rng.integers(0, nu, size=12), rng.integers(0, nq, size=12), rng.integers(0, 101, size=12)
    us[:3], qs_[:3] = [0, 1, 2], [0, 7, 3]             # some edits land in the served columns
    assert rec.rate(us, qs_, vs) >= 1
    check("after rate")
    newcomers = np.vstack((np.where(rng.random(nq) < 0.9, rec.ratings[2], 0), np.zeros(nq, dtype=np.int64)))
    rec.add_users(newcomers)
    assert rec.ratings.shape[0] == nu + 2
    check("after add_users")
    rec.remove_users([1, nu])
    check("after remove_users")
    rec.set_list_lengths(query_K=3, user_K=2)
    check("after set_list_lengths")
