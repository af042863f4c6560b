"""Diversified lists on the device (qrlsh.diversify / for_users_diverse / list_redundancy,
Recommender.recommend_users_diverse / list_redundancy).  Expected values come from the host restatement
(diversify_cases.greedy_ref / redundancy_ref, checked in tests/test_diversify_host.py), over the planted cases, the
oracle's rows or the serving calls that existed before -- never from the code under test.  Every output word is compared."""
import importlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
import diversify_cases as DC
import predict_cases as PC
from test_recommend_users_host import oracle_rows, restate_users

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402

DEV = "cuda"
NAMES = ("idx", "val", "red", "count")


def host(*ts):
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def assert_same(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s %s shape %s != %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            raise AssertionError("%s %s differs at %s" % (what, name, np.argwhere(g != w)[:5].tolist()))


_cases, _refs = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = {"planted": DC.planted_case, "main": DC.main_case, "full": DC.full_order_case}.get(
            name, lambda: DC.size_case(int(name[4:])))()
    return _cases[name]


def ref(name, penalty, max_sim):
    """the restatement of one case under one setting, and the redundancy of its lists; computed once"""
    key = (name, penalty, max_sim)
    if key not in _refs:
        c = case(name)
        out = DC.greedy_ref(*c.arrays(), c.lists, c.k, penalty, max_sim)
        _refs[key] = (out, DC.redundancy_ref(out[0], c.lists))
    return _refs[key]


def check_case(name, penalty, max_sim, tensors=False):
    c = case(name)
    ci, cv, av = c.arrays()
    coo = c.coo()
    if tensors:
        ci, cv, av = (torch.from_numpy(a).to(DEV) for a in (ci, cv, av))
        coo = tuple(torch.from_numpy(a).to(DEV) for a in coo)
    what = "%s penalty=%d max_sim=%d" % (name, penalty, max_sim)
    want, (words, totals) = ref(name, penalty, max_sim)
    got = qrlsh.diversify(ci, cv, av, *coo, c.nq, c.k, penalty=penalty, max_sim=max_sim, device=DEV)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
    assert_same(host(*got), want, what)
    r = qrlsh.list_redundancy(got[0] if tensors else host(got[0]), *coo, c.nq, device=DEV)
    assert_same((r.words, r.totals), (words, totals), what, ("words", "totals"))
    assert r.words.dtype == np.int64 and r.totals.dtype == np.int64
    # the identities, on the device's own output
    assert int(host(got[2]).max(initial=0)) == int(r.totals[3])
    if max_sim == 1:
        assert int(r.totals[1]) == 0
    return got


# ------------------------------------------------------------------------------------------------- 1. planted cases
@pytest.mark.parametrize("penalty,max_sim", DC.SETTINGS)
def test_planted_structures(penalty, max_sim):
    check_case("planted", penalty, max_sim)


@pytest.mark.parametrize("penalty,max_sim", DC.SETTINGS)
def test_main_case_of_300_mixed_requests(penalty, max_sim):
    check_case("main", penalty, max_sim, tensors=(penalty == DC.MODERATE))


@pytest.mark.parametrize("N", DC.SIZES)
def test_pool_sizes(N):
    for penalty, max_sim in ((0, 1001), (DC.MODERATE, 1001), (0, 1)):
        check_case("size%d" % N, penalty, max_sim, tensors=(N % 2 == 1))


def test_whole_pool_reordered():
    for penalty, max_sim in ((DC.MODERATE, 1001), (1 << 20, 700), (0, 1)):
        check_case("full", penalty, max_sim)


def test_plain_setting_returns_the_pool_and_redundancy_of_padded_lists():
    c = case("main")
    ci, cv, av = c.arrays()
    idx, val, red, count = host(*qrlsh.diversify(ci, cv, av, *c.coo(), c.nq, c.k, device=DEV))
    assert np.array_equal(idx, np.where(np.arange(c.k)[None, :] < count[:, None], ci[:, :c.k], -1))
    assert np.array_equal(count, np.minimum(np.clip(av, 0, c.N), c.k)) and red.max() > 0
    # the whole padded pools as lists (k = 256, -1 padding inside the array)
    r = qrlsh.list_redundancy(ci, *c.coo(), c.nq, device=DEV)
    words, totals = DC.redundancy_ref(ci, c.lists)
    assert_same((r.words, r.totals), (words, totals), "pools as lists", ("words", "totals"))
    assert r.pairs_per_list == totals[1] / len(av) and r.mean_sim == totals[2] / totals[1] / 1000.0
    empty = qrlsh.list_redundancy(np.zeros((0, 5), dtype=np.int32), *c.coo(), c.nq, device=DEV)
    assert empty.words.shape == (0, 4) and empty.totals.tolist() == [0, 0, 0, 0] and empty.mean_sim == 0.0
    none = qrlsh.diversify(ci[:0], cv[:0], av[:0], *c.coo(), c.nq, c.k, device=DEV)
    assert [tuple(t.shape) for t in none] == [(0, c.k)] * 3 + [(0,)]


# ------------------------------------------------------------------------------------------------------ 2. row blocks
def test_row_blocked_calls_equal_one_call(monkeypatch):
    dv = importlib.import_module("qrlsh.diversify")
    lib = qrlsh._lib.load()
    c = case("main")
    ci, cv, av = c.arrays()
    want, (words, totals) = ref("main", DC.MODERATE, 1001)
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in ("qrlsh_diversify", "qrlsh_list_redundancy"):
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn
    monkeypatch.setattr(dv._lib, "load", lambda: Counting())
    monkeypatch.setattr(dv, "WORKSPACE_BUDGET", int(lib.qrlsh_diversify_workspace_bytes(40, c.N, DC.K_LISTS)))
    got = qrlsh.diversify(ci, cv, av, *c.coo(), c.nq, c.k, penalty=DC.MODERATE, device=DEV)
    assert_same(host(*got), want, "blocked")
    assert calls.count("qrlsh_diversify") == 8       # 300 -> blocks of 38
    monkeypatch.setattr(dv, "WORKSPACE_BUDGET", int(lib.qrlsh_diversify_workspace_bytes(40, c.k, DC.K_LISTS)))
    r = qrlsh.list_redundancy(got[0], *c.coo(), c.nq, device=DEV)
    assert_same((r.words, r.totals), (words, totals), "blocked", ("words", "totals"))
    assert calls.count("qrlsh_list_redundancy") == 8


def test_list_redundancy_in_row_blocks_equals_its_single_call(monkeypatch):
    dv = importlib.import_module("qrlsh.diversify")
    lib = qrlsh._lib.load()
    c = case("main")
    pools = c.arrays()[0]                                # the padded pools as lists of N entries
    whole = qrlsh.list_redundancy(pools, *c.coo(), c.nq, device=DEV)
    calls = []
    real = lib.qrlsh_list_redundancy

    def counted(*args):
        calls.append(args[1])
        return real(*args)
    monkeypatch.setattr(lib, "qrlsh_list_redundancy", counted)
    monkeypatch.setattr(dv, "WORKSPACE_BUDGET", int(lib.qrlsh_diversify_workspace_bytes(40, c.N, DC.K_LISTS)))
    split = qrlsh.list_redundancy(pools, *c.coo(), c.nq, device=DEV)
    assert calls == [38] * 7 + [34]                      # 300 -> 150 -> 75 -> 38 per call, a short last block
    assert_same((split.words, split.totals), (whole.words, whole.totals), "blocked", ("words", "totals"))


# ------------------------------------------------------------------------------------------------------- 3. serving
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}
USERS = [0, 3, 9, 200, 332, 3]


@pytest.fixture(scope="module")
def knife():
    c = PC.build_case(16, nu=333, nq=5003, tu=10, tq=100, user_longest=32)
    return c, c.coo(), DC.lists_from_sims(c.qs)


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_for_users_diverse_equals_the_rerank_of_for_users_and_the_oracle_rows(knife, order):
    c, coo, lists = knife
    rows = oracle_rows(c.ratings, c.qs, c.us, USERS, summation=ORDERS[order])
    for k, pool, penalty, max_sim in ((40, None, 3000, 1001), (28, 1024, 0, 1), (300, 300, 1 << 20, 900)):
        n = 160 if pool is None else pool          # the default pool of k = 40
        pi, pv, pa = restate_users(c.ratings, rows, USERS, n)
        want = DC.greedy_ref(pi, pv, pa, lists, k, penalty, max_sim)
        # the setting does something to these pools: every list changes, and the last one ends before k
        plain = DC.greedy_ref(pi, pv, pa, lists, k, 0, 1001)
        assert (plain[0] != want[0]).any(axis=1).sum() >= 4 and plain[2].max() > 0
        assert (want[3] < k).all() == (k == 300)
        got = qrlsh.for_users_diverse(c.ratings, *coo, c.us, USERS, k, pool=pool, penalty=penalty, max_sim=max_sim,
                                      sum_order=order, device=DEV)
        what = "%s k=%d pool=%s penalty=%d max_sim=%d" % (order, k, pool, penalty, max_sim)
        assert_same(host(*got), want + (pa,), what, NAMES + ("avail",))
        served = qrlsh.for_users(c.ratings, *coo, c.us, USERS, n, sum_order=order, device=DEV)
        assert_same(host(*served), (pi, pv, pa), what, ("idx", "val", "avail"))
        again = qrlsh.diversify(*served, *coo, c.nq, k, penalty=penalty, max_sim=max_sim, device=DEV)
        assert_same(host(*again), want, what + " two calls")


# --------------------------------------------------------------------------------------------------------- 4. flags
def test_flagged_inputs_raise_and_return_nothing():
    c = case("main")
    ci, cv, av = c.arrays()
    src, dst, mil = c.coo()
    x = int(np.argmax(av >= 20))
    outside = dst.copy()
    outside[len(outside) // 2] = c.nq
    with pytest.raises(ValueError, match="neighbour index"):
        qrlsh.diversify(ci, cv, av, src, outside, mil, c.nq, c.k, device=DEV)
    with pytest.raises(ValueError, match="neighbour index"):
        qrlsh.list_redundancy(ci, src, outside, mil, c.nq, device=DEV)
    for bad in (c.nq, -1, -7):
        b = ci.copy()
        b[x, 5] = bad
        with pytest.raises(ValueError, match="candidate column"):
            qrlsh.diversify(b, cv, av, src, dst, mil, c.nq, c.k, device=DEV)
    b = ci.copy()
    b[x, 7] = -7                              # -1 is padding in a list, anything else is not
    with pytest.raises(ValueError, match="candidate column"):
        qrlsh.list_redundancy(b, src, dst, mil, c.nq, device=DEV)
    b = ci.copy()
    b[x, 9] = b[x, 2]
    with pytest.raises(ValueError, match="twice"):
        qrlsh.diversify(b, cv, av, src, dst, mil, c.nq, c.k, device=DEV)
    with pytest.raises(ValueError, match="twice"):
        qrlsh.list_redundancy(torch.from_numpy(b).to(DEV), src, dst, mil, c.nq, device=DEV)
    # a bad column past avail is never read as a candidate
    b = ci.copy()
    b[x, av[x]:] = c.nq + 5
    want, _ = ref("main", 0, 1001)
    if av[x] < c.N:
        assert_same(host(*qrlsh.diversify(b, cv, av, src, dst, mil, c.nq, c.k, device=DEV)), want, "past avail")
    assert_same(host(*qrlsh.diversify(ci, cv, av, src, dst, mil, c.nq, c.k, device=DEV)), want, "after the flagged calls")


# ---------------------------------------------------------------------------------------------------- 5. Recommender
def test_recommender_serves_diverse_lists_in_every_state():
    """recommend_users_diverse against greedy_ref over recommend_users(k = pool) and current_query_similarities(),
    after the run, after add_queries(update_lists=True) and after remove_queries(update_lists=True)"""
    from test_gpu_recommend import _recommender_on
    from qrlsh import pipeline
    rec, g = _recommender_on("cfg2")
    N, nu = rec.queriesIDs.size, rec.usersIDs.size
    n0 = N - 9
    block = rec.ratings[:, n0:].copy()
    rest, ids = np.asarray(rec.queries, dtype=object)[n0:], rec.queriesIDs[n0:]
    rec.queries, rec.queriesIDs, rec.ratings = rec.queries[:n0], rec.queriesIDs[:n0], rec.ratings[:, :n0]
    rec.max_candidates = pipeline.max_candidates(N)
    np.random.seed(int(g["seed"]))
    users = [0, nu - 1, 7, 7, 3]
    with pytest.raises(ValueError, match="no live lists"):
        rec.recommend_users_diverse(users, 5, 1000)
    rec.compute_querySimilarities()
    changed = []

    def check(what):
        usim = type(rec).compute_userSimilarities(rec)
        lists = DC.lists_from_sims(rec.current_query_similarities())
        for k, pool, penalty, max_sim in ((7, None, 5000, 1001), (5, 40, 0, 1), (12, 12, 1 << 20, 800)):
            n = 64 if pool is None else pool
            served = rec.recommend_users(users, n, user_sim=usim)
            m = len(users)
            pi, pv = np.full((m, n), -1, dtype=np.int32), np.zeros((m, n), dtype=np.int32)
            pa = np.array([served[u]["available"] for u in users], dtype=np.int32)
            for x, u in enumerate(users):
                pi[x, :len(served[u]["indexes"])] = served[u]["indexes"]
                pv[x, :len(served[u]["values"])] = served[u]["values"]
            idx, val, red, count = DC.greedy_ref(pi, pv, pa, lists, k, penalty, max_sim)
            got = rec.recommend_users_diverse(users, k, penalty, max_sim=max_sim, pool=pool, user_sim=usim)
            assert sorted(got) == sorted(set(users)), what
            for x, u in enumerate(users):
                e = got[u]
                assert e["available"] == pa[x] and all(e[f].dtype == np.int64 for f in ("indexes", "values", "redundancy"))
                assert np.array_equal(e["indexes"], idx[x, :count[x]]), (what, u)
                assert np.array_equal(e["values"], val[x, :count[x]]) and np.array_equal(e["redundancy"], red[x, :count[x]])
            first = list(dict.fromkeys(users))
            rows = [users.index(u) for u in first]
            r = rec.list_redundancy(got)
            words, totals = DC.redundancy_ref(idx[rows], lists)
            assert np.array_equal(r.words, words) and np.array_equal(r.totals, totals), what
            plain = rec.list_redundancy(rec.recommend_users(users, k, user_sim=usim))
            assert np.array_equal(plain.words, DC.redundancy_ref(pi[rows, :k], lists)[0]), what
            changed.append(not np.array_equal(idx[:, :k], pi[:, :k]))
    check("after the run")
    rec.add_queries(rest, ratings=block, ids=ids, update_lists=True)
    assert rec.queriesIDs.size == N
    check("after add_queries")
    rec.remove_queries([0, N // 2, N - 1], update_lists=True)
    assert rec.queriesIDs.size == N - 3
    check("after remove_queries")
    assert any(changed)
