"""The diversity grid on the device (qrlsh.diversify_grid / evaluate_diversity, Recommender.tune_diversity).  Expected
values come from the host restatement (diversify_grid_cases.grid_ref, checked in tests/test_diversify_grid_host.py),
from rank_eval_cases.rank_eval_ref, or from the calls the grid replaces (qrlsh.diversify, qrlsh.list_redundancy,
qrlsh.evaluate_ranking) -- every word of every (setting, request) is compared."""
import importlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
import diversify_cases as DC
import diversify_grid_cases as GC
import predict_cases as PC
import rank_eval_cases as RC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402

DEV = "cuda"
dv = importlib.import_module("qrlsh.diversify")
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}
LISTS = ("idx", "val", "red", "count")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def assert_grid(g, want, what, lists=True, per=True):
    wper, wtotals, wlists = want
    assert g.totals.dtype == np.int64 and g.totals.shape == wtotals.shape, what
    pairs = [("totals", g.totals, wtotals)]
    if per:
        assert g.per_request.is_cuda and g.per_request.dtype == torch.int64
        pairs.append(("per_request", host(g.per_request), wper))
    if lists:
        assert all(getattr(g, n).is_cuda and getattr(g, n).dtype == torch.int32 for n in LISTS)
        pairs += [(n, host(getattr(g, n)), w) for n, w in zip(LISTS, wlists)]
    for name, got, w in pairs:
        assert got.shape == w.shape, "%s %s shape %s != %s" % (what, name, got.shape, w.shape)
        if not np.array_equal(got, w):
            at = np.argwhere(got != w)[:5]
            raise AssertionError("%s: %s differs at %s: %s != %s" % (
                what, name, at.tolist(), [got[tuple(a)] for a in at], [w[tuple(a)] for a in at]))


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = {"planted": DC.planted_case, "main": DC.main_case, "full": DC.full_order_case}.get(
            name, lambda: DC.size_case(int(name[4:])))()
    return _cases[name]


def run(c, settings, kw=None, tensors=False, **more):
    ci, cv, av = c.arrays()
    coo = c.coo()
    kw = dict(kw or {})
    if tensors:
        ci, cv, av = (torch.from_numpy(a).to(DEV) for a in (ci, cv, av))
        coo = tuple(torch.from_numpy(a).to(DEV) for a in coo)
        kw = {n: torch.as_tensor(np.asarray(v)).to(DEV) if n in ("truth", "users", "request_counts") else v
              for n, v in kw.items()}
    return qrlsh.diversify_grid(ci, cv, av, *coo, c.nq, c.k, settings, device=DEV, **kw, **more)


# ------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("name", ["planted", "main"])
def test_every_word_of_the_planted_calls(name):
    c = case(name)
    kw, want = GC.scored(c)
    g = run(c, DC.SETTINGS, kw, want_per_request=True, want_lists=True, tensors=(name == "main"))
    assert_grid(g, want, name)
    assert g.settings == list(DC.SETTINGS)
    # the figures, from the expected integers
    t = want[1]
    assert g.ndcg == [t[s, 4] / t[s, 11] for s in range(6)] and g.precision == [t[s, 1] / t[s, 0] for s in range(6)]
    assert g.recall == [t[s, 1] / t[s, 5] for s in range(6)] and g.hit_rate == [t[s, 10] / t[s, 9] for s in range(6)]
    assert g.pairs_per_list == [t[s, 12] / t[s, 8] for s in range(6)] and g.ended_early == t[:, 17].tolist()
    assert g.changed_share[0] == 0.0 and min(g.changed_share[1:]) > 0.0
    # totals only: nothing else is allocated or returned
    bare = run(c, DC.SETTINGS, kw)
    assert bare.per_request is None and bare.idx is None and np.array_equal(bare.totals, t)


@pytest.mark.parametrize("N", DC.SIZES)
def test_pool_sizes(N):
    c = case("size%d" % N)
    settings = ((0, 1001), (DC.MODERATE, 1001), (0, 1))
    kw, want = GC.scored(c, settings)
    assert c.arrays()[2].tolist() == [N + 37, N, N - 1, 0, -1]
    assert_grid(run(c, settings, kw, want_per_request=True, want_lists=True, tensors=(N % 2 == 1)), want, c.name)


def test_whole_pool_reordered():
    c = case("full")
    settings = ((DC.MODERATE, 1001), (1 << 20, 700), (0, 1))
    kw, want = GC.scored(c, settings)
    assert c.k == c.N == 257
    assert_grid(run(c, settings, kw, want_per_request=True, want_lists=True), want, "full")


@pytest.fixture(scope="module")
def small():
    """a small call under 130 distinct settings: (case, scoring kwargs, settings, grid_ref's triple)"""
    c = DC.small_case(2)
    rng = np.random.default_rng(4)
    truth = (rng.integers(1, 101, (5, c.nq)) * (rng.random((5, c.nq)) < 0.6)).astype(np.int32)
    arrays = c.arrays()
    users = np.array([(3 * x) % 5 for x in range(len(arrays[2]))], dtype=np.int32)
    kw = dict(truth=truth, users=users, relevant=60, gains=RC.dcg_gains_ref(c.k),
              request_counts=GC.counts_of(arrays, truth, users, 60))
    settings = [(s, (1001, 600, 1, 1000)[s % 4]) for s in range(130)]   # a point of rating per 1000 milli: they bite
    return c, kw, settings, GC.grid_ref(arrays, c.lists, c.k, settings, **kw)


@pytest.mark.parametrize("S", [1, 128, 130])
def test_one_setting_a_full_call_and_two_stitched_calls(small, S):
    c, kw, settings, (per, totals, lists) = small
    assert len(set(p for p, _ in settings[:128])) == 128 and len(np.unique(totals[:, :16], axis=0)) >= 20
    g = run(c, settings[:S], kw, want_per_request=True, want_lists=True)
    assert_grid(g, (per[:S], totals[:S], tuple(a[:S] for a in lists)), "S=%d" % S)


def test_without_a_truth_and_without_request_counts():
    c = case("main")
    kw, want = GC.scored(c)
    arrays = c.arrays()
    bare = GC.grid_ref(arrays, c.lists, c.k, DC.SETTINGS, greedy=lambda p, ms: GC.greedy_of(c, p, ms))
    g = run(c, DC.SETTINGS, want_per_request=True, want_lists=True)
    assert_grid(g, bare, "no truth")
    assert not bare[0][:, :, 1:7].any() and bare[1][:, 12].max() > 0 and np.isnan(g.ndcg[0]) and g.pairs_per_list[0] > 0
    less = dict(kw, request_counts=None)
    nocount = GC.grid_ref(arrays, c.lists, c.k, DC.SETTINGS, greedy=lambda p, ms: GC.greedy_of(c, p, ms), **less)
    assert not nocount[1][:, [5, 6, 9, 11]].any() and nocount[1][:, 10].min() > 0
    assert_grid(run(c, DC.SETTINGS, less, want_per_request=True), nocount, "no counts", lists=False)


# -------------------------------------------------------------------------------------- 2. against the calls it replaces
def test_each_setting_equals_one_diversify_and_one_list_redundancy_call():
    c = case("main")
    kw, _ = GC.scored(c)
    ci, cv, av = c.arrays()
    g = run(c, DC.SETTINGS, kw, want_per_request=True, want_lists=True)
    per = host(g.per_request)
    for s, (penalty, max_sim) in enumerate(DC.SETTINGS):
        one = qrlsh.diversify(ci, cv, av, *c.coo(), c.nq, c.k, penalty=penalty, max_sim=max_sim, device=DEV)
        for name, a, b in zip(LISTS, one, (g.idx[s], g.val[s], g.red[s], g.count[s])):
            assert torch.equal(a, b), (name, s)
        r = qrlsh.list_redundancy(one[0], *c.coo(), c.nq, device=DEV)
        assert np.array_equal(per[s, :, 0], r.words[:, 0]) and np.array_equal(per[s, :, 8:11], r.words[:, 1:4])
        assert g.totals[s, [0, 12, 13, 14]].tolist() == r.totals.tolist()
        assert g.pairs_per_list[s] == r.pairs_per_list and g.mean_sim[s] == r.mean_sim
        assert g.totals[s, 15] == int(one[2].sum().item())


# ------------------------------------------------------------------------------------------------------ 3. row blocks
def test_row_blocked_calls_equal_one_call_and_the_totals_accumulate(monkeypatch):
    lib = qrlsh._lib.load()
    c = case("main")
    kw, want = GC.scored(c)
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name == "qrlsh_diversify_grid":
                return lambda *a: (calls.append(a[3]), fn(*a))[1]
            return fn
    monkeypatch.setattr(dv._lib, "load", lambda: Counting())
    monkeypatch.setattr(dv, "WORKSPACE_BUDGET", int(lib.qrlsh_diversify_workspace_bytes(40, c.N, DC.K_LISTS)))
    assert_grid(run(c, DC.SETTINGS, kw, want_per_request=True, want_lists=True), want, "blocked")
    assert calls == [38] * 7 + [34]       # 300 -> blocks of 38
    assert_grid(run(c, DC.SETTINGS, kw), want, "blocked, totals only", lists=False, per=False)
    # users=None: request x of a later block is still row x of the truth
    truth, relevant = GC.truth_case(nu=300, seed=92)
    arrays = c.arrays()
    rows = np.arange(300)
    mine = dict(truth=truth, relevant=relevant, gains=kw["gains"],
                request_counts=GC.counts_of(arrays, truth, rows, relevant))
    direct = GC.grid_ref(arrays, c.lists, c.k, DC.SETTINGS, greedy=lambda p, ms: GC.greedy_of(c, p, ms), **mine)
    del calls[:]
    assert_grid(run(c, DC.SETTINGS, mine, want_per_request=True), direct, "blocked, users=None", lists=False)
    assert len(calls) == 8


# ----------------------------------------------------------------------------------------------------------- 4. flags
def test_flagged_inputs_raise_and_return_nothing():
    c = case("main")
    kw, want = GC.scored(c)
    ci, cv, av = c.arrays()
    src, dst, mil = c.coo()
    x = int(np.argmax(av >= 20))

    def call(ci=ci, coo=(src, dst, mil), **over):
        return qrlsh.diversify_grid(ci, cv, av, *coo, c.nq, c.k, DC.SETTINGS, device=DEV, **dict(kw, **over))
    outside = dst.copy()
    outside[len(outside) // 2] = c.nq
    with pytest.raises(ValueError, match="neighbour index"):
        call(coo=(src, outside, mil))
    b = ci.copy()
    b[x, 9] = b[x, 2]
    with pytest.raises(ValueError, match="twice"):
        call(ci=b)
    for bad in (c.nq, -7):
        b = ci.copy()
        b[x, 5] = bad                           # never gathered from the truth
        with pytest.raises(ValueError, match="candidate column"):
            call(ci=b)
    for bad in (37, -1, 2**31 + 3):             # a device id is only seen by the library
        users = torch.from_numpy(kw["users"].astype(np.int64)).to(DEV)
        users[7] = bad
        with pytest.raises(ValueError, match="user id"):
            call(users=users)
    with pytest.raises(ValueError, match="user id"):
        call(users=np.where(np.arange(300) == 7, 37, kw["users"]))      # a host id: before the library
    with pytest.raises(ValueError, match="negative"):
        call(gains=[5, 4, 3, 2, 1, 0, 0, 0, 0, -1])
    # the library's own flags for what the host layer refuses first: a negative gain, a setting out of range
    dev = [torch.from_numpy(a).to(DEV) for a in (ci, cv, av)]
    csr = importlib.import_module("qrlsh.predict").lists_csr([torch.from_numpy(a) for a in (src, dst, mil)], c.nq, DEV)
    gain = np.array(kw["gains"], dtype=np.int64)

    def direct(settings, gain):
        prefix = np.concatenate(([0], np.cumsum(gain)))
        scoring = (torch.from_numpy(kw["truth"]).to(DEV), torch.from_numpy(kw["users"]).to(DEV), 60,
                   torch.from_numpy(gain).to(DEV), torch.from_numpy(prefix).to(DEV), None)
        return dv._grid(*dev, csr, c.nq, c.k, settings, DC.K_LISTS, DEV, scoring)
    minus = gain.copy()
    minus[c.k - 1] = -1
    with pytest.raises(ValueError, match="negative"):
        direct(list(DC.SETTINGS), minus)
    for bad in ((-1, 1001), ((1 << 20) + 1, 1001), (0, 1002), (0, -1)):
        with pytest.raises(ValueError, match="setting"):
            direct([DC.SETTINGS[1], bad], gain)
    assert np.array_equal(direct(list(DC.SETTINGS), gain).totals[:, [0, 1, 2, 3, 4, 7, 8, 10, 12, 13, 14, 15, 16, 17]],
                          want[1][:, [0, 1, 2, 3, 4, 7, 8, 10, 12, 13, 14, 15, 16, 17]])
    assert_grid(call(), want, "after the flagged calls", lists=False, per=False)


def test_a_bad_setting_raises_before_any_launch(monkeypatch):
    c = case("planted")

    def touched():
        raise AssertionError("touched the library")
    monkeypatch.setattr(dv._lib, "load", touched)
    for bad in ((-1, 1001), ((1 << 20) + 1, 1001), (0, 1002), (0, -1), (0.5, 1001)):
        with pytest.raises(ValueError):
            run(c, [(0, 1001), bad])


# ------------------------------------------------------------------------------------------ 5. the held-out evaluation
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_evaluate_diversity_on_a_split(order):
    train, truth, coo, qs, us = RC.split_case(7, 29, 200, fill=0.5, held=0.4, longest_q=7)
    coo = tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo)
    lists = DC.lists_from_sims(qs)
    k, pool, relevant = 10, 96, 60
    users = [3, 0, 28, 3, 17, 9, 11]
    settings = DC.SETTINGS
    pred = RC.candidate_predictions(train, qs, us, users, ORDERS[order])
    pi, pv, pa, pper, _ = RC.rank_eval_ref(train, truth, qs, us, users, pool, relevant, "all", RC.dcg_gains_ref(pool),
                                          ORDERS[order], pred=pred)
    want = GC.grid_ref((pi, pv, pa), lists, k, settings, truth=truth, users=users, relevant=relevant,
                       gains=RC.dcg_gains_ref(k), request_counts=pper[:, 5:7])
    assert pa.min() > pool and len(set(want[1][:, 4].tolist())) >= 2 and want[1][0, 12] > want[1][1, 12]
    assert want[1][1, 16] >= 4 and len(set(want[1][:, 1].tolist())) >= 2
    g = qrlsh.evaluate_diversity(train, truth, *coo, us, k, relevant, settings, pool=pool, users=users,
                                 sum_order=order, want_per_request=True, want_lists=True, device=DEV)
    assert_grid(g, want, order)
    # the plain setting is evaluate_ranking at k
    ev = qrlsh.evaluate_ranking(train, truth, *coo, us, k, relevant, users=users, candidates="all", sum_order=order,
                                device=DEV)
    assert np.array_equal(g.totals[0, :12], ev.totals[:12]) and not ev.totals[12:].any()
    assert torch.equal(g.per_request[0, :, :8], ev.per_user) and torch.equal(g.idx[0], ev.idx)
    assert (g.precision[0], g.recall[0], g.ndcg[0], g.hit_rate[0]) == (ev.precision, ev.recall, ev.ndcg, ev.hit_rate)
    # every user, the default pool, device matrices, totals only
    every = qrlsh.evaluate_diversity(torch.from_numpy(train).to(DEV), torch.from_numpy(truth).to(DEV), *coo, us, k,
                                     relevant, [(0, 1001), (DC.MODERATE, 1001)], sum_order=order, device=DEV)
    ev = qrlsh.evaluate_ranking(train, truth, *coo, us, k, relevant, sum_order=order, device=DEV)
    assert np.array_equal(every.totals[0, :12], ev.totals[:12]) and every.totals[1, 16] > 0 and every.per_request is None


# ------------------------------------------------------------------------------------------------------ 6. Recommender
def test_recommender_tunes_the_rerank_in_every_state():
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
    settings = [(0, 1001), (5000, 1001), (1 << 20, 1001), (0, 1), (20000, 700)]
    k, relevant, fraction, seed = 7, 60, 0.3, 11
    with pytest.raises(ValueError, match="no live lists"):
        rec.tune_diversity(k, relevant, settings)
    rec.compute_querySimilarities()
    users = [0, nu - 1, 7, 7, 3]
    usim = type(rec).compute_userSimilarities(rec)

    def state():
        qi = getattr(rec, "_query_index", None)
        index = [] if qi is None else [v.clone() for _, v in sorted(vars(qi).items()) if isinstance(v, torch.Tensor)]
        return ([t.clone() for t in rec._live_lists()], index, rec.ratings.copy(),
                (rec.query_weight, rec.user_weight, rec.default_mean))

    def same(a, b):
        return (all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1])) and len(a[1]) == len(b[1])
                and np.array_equal(a[2], b[2]) and a[3] == b[3])
    differ = []

    def check(what):
        before, keys = state(), set(vars(rec))
        grid = rec.tune_diversity(k, relevant, settings, fraction=fraction, seed=seed, user_sim=usim)
        assert same(before, state()) and (rec.diversity_penalty, rec.diversity_max_sim) == (0, 1001), what
        assert "diversity_penalty" not in vars(rec)
        lists, order, train, truth, user_sim = rec._holdout_inputs(fraction, seed, None, usim)
        want = qrlsh.evaluate_diversity(train, truth, *lists, user_sim, k, relevant, settings, sum_order=order,
                                        query_weight=rec.query_weight, user_weight=rec.user_weight,
                                        default_mean=rec.default_mean, device=DEV)
        assert np.array_equal(grid.totals, want.totals) and grid.ndcg == want.ndcg, what
        ev = rec.evaluate_ranking(k, relevant, fraction=fraction, seed=seed, user_sim=usim)
        assert np.array_equal(grid.totals[0, :12], ev.totals[:12]) and grid.totals[0, 8] == nu, what
        assert grid.totals[0, 16] == 0 and grid.totals[0, 1] > 0 and grid.totals[3, 12] == 0, what
        differ.append(len(set(grid.totals[:, 4].tolist())) > 1 and grid.totals[1, 12] < grid.totals[0, 12])
        # a request list and a pool of its own
        part = rec.tune_diversity(k, relevant, settings[:2], pool=40, fraction=fraction, seed=seed, users=users,
                                  user_sim=usim)
        assert part.totals[0, 8] == len(users), what
        assert np.array_equal(part.totals[0, :12], rec.evaluate_ranking(
            k, relevant, fraction=fraction, seed=seed, users=users, user_sim=usim).totals[:12]), what
        # before apply: the plain list
        plain = rec.recommend_users(users, k, user_sim=usim)
        got = rec.recommend_users_diverse(users, k, user_sim=usim)
        assert all(np.array_equal(got[u]["indexes"], plain[u]["indexes"]) for u in plain), what
        # apply: the two attributes, and nothing else
        tuned = rec.tune_diversity(k, relevant, settings[1:], fraction=fraction, seed=seed, user_sim=usim,
                                   max_pairs_per_list=0.0, apply=True)
        penalty, max_sim, index = tuned.best(max_pairs_per_list=0.0)
        assert (penalty, max_sim) == settings[1 + index] == (rec.diversity_penalty, rec.diversity_max_sim), what
        assert tuned.pairs_per_list[index] == 0.0
        assert sorted(vars(rec).keys() - keys) == ["diversity_max_sim", "diversity_penalty"]
        assert same(before, state()), what
        explicit = rec.recommend_users_diverse(users, k, penalty, max_sim=max_sim, user_sim=usim)
        got = rec.recommend_users_diverse(users, k, user_sim=usim)
        assert all(np.array_equal(got[u][f], explicit[u][f]) for u in explicit
                   for f in ("indexes", "values", "redundancy"))
        if max_sim == 1:
            assert rec.list_redundancy(got).totals[1] == 0
        by_ndcg = rec.tune_diversity(k, relevant, settings, fraction=fraction, seed=seed, user_sim=usim, apply=True)
        assert (rec.diversity_penalty, rec.diversity_max_sim) == by_ndcg.best()[:2], what
        with pytest.raises(ValueError, match="pairs_per_list"):
            rec.tune_diversity(k, relevant, settings[:1], fraction=fraction, seed=seed, user_sim=usim,
                               max_pairs_per_list=-1.0, apply=True)
        assert (rec.diversity_penalty, rec.diversity_max_sim) == by_ndcg.best()[:2], what    # a refusal changes nothing
        del rec.diversity_penalty, rec.diversity_max_sim
    check("after the run")
    rec.add_queries(rest, ratings=block, ids=ids, update_lists=True)
    usim = type(rec).compute_userSimilarities(rec)
    check("after add_queries")
    rec.remove_queries([0, N // 2, N - 1], update_lists=True)
    usim = type(rec).compute_userSimilarities(rec)
    check("after remove_queries")
    assert any(differ)
