"""The diversity grid (qrlsh.diversify_grid / evaluate_diversity / DiversityGrid, Recommender.tune_diversity): what needs
no device.  The restatement the GPU tests hold the device to (diversify_grid_cases.grid_ref) against a form built on
the dense brute rule; its identities; the choosers of DiversityGrid; the stitching of settings and row blocks, over a
stand-in for the library's entry point that writes what it was handed; the argument checks of the C ABI (fake
pointers: each call fails a check before anything is dereferenced) and of the host layer (before the library is
loaded); and the conditions that make the GPU comparison mean something, asserted on the restatement alone."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import diversify_cases as DC
import diversify_grid_cases as GC
import rank_eval_cases as RC

dv = importlib.import_module("qrlsh.diversify")


@pytest.fixture(scope="module")
def main():
    c = DC.main_case()
    return c, GC.scored(c)


@pytest.fixture(scope="module")
def planted():
    c = DC.planted_case()
    return c, GC.scored(c)


# ------------------------------------------------------------------------------------------- restatement vs brute form
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_grid_ref_equals_the_dense_brute_form(seed):
    c = DC.small_case(seed)
    arrays = c.arrays()
    ci, cv, av = arrays
    m = len(av)
    dense = DC.brute_sim(c.lists, c.nq)
    rng = np.random.default_rng(seed)
    truth = (rng.integers(1, 101, (5, c.nq)) * (rng.random((5, c.nq)) < 0.6)).astype(np.int32)
    users = np.array([(3 * x) % 5 for x in range(m)])
    gains = RC.dcg_gains_ref(c.k)
    counts = GC.counts_of(arrays, truth, users, 60)
    settings = ((0, 1001), (700, 1001), (1 << 20, 1001), (0, 1000), (0, 1), (300, 400))

    def dense_words(idx):
        words = np.zeros((m, 4), dtype=np.int64)
        for x, row in enumerate(idx):
            cols = row[row >= 0].astype(np.int64)
            sub = np.triu(dense[np.ix_(cols, cols)], 1)
            words[x] = [len(cols), int((sub > 0).sum()), int(sub.sum()), int(sub.max()) if sub.size else 0]
        return words, None
    kw = dict(truth=truth, users=users, relevant=60, gains=gains, request_counts=counts)
    got = GC.grid_ref(arrays, c.lists, c.k, settings, **kw)
    want = GC.grid_ref(arrays, None, c.k, settings, redundancy=dense_words,
                       greedy=lambda p, ms: DC.greedy_brute(ci, cv, av, dense, c.k, p, ms), **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all(np.array_equal(g, w) for g, w in zip(got[2], want[2]))
    per, totals, (idx, val, red, count) = got
    # the scoring words from numpy over the lists, the totals from the lines
    for s in range(len(settings)):
        for x in range(m):
            t = count[s, x]
            tv = truth[users[x], idx[s, x, :t].astype(np.int64)]
            hit = np.nonzero(tv >= 60)[0]
            assert per[s, x, :5].tolist() == [t, len(hit), int((tv != 0).sum()), int(hit[0]) + 1 if len(hit) else 0,
                                              sum(gains[p] for p in hit)]
            assert per[s, x, 5:8].tolist() == counts[x].tolist() + [av[x]] and per[s, x, 11] == red[s, x].sum()
        assert totals[s, :8].tolist() == per[s, :, :8].sum(axis=0).tolist() and totals[s, 8] == m
        assert totals[s, 9] == (counts[:, 0] > 0).sum() and totals[s, 10] == (per[s, :, 1] > 0).sum()
        assert totals[s, 11] == sum(sum(gains[:min(c.k, r)]) for r in counts[:, 0])
        assert totals[s, 12:16].tolist() == [per[s, :, 8].sum(), per[s, :, 9].sum(), per[s, :, 10].max(),
                                             per[s, :, 11].sum()]
        assert not totals[s, 18:].any()
    assert totals[0, 16] == totals[0, 17] == 0 and (totals[1:, 16] > 0).all() and totals[4, 17] > 0
    assert len(set(totals[:, 1].tolist())) >= 2
    # without a truth the ranking words stay 0 and the rest is unchanged
    bare = GC.grid_ref(arrays, c.lists, c.k, settings)
    assert not bare[0][:, :, 1:7].any() and not bare[1][:, [1, 2, 3, 4, 5, 6, 9, 10, 11]].any()
    assert np.array_equal(bare[0][:, :, 7:], per[:, :, 7:]) and np.array_equal(bare[1][:, 12:], totals[:, 12:])
    assert np.array_equal(bare[0][:, :, 0], per[:, :, 0])


def test_plain_setting_is_the_ranking_evaluation_of_the_prefix():
    """setting (0, 1001) over rank_eval_ref's pools at k = pool: words 0-7 are rank_eval_ref's lines at k"""
    train, truth, coo, qs, us = RC.split_case(5, 11, 140, fill=0.5, held=0.4)
    lists = DC.lists_from_sims(qs)
    k, pool, relevant = 6, 64, 60
    users = [3, 0, 10, 3, 7]
    pred = RC.candidate_predictions(train, qs, us, users)
    pi, pv, pa, pper, _ = RC.rank_eval_ref(train, truth, qs, us, users, pool, relevant, "all", RC.dcg_gains_ref(pool),
                                          pred=pred)
    _, _, _, want, want_totals = RC.rank_eval_ref(train, truth, qs, us, users, k, relevant, "all", RC.dcg_gains_ref(k),
                                                  pred=pred)
    assert pa.max() > k and want[:, 1].sum() > 0
    per, totals, (idx, _, _, count) = GC.grid_ref(
        (pi, pv, pa), lists, k, ((0, 1001), (DC.MODERATE, 1001)), truth=truth, users=users, relevant=relevant,
        gains=RC.dcg_gains_ref(k), request_counts=pper[:, 5:7])
    assert np.array_equal(per[0, :, :8], want) and np.array_equal(totals[0, :12], want_totals[:12])
    assert totals[0, 16] == totals[0, 17] == 0
    assert np.array_equal(idx[0], pi[:, :k]) and np.array_equal(count[0], np.minimum(pa, k))
    assert np.array_equal(per[1, :, 5:8], want[:, 5:8])   # the counts and avail do not depend on the setting


# --------------------------------------------------------------------------------------- the conditions of the cases
def test_main_case_conditions(main):
    c, (kw, (per, totals, (idx, val, red, count))) = main
    ci, cv, av = c.arrays()
    assert list(DC.SETTINGS) == [(0, 1001), (DC.MODERATE, 1001), (1 << 20, 1001), (0, 1000), (0, 1), (5000, 500)]
    assert per.shape == (6, 300, 12) and c.N == 256 and c.k == 10
    changed_dcg = [(per[s, :, 4] != per[0, :, 4]).sum() for s in range(1, 6)]
    assert min(changed_dcg) >= 100, changed_dcg
    assert len(set(totals[:, 12].tolist())) >= 4, totals[:, 12]
    assert totals[4, 17] >= 10 and totals[3, 17] >= 10, totals[:, 17]
    assert len(set(totals[:, 1].tolist())) >= 3, totals[:, 1]
    assert totals[0, 16] == 0 and totals[0, 17] == 0 and totals[4, 12] == 0
    # word 11 is the sum of red, word 10 its maximum
    assert np.array_equal(per[:, :, 11], red.sum(axis=2)) and np.array_equal(per[:, :, 10], red.max(axis=2))
    # requests without a relevant test cell and requests not served are both there
    assert 0 < totals[0, 9] < totals[0, 8] == (av >= 0).sum() and len(set(kw["users"].tolist())) < 300


def test_planted_case_conditions(planted):
    c, (kw, (per, totals, lists)) = planted
    assert per.shape[1] == 9
    assert (per[4, :, 1] != per[0, :, 1]).sum() >= 6
    assert totals[0, 12] > totals[1, 12] > 0, totals[:, 12]
    assert np.array_equal(per[:, :, 11], lists[2].sum(axis=2))


# ---------------------------------------------------------------------------------------------------- the choosers
def _grid_of(rows):
    """rows: (hits, listed, dcg, ideal, pairs, sim_sum) per setting, 10 requests each"""
    totals = np.zeros((len(rows), 24), dtype=np.int64)
    for s, (hits, listed, dcg, ideal, pairs, sim) in enumerate(rows):
        totals[s, [1, 0, 4, 11, 12, 13, 8, 5, 9, 10]] = [hits, listed, dcg, ideal, pairs, sim, 10, 50, 10, min(hits, 10)]
    return dv.DiversityGrid([(100 * s, 1001 - s) for s in range(len(rows))], totals)


def test_choosers_order_and_ties():
    g = _grid_of([(30, 100, 900, 1000, 40, 9000), (30, 100, 950, 1000, 30, 8000), (30, 100, 950, 1000, 20, 7000),
                  (20, 100, 940, 1000, 5, 900), (20, 100, 940, 1000, 5, 800), (10, 100, 500, 1000, 0, 0)])
    assert g.ndcg == [0.9, 0.95, 0.95, 0.94, 0.94, 0.5] and g.precision[0] == 0.3 and g.recall[3] == 0.4
    assert g.pairs_per_list == [4.0, 3.0, 2.0, 0.5, 0.5, 0.0] and g.mean_sim[0] == 0.225 and g.mean_sim[5] == 0.0
    assert g.hit_rate == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0] and g.setting(2) == (200, 999)
    assert g.best() == (100, 1000, 1)                               # the first of the two 0.95
    assert g.best("precision") == (0, 1001, 0)
    assert g.best(max_pairs_per_list=2.0) == (200, 999, 2)
    assert g.best(max_pairs_per_list=1) == (300, 998, 3)            # the first of the two 0.94
    assert g.best(max_pairs_per_list=0) == (500, 996, 5)
    with pytest.raises(ValueError, match="pairs_per_list"):
        g.best(max_pairs_per_list=-1)
    with pytest.raises(ValueError, match="metric"):
        g.best("rmse")
    # within 0.98 of 0.95: settings 1 - 4; the fewest pairs: 3 and 4; the smaller sim sum: 4
    assert g.least_redundant() == (400, 997, 4)
    assert g.least_redundant(keep=1.0) == (200, 999, 2)
    assert g.least_redundant(keep=0.0) == (500, 996, 5)
    assert g.least_redundant("precision", keep=1.0) == (200, 999, 2)
    tie = _grid_of([(30, 100, 900, 1000, 7, 70), (30, 100, 900, 1000, 7, 70)])
    assert tie.best() == (0, 1001, 0) and tie.least_redundant() == (0, 1001, 0)
    # no truth: no figure, nobody wins
    bare = dv.DiversityGrid([(0, 1001)], np.zeros((1, 24), dtype=np.int64))
    assert np.isnan(bare.ndcg[0]) and bare.pairs_per_list == [0.0] and bare.changed_share == [0.0]
    with pytest.raises(ValueError):
        bare.best()
    with pytest.raises(ValueError):
        bare.least_redundant()
    t = np.zeros((1, 24), dtype=np.int64)
    t[0, [8, 16, 17]] = [8, 2, 1]
    assert dv.DiversityGrid([(5, 7)], t).changed_share == [0.25] and dv.DiversityGrid([(5, 7)], t).ended_early == [1]


# ------------------------------------------------------------------------- stitching, over a stand-in entry point
class _Echo:
    """the library with qrlsh_diversify_grid replaced by a function that writes what it was handed: per setting the
    penalty into totals word 0 (added), the block's requests into word 8 (added); per (setting, request) the penalty,
    max_sim and avail into the line and the lists"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def qrlsh_diversify_grid(self, ci, cv, av, m, N, nq, qo, qi, qm, k, pen, cut, S, truth, nu, users, relevant, gain,
                             prefix, counts, io, vo, ro, co, per, totals, flag, ws, ws_bytes, stream):
        def arr(p, ctype, n):
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(n,))
        self.calls.append((m, S))
        assert 1 <= S <= 128 and ws_bytes >= self.lib.qrlsh_diversify_workspace_bytes(m, N, 0)
        pen, cut, av = arr(pen, ctypes.c_int64, S), arr(cut, ctypes.c_int32, S), arr(av, ctypes.c_int32, m)
        tot = arr(totals, ctypes.c_int64, 24 * S).reshape(S, 24)
        tot[:, 0] += pen
        tot[:, 8] += m
        if per:
            line = arr(per, ctypes.c_int64, S * m * 12).reshape(S, m, 12)
            line[:, :, 0], line[:, :, 10], line[:, :, 7] = pen[:, None], cut[:, None], av[None, :]
        if io:
            arr(io, ctypes.c_int32, S * m * k).reshape(S, m, k)[:] = (pen[:, None] + av[None, :])[:, :, None]
            arr(co, ctypes.c_int32, S * m).reshape(S, m)[:] = cut[:, None] - av[None, :]
        return 0


@pytest.mark.parametrize("blocked", [False, True])
def test_settings_past_128_and_row_blocks_are_stitched(monkeypatch, blocked):
    from qrlsh import _lib
    real = _lib.load()
    echo = _Echo(real)
    monkeypatch.setattr(dv._lib, "load", lambda: echo)
    monkeypatch.setattr(dv, "_stream", lambda: None)
    m, N, k, S = 11, 16, 4, 130
    if blocked:
        monkeypatch.setattr(dv, "WORKSPACE_BUDGET", int(real.qrlsh_diversify_workspace_bytes(4, N, 1)))
    ci = np.tile(np.arange(N, dtype=np.int32), (m, 1))
    av = np.arange(m, dtype=np.int32)
    settings = [(7 * s, 1001 - (s % 9)) for s in range(S)]
    g = dv.diversify_grid(ci, ci, av, [0], [1], [500], 40, k, settings, want_per_request=True, want_lists=True,
                          device="cpu")
    rows = [3, 3, 3, 2] if blocked else [11]     # 11 -> blocks of 3
    assert echo.calls == [(r, s) for s in (128, 2) for r in rows]
    assert g.settings == settings and g.totals.shape == (130, 24)
    assert g.totals[:, 0].tolist() == [7 * s * len(rows) for s in range(S)] and (g.totals[:, 8] == m).all()
    assert g.per_request.shape == (S, m, 12) and g.idx.shape == (S, m, k) and g.count.shape == (S, m)
    pen, cut = np.array([p for p, _ in settings]), np.array([c for _, c in settings])
    per = g.per_request.numpy()
    assert np.array_equal(per[:, :, 0], np.tile(pen[:, None], (1, m)))
    assert np.array_equal(per[:, :, 10], np.tile(cut[:, None], (1, m)))
    assert np.array_equal(per[:, :, 7], np.tile(av[None, :], (S, 1)))
    assert np.array_equal(g.idx.numpy(), np.broadcast_to((pen[:, None] + av[None, :])[:, :, None], (S, m, k)))
    assert np.array_equal(g.count.numpy(), cut[:, None] - av[None, :])
    assert g.val is not None and g.red is not None
    bare = dv.diversify_grid(ci, ci, av, [0], [1], [500], 40, k, settings[:3], device="cpu")
    assert bare.per_request is None and bare.idx is None and bare.count is None and bare.totals.shape == (3, 24)


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def _grid(lib, m=4, N=64, nq=5000, k=10, S=6, nu=9, relevant=60, truth=True, gains=True, settings=True, flag=True,
          totals=True, pools=True, lists=True, ws_bytes=None, ws_addr=None):
    ci, cv, av, qo, qi, qm, pe, ms, tr, us, ga, gp, rc, io, vo, ro, co, pr, to, fl, ws = _fake(21)
    need = lib.qrlsh_diversify_workspace_bytes(m, N, 28) if ws_bytes is None else ws_bytes
    return lib.qrlsh_diversify_grid(ci if pools else None, cv, av, m, N, nq, qo if lists else None, qi, qm, k,
                                    pe if settings else None, ms, S, tr if truth else None, nu, us, relevant,
                                    ga if gains else None, gp, rc, io, vo, ro, co, pr, to if totals else None,
                                    fl if flag else None, ws if ws_addr is None else ctypes.c_void_p(ws_addr), need, None)


def test_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for kw in (dict(N=0), dict(N=1025), dict(k=0), dict(k=65), dict(S=0), dict(S=129), dict(S=-1), dict(m=-1),
               dict(nq=-1), dict(nq=2**31), dict(flag=False), dict(totals=False), dict(settings=False),
               dict(relevant=0), dict(nu=-1), dict(nu=2**31), dict(gains=False), dict(pools=False), dict(lists=False),
               dict(ws_addr=0x100004)):
        assert _grid(lib, **kw) == E, kw
    assert b"aligned" in lib.qrlsh_last_error()
    assert _grid(lib, m=(1 << 24) + 1, ws_bytes=1 << 40) == _lib.QRLSH_EUNSUPPORTED
    assert _grid(lib, ws_bytes=4 * 68 * 4 - 1) == _lib.QRLSH_EWORKSPACE
    assert b"workspace" in lib.qrlsh_last_error()
    # m = 0 returns at once; without a truth the scoring arguments are not looked at
    assert _grid(lib, m=0, pools=False, lists=False) == _lib.QRLSH_OK
    assert _grid(lib, m=0, truth=False, relevant=0, nu=-1, gains=False) == _lib.QRLSH_OK
    assert _grid(lib, m=0, S=129) == E


# ----------------------------------------------------------------------------------- host layer, before the library
@pytest.fixture()
def no_library(monkeypatch):
    from qrlsh import _lib

    def touched(*a, **kw):
        raise AssertionError("touched the library")
    monkeypatch.setattr(_lib, "load", touched)


def _pools():
    ci = np.array([[3, 1, 0, -1], [2, 4, -1, -1]], dtype=np.int32)
    cv = np.array([[9, 8, 7, 0], [5, 5, 0, 0]], dtype=np.int32)
    av = np.array([3, 2], dtype=np.int32)
    src, dst, mil = np.array([0, 0, 3]), np.array([1, 2, 4]), np.array([900, 100, 500])
    return ci, cv, av, src, dst, mil


def test_diversify_grid_rejects_bad_arguments_before_the_library(no_library):
    import qrlsh
    ci, cv, av, src, dst, mil = _pools()
    ok = [(0, 1001), (500, 900)]
    truth = np.ones((3, 7), dtype=np.int32)

    def call(*a, **kw):
        with pytest.raises(ValueError):
            qrlsh.diversify_grid(*a, **kw)
    for settings in ([], None, 5, [(0,)], [(0, 1001, 3)], [(-1, 1001)], [((1 << 20) + 1, 5)], [(0, 1002)], [(0, -1)],
                     [(0.5, 1001)], [(0, True)], ok + [(0, 2000)]):
        call(ci, cv, av, src, dst, mil, 7, 2, settings)
    for k in (0, 5, 1025, 2.5, True, None):
        call(ci, cv, av, src, dst, mil, 7, k, ok)
    for nq in (-1, 2**31, 7.0):
        call(ci, cv, av, src, dst, mil, nq, 2, ok)
    call(ci[0], cv[0], av, src, dst, mil, 7, 2, ok)
    call(ci, cv[:, :3], av, src, dst, mil, 7, 2, ok)
    call(ci, cv, av[:1], src, dst, mil, 7, 2, ok)
    call(ci.astype(np.float64), cv, av, src, dst, mil, 7, 2, ok)
    call(ci, cv, av, src, dst[:2], mil, 7, 2, ok)
    wide = np.zeros((1, 1025), dtype=np.int32)
    call(wide, wide, np.array([0]), src, dst, mil, 7, 2, ok)
    # the scoring arguments
    for kw in (dict(relevant=60), dict(users=[0, 1]), dict(gains=[2, 1]), dict(request_counts=np.zeros((2, 2), int))):
        call(ci, cv, av, src, dst, mil, 7, 2, ok, **kw)                       # no truth to hold them to
    for kw in (dict(), dict(relevant=0), dict(relevant=2.0), dict(relevant=2**31), dict(relevant=True),
               dict(relevant=60, gains=[3, 2, 1]), dict(relevant=60, gains=[2, -1]), dict(relevant=60, gains=[2.0, 1.0]),
               dict(relevant=60, gains=[2**62, 2**62]), dict(relevant=60, users=[0]), dict(relevant=60, users=[0, 3]),
               dict(relevant=60, users=[-1, 0]), dict(relevant=60, users=[[0, 1]]), dict(relevant=60, users=[0.0, 1.0]),
               dict(relevant=60, request_counts=np.zeros((2, 3), int)),
               dict(relevant=60, request_counts=np.zeros(2, int)),
               dict(relevant=60, request_counts=np.zeros((3, 2), int)),
               dict(relevant=60, request_counts=np.zeros((2, 2)))):
        call(ci, cv, av, src, dst, mil, 7, 2, ok, truth=truth, **kw)
    call(ci, cv, av, src, dst, mil, 7, 2, ok, truth=truth[:, :6], relevant=60)     # columns != nq
    call(ci, cv, av, src, dst, mil, 7, 2, ok, truth=truth[0], relevant=60)
    call(ci, cv, av, src, dst, mil, 7, 2, ok, truth=truth[:1], relevant=60)        # two requests, one row, no users
    call(ci, cv, av, src, dst, mil, 7, 2, ok, truth=truth.astype(np.float32), relevant=60)


def test_evaluate_diversity_rejects_bad_arguments_before_the_library(no_library):
    import qrlsh
    r = np.zeros((5, 7), dtype=np.int32)
    _, _, _, src, dst, mil = _pools()
    us = {0: {"indexes": np.array([1, 2]), "values": np.array([0.5, 0.25])}}
    ok = [(0, 1001)]
    for kw in (dict(k=0), dict(k=1025), dict(k=2.5), dict(k=3, pool=2), dict(k=3, pool=1025), dict(k=3, relevant=0),
               dict(k=3, settings=[]), dict(k=3, settings=[(0, 1002)]), dict(k=3, settings=[(-1, 5)]),
               dict(k=3, slices=257), dict(k=3, lo=2**31), dict(k=3, sum_order="kahan"), dict(k=3, users=[5]),
               dict(k=3, gains=[1, 2]), dict(k=3, gains=[3, 2, -1]), dict(k=3, truth=r[:4])):
        a = dict(k=3, relevant=60, settings=ok, truth=r)
        a.update(kw)
        with pytest.raises(ValueError):
            qrlsh.evaluate_diversity(r, a.pop("truth"), src, dst, mil, us, a.pop("k"), a.pop("relevant"),
                                     a.pop("settings"), **a)


def test_recommender_rejects_bad_arguments_before_the_library(no_library):
    import recommender
    from helpers import load
    rec = recommender.Recommender()
    rec.ratings = load("cfg2_scores")["ratings"]
    assert (rec.diversity_penalty, rec.diversity_max_sim) == (0, 1001)
    ok = [(0, 1001), (5000, 1001)]
    for kw in (dict(k=0), dict(k=1025), dict(pool=4), dict(pool=2000), dict(settings=[]), dict(settings=[(0, 1002)]),
               dict(fraction=-0.1), dict(fraction=1.5), dict(metric="rmse")):
        a = dict(k=5, relevant=60, settings=ok)
        a.update(kw)
        with pytest.raises(ValueError):
            rec.tune_diversity(a.pop("k"), a.pop("relevant"), a.pop("settings"), **a)
    with pytest.raises(ValueError, match="no live lists"):
        rec.tune_diversity(5, 60, ok)
    # a tuned pair is what recommend_users_diverse checks when called without one
    rec.diversity_penalty = -5
    with pytest.raises(ValueError, match="penalty"):
        rec.recommend_users_diverse([0], 5)
    rec.diversity_penalty, rec.diversity_max_sim = 0, 1002
    with pytest.raises(ValueError, match="max_sim"):
        rec.recommend_users_diverse([0], 5)
    with pytest.raises(ValueError, match="no live lists"):
        rec.recommend_users_diverse([0], 5, max_sim=1001)
    assert (type(rec).diversity_penalty, type(rec).diversity_max_sim) == (0, 1001)
