"""Ranking evaluation (qrlsh.evaluate_ranking, Recommender.evaluate_ranking): what needs no device.  The restatement
of tests/rank_eval_cases.py against a brute-force double loop; the default gain table; the ratios of RankingEvaluation;
every argument check of the host layer (before the library is loaded) and of the C ABI (fake pointers: each call fails a
check before anything is dereferenced)."""
import ctypes
import math

import numpy as np
import pytest

from helpers import load
import evaluate_cases as EC
import predict_cases as PC
import rank_eval_cases as RC


# ------------------------------------------------------------------------------------------------- the restatement
def brute_force(train, truth, qs, us, k, relevant, candidates, gains, summation):
    """One (user, column) double loop, no sort: the list is drawn by taking the best remaining candidate k times.  The
    predictions come from evaluate_cases.predict_unrated, the evaluation tests' own statement of the blend."""
    nu, nq = train.shape
    per, lists = [], []
    for u in range(nu):
        pred, test, rel = {}, 0, 0
        for j in range(nq):
            if train[u, j] != 0:
                continue
            is_test = truth[u, j] != 0
            test += is_test
            rel += is_test and truth[u, j] >= relevant
            if candidates == "heldout" and not is_test:
                continue
            p = EC.predict_unrated(train, qs, us, u, j, summation)[0]
            if p != 0:
                pred[j] = p
        avail, shown = len(pred), []
        while pred and len(shown) < k:
            best = max(pred.values())
            j = min(c for c in pred if pred[c] == best)
            shown.append((j, pred.pop(j)))
        hits = [p for p, (j, _) in enumerate(shown) if truth[u, j] >= relevant]
        per.append([len(shown), len(hits), sum(1 for j, _ in shown if truth[u, j] != 0), hits[0] + 1 if hits else 0,
                    sum(gains[p] for p in hits), int(rel), int(test), avail])
        lists.append(shown)
    return lists, np.array(per, dtype=np.int64)


@pytest.mark.parametrize("nu,nq,k", [(3, 7, 2), (3, 7, 7), (5, 40, 1), (5, 40, 6), (5, 40, 64)])
@pytest.mark.parametrize("candidates", ["all", "heldout"])
def test_restatement_equals_a_brute_force_double_loop(nu, nq, k, candidates):
    train, truth, _, qs, us = RC.split_case(nu * 100 + nq, nu, nq, fill=0.7, held=0.4, longest_q=4, ku=2)
    gains = RC.primes(k)
    for summation in (RC.O.np_sum_order, PC.sequential_sum):
        idx, val, avail, per, totals = RC.rank_eval_ref(train, truth, qs, us, None, k, 50, candidates, gains, summation)
        lists, want = brute_force(train, truth, qs, us, k, 50, candidates, gains, summation)
        assert np.array_equal(per, want)
        for u, shown in enumerate(lists):
            n = len(shown)
            assert idx[u, :n].tolist() == [j for j, _ in shown] and val[u, :n].tolist() == [v for _, v in shown]
            assert (idx[u, n:] == -1).all() and (val[u, n:] == 0).all() and avail[u] == want[u, 7]
        assert np.array_equal(totals[:8], want.sum(axis=0)) and totals[8] == nu
        assert totals[9] == (want[:, 5] > 0).sum() and totals[10] == (want[:, 1] > 0).sum()
        assert totals[11] == sum(sum(gains[:min(k, int(r))]) for r in want[:, 5]) and not totals[12:].any()
    assert want[:, 6].sum() > 0 and want[:, 1].sum() > 0         # the case has test cells, and lists that hit some
    # a request list with repeats: each request its user's line
    users = [nu - 1, 0, nu - 1]
    again = RC.rank_eval_ref(train, truth, qs, us, users, k, 50, candidates, gains, summation)
    assert np.array_equal(again[3], per[users]) and again[4][8] == 3


def test_cut_case_is_what_it_says():
    """the planted positions of rank_eval_cases.cut_case, read off the restatement"""
    for k in (1, 64):
        train, truth, _, qs, us, rows = RC.cut_case(k)
        got = RC.rank_eval_ref(train, truth, qs, us, None, k, RC.CUT_RELEVANT, "all", RC.primes(k))
        idx, val, avail, per, totals = got
        t = min(3, k)
        u = rows["ties"]
        assert avail[u] == k - t + 6 and (val[u, k - t:] == 20).all()
        inside = idx[u, k - t:]
        assert (np.diff(inside) > 0).all() and (truth[u, inside] >= RC.CUT_RELEVANT).sum() == min(t, 2)
        assert per[u, 5] == (truth[u] >= RC.CUT_RELEVANT).sum() - (train[u] >= RC.CUT_RELEVANT).sum() > per[u, 1]
        assert per[rows["short"]].tolist()[:4] == [min(k, 3), 1 if k >= 2 else 0, min(k, 3) - 1 if k >= 2 else 0,
                                                   2 if k >= 2 else 0]
        assert per[rows["nothing"]].tolist() == [0, 0, 0, 0, 0, 2, 2, 0]
        assert per[rows["no_relevant"], 5] == 0 and per[rows["no_relevant"], 0] == k
        assert per[rows["first"], 3] == 1 and per[rows["last"], 3] == k and per[rows["unlisted"], 3] == 0
        assert per[rows["unlisted"], 5] == 1 and per[rows["unlisted"], 1] == 0
        assert totals[9] == 6 and totals[10] == (4 if k >= 2 else 3)


# ------------------------------------------------------------------------------------------------- gains and ratios
def test_default_gains():
    import qrlsh
    g = qrlsh.dcg_gains(1024)
    assert g.dtype == np.int64 and g.shape == (1024,) and int(g[0]) == 2**32
    assert (np.diff(g) < 0).all() and g[-1] > 0
    assert g.tolist() == RC.dcg_gains_ref(1024)
    assert int(g[1]) == round(2**32 / math.log2(3)) and int(g[2]) == 2**31
    assert qrlsh.dcg_gains(1).tolist() == [2**32]
    for k in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            qrlsh.dcg_gains(k)


def test_ratios_from_hand_made_totals():
    import qrlsh
    t = np.zeros(16, dtype=np.int64)
    t[:12] = [200, 50, 80, 300, 7000, 125, 400, 99999, 20, 16, 12, 28000]
    ev = qrlsh.RankingEvaluation(t)
    assert ev.precision == 50 / 200 and ev.recall == 50 / 125 and ev.hit_rate == 12 / 16
    assert ev.ndcg == 7000 / 28000 and ev.known_share == 80 / 200 and ev.requests == 20
    assert ev.totals.dtype == np.int64 and np.array_equal(ev.totals, t) and "precision=0.2500" in repr(ev)
    # nothing listed, nobody with a relevant test cell: every ratio nan, none raises
    ev = qrlsh.RankingEvaluation(np.zeros(16, dtype=np.int64))
    assert all(math.isnan(x) for x in (ev.precision, ev.recall, ev.hit_rate, ev.ndcg, ev.known_share))
    # lists without any relevant test cell: precision 0, recall and ndcg nan
    t = np.zeros(16, dtype=np.int64)
    t[0], t[2], t[8] = 30, 4, 3
    ev = qrlsh.RankingEvaluation(t)
    assert ev.precision == 0.0 and ev.known_share == 4 / 30
    assert math.isnan(ev.recall) and math.isnan(ev.ndcg) and math.isnan(ev.hit_rate)
    # numbers past 2^53 stay exact in the integer division's operands
    t = np.zeros(16, dtype=np.int64)
    t[4], t[11] = 2**62, 2**62
    assert qrlsh.RankingEvaluation(t).ndcg == 1.0


def test_macro_from_hand_made_lines():
    import torch
    import qrlsh
    gains = [8, 4, 2, 1]
    prefix = torch.tensor([0, 8, 12, 14, 15])
    per = np.array([[4, 2, 3, 2, 6, 3, 5, 9],        # precision 1/2, recall 2/3, ndcg 6/14, rr 1/2
                    [0, 0, 0, 0, 0, 2, 2, 0],        # nothing listed: 0, 0, 0, 0
                    [4, 0, 1, 0, 0, 0, 3, 7],        # no relevant test cell: not counted
                    [1, 1, 1, 1, 8, 9, 9, 1],        # ideal = all four gains
                    [0, 0, 0, 0, 0, 0, 0, -1]], dtype=np.int64)
    ev = qrlsh.RankingEvaluation(np.zeros(16, dtype=np.int64), per_user=torch.from_numpy(per), gain_prefix=prefix)
    got, want = ev.macro(), RC.macro_ref(per, gains)
    assert got["n"] == want["n"] == 3
    assert want["precision"] == (0.5 + 0 + 1) / 3 and want["mrr"] == (0.5 + 0 + 1) / 3
    for name in ("precision", "recall", "ndcg", "mrr"):
        assert np.isclose(got[name], want[name], rtol=1e-12, atol=0), name
    none = qrlsh.RankingEvaluation(np.zeros(16, dtype=np.int64), per_user=torch.from_numpy(per[2:3]), gain_prefix=prefix)
    assert none.macro()["n"] == 0 and math.isnan(none.macro()["ndcg"])


# ----------------------------------------------------------------------------------- host layer, before the library
@pytest.fixture()
def no_library(monkeypatch):
    from qrlsh import _lib

    def touched(*a, **kw):
        raise AssertionError("touched the library")
    monkeypatch.setattr(_lib, "load", touched)


def _small():
    import torch
    truth = np.arange(35, dtype=np.int32).reshape(5, 7) % 4 * 30
    train = np.where(np.arange(35).reshape(5, 7) % 3 == 0, 0, truth).astype(np.int32)
    src = torch.tensor([0, 0, 3], dtype=torch.int32)
    dst = torch.tensor([1, 2, 4], dtype=torch.int32)
    mil = torch.tensor([900, 100, 500], dtype=torch.int32)
    us = {0: {"indexes": np.array([1, 2]), "values": np.array([0.5, 0.25])}}
    return train, truth, src, dst, mil, us


def test_evaluate_ranking_rejects_bad_arguments_before_the_library(no_library):
    import torch
    import qrlsh
    train, truth, src, dst, mil, us = _small()

    def call(k=3, relevant=50, train=train, truth=truth, us=us, **kw):
        return qrlsh.evaluate_ranking(train, truth, src, dst, mil, us, k, relevant, **kw)
    for k in (0, 1025, -3, 2.5, True, "3", None):
        with pytest.raises(ValueError, match="k must"):
            call(k=k)
    for relevant in (0, -1, 2**31, 1.5, True, None):
        with pytest.raises(ValueError, match="relevant"):
            call(relevant=relevant)
    for candidates in ("rated", "ALL", None, 0):
        with pytest.raises(ValueError, match="candidates"):
            call(candidates=candidates)
    for gains in ([5, 4], [5, 4, 3, 2], [5, -1, 3], [5.0, 4.0, 3.0], [[5, 4, 3]], torch.tensor([5, 4, -3])):
        with pytest.raises(ValueError, match="gains"):
            call(gains=gains)
    with pytest.raises(ValueError, match="int64"):
        call(gains=[2**62, 2**61, 5])                     # 5 requests x the sum >= 2^63
    with pytest.raises(ValueError, match="int64"):
        call(gains=[2**62 // 5 * 2] * 3, users=[0, 1, 2, 3, 4, 0, 1, 2])
    for slices in (-1, 257, 1.5, True):
        with pytest.raises(ValueError, match="slices"):
            call(slices=slices)
    for lo in (2**31, -2**31 - 1, 0.5):
        with pytest.raises(ValueError, match="lo must"):
            call(lo=lo)
    with pytest.raises(ValueError, match="sum_order"):
        call(sum_order="kahan")
    for other in (truth[:4], truth[:, :6], truth[0], truth.astype(np.float64)):
        with pytest.raises(ValueError, match="truth"):
            call(truth=other)
    with pytest.raises(ValueError):
        call(train=train.astype(np.float32))
    for users in ([5], [-1], [0, 1, 99], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="user"):
            call(users=users)
    with pytest.raises(ValueError, match="neighbours"):
        call(us={1: {"indexes": np.arange(65) % 5, "values": np.full(65, 0.5)}})


def test_recommender_evaluate_ranking_rejects_bad_arguments_before_the_library(no_library):
    import recommender
    g = load("cfg2_scores")
    rec = recommender.Recommender()
    rec.ratings = g["ratings"]
    with pytest.raises(ValueError, match="k must"):
        rec.evaluate_ranking(0, 50)
    with pytest.raises(ValueError, match="relevant"):
        rec.evaluate_ranking(5, 0)
    with pytest.raises(ValueError, match="candidates"):
        rec.evaluate_ranking(5, 50, candidates="some")
    with pytest.raises(ValueError, match="fraction"):
        rec.evaluate_ranking(5, 50, fraction=1.5)
    with pytest.raises(ValueError, match="no live lists"):
        rec.evaluate_ranking(5, 50)                       # no run yet


# ---------------------------------------------------------------------------------------------- C ABI, no device
MAX_GROUPS = 1 << 24


def _fake(n):
    """distinct, 16-byte-aligned non-null addresses; the argument checks return before anything is dereferenced"""
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def _rank(lib, nu=4, nq=100000, ku=8, sum_order=0, users=True, m=4, k=10, relevant=50, candidates=0, lo=0, slices=1,
          outs=True, per=True, totals=True, flags=True, gains=True, ws_bytes=None, ws_addr=None, lists=True, truth=True):
    tr, tt, qo, qi, qm, ui, uv, us, g, gp, io, vo, ao, po, to, fl, ws = _fake(17)
    need = lib.qrlsh_evaluate_ranking_workspace_bytes(m, nq, k, slices) if ws_bytes is None else ws_bytes
    return lib.qrlsh_evaluate_ranking(tr, tt if truth else None, nu, nq, qo if lists else None, qi, qm, ui, uv, ku, 0.6,
                                      0.4, 60.0, sum_order, us if users else None, m, k, relevant, candidates, lo, slices,
                                      g if gains else None, gp if gains else None, io if outs else None,
                                      vo if outs else None, ao if outs else None, po if per else None,
                                      to if totals else None, fl if flags else None,
                                      ws if ws_addr is None else ctypes.c_void_p(ws_addr), need, None)


def test_evaluate_ranking_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for k in (0, 1025, -1):
        assert _rank(lib, k=k) == E
        assert b"k=" in lib.qrlsh_last_error()
    for ku in (65, -1):
        assert _rank(lib, ku=ku) == E
        assert b"ku=" in lib.qrlsh_last_error()
    for bad in (dict(nq=2**31), dict(nq=-1), dict(nu=-2), dict(m=-1)):
        assert _rank(lib, **bad) == E
    for so in (2, -1):
        assert _rank(lib, sum_order=so) == E
        assert b"sum_order" in lib.qrlsh_last_error()
    for relevant in (0, -5):
        assert _rank(lib, relevant=relevant) == E
        assert b"relevant=" in lib.qrlsh_last_error()
    for candidates in (2, -1):
        assert _rank(lib, candidates=candidates) == E
        assert b"candidates" in lib.qrlsh_last_error()
    for slices in (257, -1):
        assert _rank(lib, slices=slices) == E
        assert b"slices=" in lib.qrlsh_last_error()
    assert _rank(lib, users=False, m=3, nu=4) == E
    for hole in ("outs", "per"):
        assert _rank(lib, **{hole: False}) == E
        assert b"null output" in lib.qrlsh_last_error()
    for hole in ("totals", "flags"):
        assert _rank(lib, **{hole: False}) == E
        assert b"required" in lib.qrlsh_last_error()
    assert _rank(lib, gains=False) == E
    assert b"gain" in lib.qrlsh_last_error()
    for hole in ("lists", "truth"):
        assert _rank(lib, **{hole: False}) == E
        assert b"null pointer" in lib.qrlsh_last_error()
    assert _rank(lib, m=MAX_GROUPS // 256 + 1, slices=256) == _lib.QRLSH_EUNSUPPORTED
    assert b"workgroups" in lib.qrlsh_last_error()
    need = lib.qrlsh_evaluate_ranking_workspace_bytes(4, 100000, 10, 1)
    assert _rank(lib, ws_bytes=need - 1) == _lib.QRLSH_EWORKSPACE
    assert b"workspace" in lib.qrlsh_last_error()
    assert _rank(lib, ws_addr=0x100004) == E
    assert b"aligned" in lib.qrlsh_last_error()


def test_evaluate_ranking_workspace_bytes():
    from qrlsh import _lib
    lib = _lib.load()
    w, served = lib.qrlsh_evaluate_ranking_workspace_bytes, lib.qrlsh_recommend_users_workspace_bytes
    for args in ((4, 100000, 10, 1), (7, 5003, 28, 3), (1, 1, 1, 0), (37, 8192, 64, 1), (2000, 100000, 100, 0)):
        assert w(*args) % 256 == 0
        # the compact rows and the selection's own, plus two int64 per (request, sweep slice): at most one per 1024 columns
        extra = w(*args) - served(*args)
        assert 16 * args[0] <= extra <= 16 * args[0] * ((args[1] + 1023) // 1024) + 256, args
    assert w(4, 100000, 10, 3) - served(4, 100000, 10, 3) == 256         # 4 x 3 x 16 bytes, rounded
    assert w(0, 100, 10, 1) == 0 and w(4, 0, 10, 1) == 0
    assert w(4, 100, 0, 1) == 0 and w(4, 100, 1025, 1) == 0 and w(4, 100, 10, 257) == 0 and w(4, 100, 10, -1) == 0
    assert w(MAX_GROUPS // 256 + 1, 100000, 10, 256) == 0
