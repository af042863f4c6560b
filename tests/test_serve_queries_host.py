"""Serving chosen queries (qrlsh_predict_queries / qrlsh_recommend_queries, qrlsh.predict_queries / for_queries /
query_utility, Recommender.recommend_queries / predict_queries / query_utility): what needs no device.  The
restatements of serve_queries_cases.py on the golden score sets in both sum orders; every argument check of the C ABI
(fake pointers: each call fails a check before anything is dereferenced) and of the host layer (before the library is
loaded); QueryUtility's divisions; the header declares no new size export."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
import serve_queries_cases as SQ
from test_recommend_host import SCORES, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_M = 1 << 24


# ------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("name", SCORES)
def test_restatements_on_golden_in_both_orders(name):
    ratings, golden_final, qs, us = SQ.golden_case(name)
    nu, nq = ratings.shape
    queries = [0, nq - 1, nq // 2, 3, nq - 1]
    for order, summation in SQ.ORDERS.items():
        final = golden_final if order == "pairwise" else O.predict_scores(ratings, qs, us, summation=summation)
        cols = SQ.restate_columns(final, queries)
        assert cols.shape == (len(queries), nu)
        # the column, cell by cell from the oracle
        for x, j in enumerate(queries):
            cells = np.stack([np.arange(nu), np.full(nu, j)], axis=1)
            assert np.array_equal(cols[x], O.predict_cells(ratings, qs, us, cells, summation=summation)), (order, j)
        # the top-k users: the two-step contract over the transposes, ordered by value then user
        for k in (1, 5, 1024):
            users, val, avail = SQ.restate_top_users(ratings, final, queries, k)
            want = restate(np.ascontiguousarray(ratings.T), np.ascontiguousarray(final.T), k, users=queries)
            for a, b in zip((users, val, avail), want):
                assert np.array_equal(a, b)
            for x in range(len(queries)):
                n = min(k, int(avail[x]))
                assert np.all(users[x, n:] == -1) and np.all(val[x, n:] == 0)
                for a in range(n - 1):
                    assert val[x, a] > val[x, a + 1] or (val[x, a] == val[x, a + 1] and users[x, a] < users[x, a + 1])
                assert np.all(ratings[users[x, :n], queries[x]] == 0)
        assert (SQ.restate_top_users(ratings, final, queries, 5)[2] > 0).any()
        # the words: every user is counted once; a prediction needs a side, and with ratings >= 1 a side gives one
        words = SQ.restate_words(ratings, final, qs, us, queries, summation)
        assert np.array_equal(words[:, 0] + words[:, 2] + words[:, 4], np.full(len(queries), nu))
        assert np.array_equal(words[:, 2], words[:, 5:].sum(axis=1)) and ratings.min() >= 0
        assert np.array_equal(words[1], words[4]) and words[:, 5:].sum() > 0
        assert np.array_equal(words[:, 1], ratings[:, queries].sum(axis=0))
        assert np.array_equal(words[:, 3], (cols * (ratings[:, queries].T == 0)).sum(axis=1))


def test_knife_and_mixed_cases_hold_what_they_promise():
    c, queries, finals = SQ.knife_case()
    assert sorted(set(queries)) != queries and c.spare in queries
    w = {o: SQ.restate_words(c.ratings, finals[o], c.qs, c.us, queries, s) for o, s in SQ.ORDERS.items()}
    assert (w["pairwise"][:, 3] != w["sequential"][:, 3]).any()     # the orders part in the sums of the predictions
    assert all((w[o][:, 5:] > 0).any(axis=0).all() for o in w)       # every branch occurs
    c2, q2 = SQ.mixed_forms_case()
    assert c2.nu == 2000 and len(set(q2)) < len(q2)


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    """distinct, 16-byte-aligned non-null addresses; the argument checks return before anything is dereferenced"""
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def _predict(lib, nu=2000, nq=100, ku=8, sum_order=0, queries=True, m=4, out=True, cols=True, util=True, flags=True,
             lists=True, ratings=True, ulists=True):
    r, qo, qi, qm, ui, uv, qs, o, ct, ut, fl = _fake(11)
    return lib.qrlsh_predict_queries(r if ratings else None, nu, nq, qo if lists else None, qi, qm,
                                     ui if ulists else None, uv if ulists else None, ku, 0.6, 0.4, 60.0, sum_order,
                                     qs if queries else None, m, o if out else None, ct if cols else None,
                                     ut if util else None, fl if flags else None, None)


def _recommend(lib, nu=100000, nq=100, ku=8, sum_order=0, queries=True, m=4, k=10, lo=0, slices=1, outs=True,
               flags=True, cols=True, ws_bytes=None, ws_addr=None, lists=True):
    r, qo, qi, qm, ui, uv, qs, io, vo, ao, ut, fl, ct, ws = _fake(14)
    need = lib.qrlsh_recommend_users_workspace_bytes(m, nu, k, slices) if ws_bytes is None else ws_bytes
    return lib.qrlsh_recommend_queries(r, nu, nq, qo if lists else None, qi, qm, ui, uv, ku, 0.6, 0.4, 60.0, sum_order,
                                       qs if queries else None, m, k, lo, slices, io if outs else None,
                                       vo if outs else None, ao if outs else None, ut, fl if flags else None,
                                       ct if cols else None, ws if ws_addr is None else ctypes.c_void_p(ws_addr), need,
                                       None)


def test_predict_queries_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for ku in (65, -1):
        assert _predict(lib, ku=ku) == E
        assert b"ku=" in lib.qrlsh_last_error()
    for so in (2, -1):
        assert _predict(lib, sum_order=so) == E
        assert b"sum_order" in lib.qrlsh_last_error()
    assert _predict(lib, nq=2**31) == E
    assert _predict(lib, nu=2**31) == E
    assert _predict(lib, nq=-1) == E and _predict(lib, nu=-1) == E and _predict(lib, m=-1) == E
    assert _predict(lib, queries=False, m=99, nq=100) == E            # queries == NULL: m must be nq
    assert b"must equal nq" in lib.qrlsh_last_error()
    assert _predict(lib, cols=False) == E
    assert b"cols_tmp" in lib.qrlsh_last_error()
    assert _predict(lib, flags=False) == E
    assert b"flags_out" in lib.qrlsh_last_error()
    for hole in ("lists", "ratings", "ulists"):
        assert _predict(lib, **{hole: False}) == E
        assert b"null pointer" in lib.qrlsh_last_error()
    assert _predict(lib, m=MAX_M + 1) == _lib.QRLSH_EUNSUPPORTED
    with pytest.raises(NotImplementedError):
        _lib.check(_predict(lib, m=MAX_M + 1))
    with pytest.raises(_lib.QrlshError):
        _lib.check(_predict(lib, ku=65))
    # m = 0: nothing to do, whatever else is null
    fl = _fake(1)[0]
    assert lib.qrlsh_predict_queries(None, 4, 10, None, None, None, None, None, 0, 0.6, 0.4, 60.0, 0, fl, 0, None, None,
                                     None, fl, None) == _lib.QRLSH_OK


def test_recommend_queries_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for k in (0, 1025, -1):
        assert _recommend(lib, k=k) == E
        assert b"k=" in lib.qrlsh_last_error()
    for ku in (65, -1):
        assert _recommend(lib, ku=ku) == E
        assert b"ku=" in lib.qrlsh_last_error()
    for so in (2, -1):
        assert _recommend(lib, sum_order=so) == E
        assert b"sum_order" in lib.qrlsh_last_error()
    for slices in (257, -1):
        assert _recommend(lib, slices=slices) == E
        assert b"slices=" in lib.qrlsh_last_error()
    assert _recommend(lib, nq=2**31) == E and _recommend(lib, nu=2**31) == E
    assert _recommend(lib, nq=-1) == E and _recommend(lib, nu=-1) == E and _recommend(lib, m=-1) == E
    assert _recommend(lib, queries=False, m=99, nq=100) == E
    assert b"must equal nq" in lib.qrlsh_last_error()
    assert _recommend(lib, cols=False) == E
    assert b"cols_tmp" in lib.qrlsh_last_error()
    assert _recommend(lib, flags=False) == E
    assert b"flags_out" in lib.qrlsh_last_error()
    assert _recommend(lib, outs=False) == E
    assert b"null output" in lib.qrlsh_last_error()
    assert _recommend(lib, lists=False) == E
    assert b"null pointer" in lib.qrlsh_last_error()
    # the two limits: m alone, and m x slices workgroups of the selection
    assert _recommend(lib, m=MAX_M + 1, nu=64, slices=0) == _lib.QRLSH_EUNSUPPORTED
    assert _recommend(lib, m=MAX_M // 256 + 1, slices=256) == _lib.QRLSH_EUNSUPPORTED
    assert b"workgroups" in lib.qrlsh_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(_recommend(lib, m=MAX_M // 256 + 1, slices=256))
    # the workspace is qrlsh_recommend_users_workspace_bytes(m, nu, k, slices): short by one byte, and misaligned
    need = lib.qrlsh_recommend_users_workspace_bytes(4, 100000, 10, 1)
    assert need >= 4 * 100000 * 4
    assert _recommend(lib, ws_bytes=need - 1) == _lib.QRLSH_EWORKSPACE
    assert b"workspace" in lib.qrlsh_last_error()
    assert _recommend(lib, ws_addr=0x100004) == E
    assert b"aligned" in lib.qrlsh_last_error()
    # the rows form (nu <= 2048) needs its compact columns too
    assert _recommend(lib, nu=64, slices=0, ws_bytes=lib.qrlsh_recommend_users_workspace_bytes(4, 64, 10, 0) - 1) \
        == _lib.QRLSH_EWORKSPACE
    fl = _fake(1)[0]
    assert lib.qrlsh_recommend_queries(None, 4, 10, None, None, None, None, None, 0, 0.6, 0.4, 60.0, 0, fl, 0, 5, 0, 0,
                                       None, None, None, None, fl, None, None, 0, None) == _lib.QRLSH_OK


# ----------------------------------------------------------------------------------- host layer, before the library
@pytest.fixture()
def no_library(monkeypatch):
    from qrlsh import _lib

    def touched(*a, **kw):
        raise AssertionError("touched the library")
    monkeypatch.setattr(_lib, "load", touched)


def _small():
    import torch
    r = np.zeros((5, 7), dtype=np.int32)
    src = torch.tensor([0, 0, 3], dtype=torch.int32)
    dst = torch.tensor([1, 2, 4], dtype=torch.int32)
    mil = torch.tensor([900, 100, 500], dtype=torch.int32)
    us = {0: {"indexes": np.array([1, 2]), "values": np.array([0.5, 0.25])}}
    return r, src, dst, mil, us


def test_host_layer_rejects_bad_arguments_before_the_library(no_library):
    import torch
    import qrlsh
    r, src, dst, mil, us = _small()
    for k in (0, 1025, -3, 2.5, True, "3", None):
        with pytest.raises(ValueError):
            qrlsh.for_queries(r, src, dst, mil, us, [0], k)
    for slices in (-1, 257, 1.5, True):
        with pytest.raises(ValueError):
            qrlsh.for_queries(r, src, dst, mil, us, [0], 3, slices=slices)
    for lo in (2**31, -2**31 - 1, 0.5):
        with pytest.raises(ValueError):
            qrlsh.for_queries(r, src, dst, mil, us, [0], 3, lo=lo)
    calls = (lambda *a, **kw: qrlsh.for_queries(*a, 3, **kw), qrlsh.predict_queries, qrlsh.query_utility)
    for call in calls:
        with pytest.raises(ValueError):
            call(r, src, dst, mil, us, [0], sum_order="kahan")
        with pytest.raises(ValueError):
            call(r[0], src, dst, mil, us, [0])                                   # not 2-D
        with pytest.raises(ValueError):
            call(r.astype(np.float64), src, dst, mil, us, [0])                   # not integers
        with pytest.raises(ValueError):
            call(r, src, dst[:2], mil, us, [0])                                  # lists differ in length
        # host ids are range-checked against nq (7), not nu (5), before anything is uploaded
        for queries in ([7], [-1], [0, 1, 99], [2**40], [[0, 1]], [0.5], torch.tensor([0.5]), torch.tensor([[0]])):
            with pytest.raises(ValueError):
                call(r, src, dst, mil, us, queries)
        with pytest.raises(ValueError, match=r"query id outside \[0, 7\)"):
            call(r, src, dst, mil, us, [6, 7])
        long_list = {1: {"indexes": np.arange(65) % 5, "values": np.full(65, 0.5)}}
        with pytest.raises(ValueError):
            call(r, src, dst, mil, long_list, [0])
    # ids 5 and 6 are columns, not rows: accepted by the checks (the library is what stops this call)
    with pytest.raises(AssertionError, match="touched the library"):
        qrlsh.predict_queries(r, src, dst, mil, us, [5, 6])
    # and the user entry points still check against nu
    with pytest.raises(ValueError, match=r"user id outside \[0, 5\)"):
        qrlsh.predict_users(r, src, dst, mil, us, [5])


def test_recommender_rejects_bad_arguments_before_the_library(no_library):
    import recommender
    from helpers import load
    g = load("cfg2_scores")
    rec = recommender.Recommender()
    rec.ratings = g["ratings"]

    def no_similarities():
        raise AssertionError("computed user similarities")
    rec.compute_userSimilarities = no_similarities
    for k in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            rec.recommend_queries([0], k)
    for call in (lambda: rec.recommend_queries([0], 5), lambda: rec.predict_queries([0]), rec.query_utility):
        with pytest.raises(ValueError, match="no live lists"):
            call()                                          # no run yet


# --------------------------------------------------------------------------------------------------- QueryUtility
def test_query_utility_divisions():
    import qrlsh
    words = np.array([[4, 200, 6, 330, 10, 1, 2, 3],       # ordinary
                      [0, 0, 0, 0, 20, 0, 0, 0],           # nobody rated it, nobody gets a prediction
                      [20, 900, 0, 0, 0, 0, 0, 0],         # fully rated
                      [0, 0, 5, 250, 0, 5, 0, 0]], dtype=np.int64)
    u = qrlsh.QueryUtility(words)
    assert u.words.dtype == np.int64 and u.words.shape == (4, 8)
    assert u.rated.tolist() == [4, 0, 20, 0] and u.predicted.tolist() == [6, 0, 0, 5] and u.missed.tolist() == [10, 20, 0, 0]
    assert u.utility.dtype == np.float64
    assert u.utility[0] == 530 / 10 and math.isnan(u.utility[1]) and u.utility[2] == 45.0 and u.utility[3] == 50.0
    assert u.mean_rating[0] == 50.0 and math.isnan(u.mean_rating[1]) and math.isnan(u.mean_rating[3])
    assert u.mean_prediction[0] == 55.0 and math.isnan(u.mean_prediction[2]) and u.mean_prediction[3] == 50.0
    assert u.coverage[0] == 1 - 10 / 16 and u.coverage[1] == 0.0 and math.isnan(u.coverage[2]) and u.coverage[3] == 1.0
    assert {k: v.tolist() for k, v in u.by_branch.items()} == {"query": [1, 0, 0, 5], "user": [2, 0, 0, 0],
                                                              "both": [3, 0, 0, 0]}
    empty = qrlsh.QueryUtility(np.zeros((0, 8), dtype=np.int64))
    assert empty.utility.shape == (0,) and empty.words.shape == (0, 8)


# ------------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_two_calls_and_no_new_size_export():
    spec = importlib.util.spec_from_file_location("workspace_sizes", os.path.join(ROOT, "tools", "workspace_sizes.py"))
    ws = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ws)
    text = re.sub(r"/\*.*?\*/", " ", open(ws.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(qrlsh_\w*queries\w*)\s*\(", text))
    assert declared == {"qrlsh_predict_queries", "qrlsh_recommend_queries"}
    assert not any(ws.SIZE_EXPORT.match(n) for n in declared)
    import json
    recorded = [e["fn"] for e in json.load(open(ws.GOLDEN))]
    assert [n for n, _ in ws.size_exports()] == recorded
    from qrlsh import _lib
    assert declared <= set(_lib.SIGNATURES)
