"""Serving chosen users (qrlsh_predict_users / qrlsh_recommend_users, qrlsh.predict_users / for_users,
Recommender.recommend_users): what needs no device.  The restatement the GPU tests hold the device to -- the oracle's
predict_cells over the requested rows, then test_recommend_host.restate -- checked on the golden score sets; every
argument check of the C ABI (fake pointers: each call fails a check before anything is dereferenced) and of the host
layer (before the library is loaded); the workspace sizes; predict.user_lists' padding."""
import ctypes

import numpy as np
import pytest

from helpers import load
from oracle import oracle as O
import predict_cases as PC
from test_recommend_host import SCORES, restate

MAX_GROUPS = 1 << 24


# ------------------------------------------------------------------------------------------------- the restatement
def oracle_rows(ratings, qs, us, users, summation=O.np_sum_order, **weights):
    """the completed rows of `users` (repeats allowed): predict_cells over every cell of each distinct row"""
    ratings = np.asarray(ratings)
    nq = ratings.shape[1]
    distinct = sorted(set(int(u) for u in users))
    cells = np.stack([np.repeat(distinct, nq), np.tile(np.arange(nq), len(distinct))], axis=1)
    rows = O.predict_cells(ratings, qs, us, cells, summation=summation, **weights).reshape(len(distinct), nq)
    return rows[[distinct.index(int(u)) for u in users]]


def restate_users(ratings, rows, users, k):
    """restate() over the requested rows alone: row x of `rows` belongs to users[x]"""
    return restate(np.asarray(ratings)[np.asarray(users, dtype=np.int64)], rows, k)


def golden_lists(name):
    g, h = load(name), load(name.replace("_scores", "_hotpath"))
    qs = {int(q): {"indexes": h["qs_idx"][h["qs_off"][n]:h["qs_off"][n + 1]].astype(np.int64),
                   "values": h["qs_val"][h["qs_off"][n]:h["qs_off"][n + 1]]} for n, q in enumerate(h["qs_q"])}
    us = {}
    for u in range(len(g["ratings"])):
        n = int((g["us_idx"][u] >= 0).sum())
        us[u] = {"indexes": g["us_idx"][u][:n].astype(np.int64), "values": g["us_val"][u][:n]}
    return g, qs, us


@pytest.mark.parametrize("name", SCORES)
def test_restatement_equals_the_two_step_contract_on_golden(name):
    g, qs, us = golden_lists(name)
    ratings, final = g["ratings"], g["final"]
    nu = ratings.shape[0]
    users = [0, nu - 1, nu // 2, 3, nu - 1]
    rows = oracle_rows(ratings, qs, us, users)
    assert np.array_equal(rows, final[users])
    for k in (1, 5, 1024):
        got = restate_users(ratings, rows, users, k)
        want = restate(ratings, final, k, users=users)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert (got[2] > 0).any()


def test_restatement_orders_differ_on_a_knife_case():
    c = PC.build_case(7, nu=160, nq=400, tu=6, tq=12)
    users = [0, 5, 0]
    pw = oracle_rows(c.ratings, c.qs, c.us, users)
    sq = oracle_rows(c.ratings, c.qs, c.us, users, summation=PC.sequential_sum)
    assert np.array_equal(pw[0], pw[2]) and pw.shape == (3, 400)
    assert np.array_equal(pw, O.predict_scores(c.ratings, c.qs, c.us)[users])
    assert (pw != sq).any()


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    """distinct, 16-byte-aligned non-null addresses; the argument checks return before anything is dereferenced"""
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def _predict(lib, nu=4, nq=100000, ku=8, sum_order=0, users=True, m=4, out=True, flags=True, lists=True, ratings=True,
             ulists=True):
    r, qo, qi, qm, ui, uv, us, o, fl = _fake(9)
    return lib.qrlsh_predict_users(r if ratings else None, nu, nq, qo if lists else None, qi, qm,
                                   ui if ulists else None, uv if ulists else None, ku, 0.6, 0.4, 60.0, sum_order,
                                   us if users else None, m, o if out else None, fl if flags else None, None, 0, None)


def _recommend(lib, nu=4, nq=100000, ku=8, sum_order=0, users=True, m=4, k=10, lo=0, slices=1, outs=True, flags=True,
               ws_bytes=None, ws_addr=None, lists=True):
    r, qo, qi, qm, ui, uv, us, io, vo, ao, fl, ws = _fake(12)
    need = lib.qrlsh_recommend_users_workspace_bytes(m, nq, k, slices) if ws_bytes is None else ws_bytes
    return lib.qrlsh_recommend_users(r, nu, nq, qo if lists else None, qi, qm, ui, uv, ku, 0.6, 0.4, 60.0, sum_order,
                                     us if users else None, m, k, lo, slices, io if outs else None,
                                     vo if outs else None, ao if outs else None, fl if flags else None,
                                     ws if ws_addr is None else ctypes.c_void_p(ws_addr), need, None)


def test_predict_users_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for ku in (65, -1):
        assert _predict(lib, ku=ku) == E
        assert b"ku=" in lib.qrlsh_last_error()
    assert _predict(lib, nq=2**31) == E
    assert _predict(lib, nq=-1) == E
    assert _predict(lib, nu=-1) == E
    assert _predict(lib, m=-1) == E
    for so in (2, -1):
        assert _predict(lib, sum_order=so) == E
        assert b"sum_order" in lib.qrlsh_last_error()
    assert _predict(lib, users=False, m=3, nu=4) == E            # no user list: m must be nu
    assert _predict(lib, flags=False) == E
    assert b"flags_out" in lib.qrlsh_last_error()
    for hole in ("out", "lists", "ratings", "ulists"):
        assert _predict(lib, **{hole: False}) == E
        assert b"null pointer" in lib.qrlsh_last_error()
    assert _predict(lib, m=MAX_GROUPS + 1) == _lib.QRLSH_EUNSUPPORTED
    # m = 0: nothing to do, whatever else is null
    fl = _fake(1)[0]
    assert lib.qrlsh_predict_users(None, 4, 10, None, None, None, None, None, 0, 0.6, 0.4, 60.0, 0, fl, 0, None, fl,
                                   None, 0, None) == _lib.QRLSH_OK
    with pytest.raises(_lib.QrlshError):
        _lib.check(_predict(lib, ku=65))
    with pytest.raises(NotImplementedError):
        _lib.check(_predict(lib, m=MAX_GROUPS + 1))


def test_recommend_users_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for k in (0, 1025, -1):
        assert _recommend(lib, k=k) == E
        assert b"k=" in lib.qrlsh_last_error()
    for ku in (65, -1):
        assert _recommend(lib, ku=ku) == E
        assert b"ku=" in lib.qrlsh_last_error()
    assert _recommend(lib, nq=2**31) == E
    assert _recommend(lib, nq=-1) == E
    assert _recommend(lib, nu=-2) == E
    assert _recommend(lib, m=-1) == E
    for so in (2, -1):
        assert _recommend(lib, sum_order=so) == E
        assert b"sum_order" in lib.qrlsh_last_error()
    for slices in (257, -1):
        assert _recommend(lib, slices=slices) == E
        assert b"slices=" in lib.qrlsh_last_error()
    assert _recommend(lib, users=False, m=3, nu=4) == E
    assert _recommend(lib, outs=False) == E
    assert b"null output" in lib.qrlsh_last_error()
    assert _recommend(lib, flags=False) == E
    assert b"flags_out" in lib.qrlsh_last_error()
    assert _recommend(lib, lists=False) == E
    assert b"null pointer" in lib.qrlsh_last_error()
    # m x max(slices, 1) workgroups: the rows form counts one per row, the slice form `slices`
    assert _recommend(lib, m=MAX_GROUPS // 256 + 1, slices=256) == _lib.QRLSH_EUNSUPPORTED
    assert _recommend(lib, m=MAX_GROUPS + 1, nq=64, slices=0) == _lib.QRLSH_EUNSUPPORTED
    assert b"workgroups" in lib.qrlsh_last_error()
    need = lib.qrlsh_recommend_users_workspace_bytes(4, 100000, 10, 1)
    assert _recommend(lib, ws_bytes=need - 1) == _lib.QRLSH_EWORKSPACE
    assert b"workspace" in lib.qrlsh_last_error()
    assert _recommend(lib, ws_addr=0x100004) == E
    assert b"aligned" in lib.qrlsh_last_error()
    # the rows form needs its compact rows too
    assert _recommend(lib, nq=64, slices=0, ws_bytes=lib.qrlsh_recommend_users_workspace_bytes(4, 64, 10, 0) - 1) \
        == _lib.QRLSH_EWORKSPACE
    fl = _fake(1)[0]
    assert lib.qrlsh_recommend_users(None, 4, 10, None, None, None, None, None, 0, 0.6, 0.4, 60.0, 0, fl, 0, 5, 0, 0,
                                     None, None, None, fl, None, 0, None) == _lib.QRLSH_OK
    with pytest.raises(NotImplementedError):
        _lib.check(_recommend(lib, m=MAX_GROUPS // 256 + 1, slices=256))


def test_workspace_bytes():
    from qrlsh import _lib
    lib = _lib.load()
    assert lib.qrlsh_predict_users_workspace_bytes(16, 100000) == 0
    assert lib.qrlsh_predict_users_workspace_bytes(0, 0) == 0
    w = lib.qrlsh_recommend_users_workspace_bytes
    sel = lib.qrlsh_recommend_workspace_bytes
    base = w(4, 100000, 10, 1)
    assert base >= 4 * 100000 * 4 + sel(4, 100000, 10, 1)          # the compact rows and the selection's own
    assert w(8, 100000, 10, 1) > base and w(4, 100001, 10, 1) > base   # grows with m and nq
    assert w(4, 100000, 10, 2) > base and w(4, 100000, 1024, 1) > base   # with slices and k
    assert w(2000, 100000, 28, 0) > 2000 * 100000 * 4 and w(8, 3000000, 1024, 0) > 0     # auto slicing
    # rows form: the compact rows alone, their stride a 16-byte multiple
    assert w(4, 2048, 10, 0) == 4 * 2048 * 4
    assert 1000 * 40 * 4 <= w(1000, 37, 10, 0) < 1000 * 40 * 4 + 256
    for args in ((4, 100000, 10, 1), (7, 5003, 28, 3), (1, 1, 1, 0), (333, 2049, 1024, 0)):
        assert w(*args) % 256 == 0 and w(*args) > 0
    prev = 0
    for m in (1, 2, 16, 256, 2000):
        assert w(m, 100000, 28, 0) > prev
        prev = w(m, 100000, 28, 0)
    assert w(0, 100, 10, 1) == 0 and w(4, 0, 10, 1) == 0
    assert w(4, 100, 0, 1) == 0 and w(4, 100, 1025, 1) == 0 and w(4, 100, 10, 257) == 0 and w(4, 100, 10, -1) == 0
    assert w(MAX_GROUPS // 256 + 1, 100000, 10, 256) == 0


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


def test_for_users_rejects_bad_arguments_before_the_library(no_library):
    import qrlsh
    r, src, dst, mil, us = _small()
    for k in (0, 1025, -3, 2.5, True, "3", None):
        with pytest.raises(ValueError):
            qrlsh.for_users(r, src, dst, mil, us, [0], k)
    for slices in (-1, 257, 1.5, True):
        with pytest.raises(ValueError):
            qrlsh.for_users(r, src, dst, mil, us, [0], 3, slices=slices)
    for lo in (2**31, -2**31 - 1, 0.5):
        with pytest.raises(ValueError):
            qrlsh.for_users(r, src, dst, mil, us, [0], 3, lo=lo)
    with pytest.raises(ValueError):
        qrlsh.for_users(r, src, dst, mil, us, [0], 3, sum_order="kahan")
    with pytest.raises(ValueError):
        qrlsh.for_users(r[0], src, dst, mil, us, [0], 3)                       # not 2-D
    with pytest.raises(ValueError):
        qrlsh.for_users(r.astype(np.float64), src, dst, mil, us, [0], 3)       # not integers
    with pytest.raises(ValueError):
        qrlsh.for_users(r, src, dst[:2], mil, us, [0], 3)                      # lists differ in length
    with pytest.raises(ValueError):
        qrlsh.for_users(r, src, dst, mil.to(dtype=__import__("torch").float64), us, [0], 3)
    for users in ([5], [-1], [0, 1, 99], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            qrlsh.for_users(r, src, dst, mil, us, users, 3)
    long_list = {1: {"indexes": np.arange(65) % 5, "values": np.full(65, 0.5)}}
    with pytest.raises(ValueError):
        qrlsh.for_users(r, src, dst, mil, long_list, [0], 3)


def test_predict_users_rejects_bad_arguments_before_the_library(no_library):
    import torch
    import qrlsh
    from qrlsh import predict
    r, src, dst, mil, us = _small()
    with pytest.raises(ValueError):
        qrlsh.predict_users(r, src, dst, mil, us, [0], sum_order="kahan")
    with pytest.raises(ValueError):
        qrlsh.predict_users(r[0], src, dst, mil, us, [0])
    with pytest.raises(ValueError):
        qrlsh.predict_users(r, src[:1], dst, mil, us, [0])
    for users in ([5], [-1], [[0, 1]], [0.5], torch.tensor([0.5]), torch.tensor([[0]])):
        with pytest.raises(ValueError):
            qrlsh.predict_users(r, src, dst, mil, us, users)
    # a prepared tuple for another number of users, or claiming more than 64 neighbours
    ui, uv, ku = predict.user_lists(us, 5, "cpu")
    with pytest.raises(ValueError):
        qrlsh.predict_users(np.zeros((6, 7), dtype=np.int32), src, dst, mil, (ui, uv, ku), [0])
    with pytest.raises(ValueError):
        qrlsh.predict_users(r, src, dst, mil, (ui, uv, 65), [0])


def test_recommender_recommend_users_rejects_bad_arguments_before_the_library(no_library):
    import recommender
    g = load("cfg2_scores")
    rec = recommender.Recommender()
    rec.ratings = g["ratings"]

    def no_similarities():
        raise AssertionError("computed user similarities")
    rec.compute_userSimilarities = no_similarities
    for k in (0, 1025, 2.5):
        with pytest.raises(ValueError):
            rec.recommend_users([0], k)
    with pytest.raises(ValueError, match="no live lists"):
        rec.recommend_users([0], 5)                      # no run yet
    with pytest.raises(ValueError, match="no live lists"):
        rec.predict_users([0])


# ------------------------------------------------------------------------------------------------------ user_lists
def test_user_lists_pads_as_fill_predictions_did():
    from qrlsh import predict
    c = PC.build_case(7, nu=160, nq=400, tu=6, tq=12, user_longest=64)
    ui, uv, ku = predict.user_lists(c.us, c.nu, "cpu")
    want_i, want_v = c.user_lists()
    assert ku == want_i.shape[1] == max(len(v["indexes"]) for v in c.us.values())
    assert ui.dtype == __import__("torch").int32 and uv.dtype == __import__("torch").float64
    assert np.array_equal(ui.numpy(), want_i) and np.array_equal(uv.numpy(), want_v)
    # users without an entry get an empty list; no lists at all: one padding column, ku = 0
    part = {u: c.us[u] for u in (0, 5, 159)}
    ui, uv, ku = predict.user_lists(part, c.nu, "cpu")
    assert ku == max(len(part[u]["indexes"]) for u in part) and ui.shape == (c.nu, ku)
    assert (ui[1] == -1).all() and (uv[1] == 0).all()
    assert np.array_equal(ui[5, :len(part[5]["indexes"])].numpy(), part[5]["indexes"])
    ui, uv, ku = predict.user_lists({}, 9, "cpu")
    assert ku == 0 and ui.shape == (9, 1) and (ui == -1).all() and (uv == 0).all()
    with pytest.raises(ValueError):
        predict.user_lists({0: {"indexes": np.arange(65), "values": np.ones(65)}}, 70, "cpu")
