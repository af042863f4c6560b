"""Recommendations (qrlsh_recommend_topk): the numpy restatement the GPU tests hold the device to, checked against
the reference's own expressions (recommender.py:361, :370) on the golden fixtures, and every argument check of the
C ABI and the host layer, none of which needs a device."""
import ctypes

import numpy as np
import pytest

from helpers import load

SCORES = ["cfg1_scores", "cfg1b_scores", "cfg2_scores"]


def restate(ratings, pred, k, users=None):
    """The contract: per user the eligible cells (unrated, non-zero prediction), value descending then index
    ascending, the first k; idx -1 / val 0 past them.  -> (idx, val, avail) int64 arrays."""
    ratings, pred = np.asarray(ratings), np.asarray(pred)
    rows = np.arange(ratings.shape[0]) if users is None else np.asarray(users)
    idx = np.full((len(rows), k), -1, dtype=np.int64)
    val = np.zeros((len(rows), k), dtype=np.int64)
    avail = np.zeros(len(rows), dtype=np.int64)
    for i, u in enumerate(rows):
        cols = np.nonzero((ratings[u] == 0) & (pred[u] != 0))[0]
        v = pred[u][cols].astype(np.int64)
        order = np.lexsort((cols, -v))[:k]      # last key primary: -value, then index
        n = len(order)
        idx[i, :n], val[i, :n], avail[i] = cols[order], v[order], len(cols)
    return idx, val, avail


def reference_topk(to_predict, predictions, user, k):
    """recommender.py:361 and :370, literally (the prompt's selection for one user)"""
    just_scored = [j for i, j in to_predict if i == user and predictions[i][j] != 0]
    top_k_predictions = np.argsort(predictions[user][just_scored])[::-1][0:k]
    return just_scored, [just_scored[p] for p in top_k_predictions]


@pytest.mark.parametrize("name", SCORES)
def test_restatement_matches_reference_expressions_on_golden(name):
    g = load(name)
    ratings, final = g["ratings"], g["final"]
    to_predict = [tuple(x) for x in g["to_predict"]]
    nu = ratings.shape[0]
    for u in range(nu):
        just_scored, _ = reference_topk(to_predict, final, u, 1)
        for k in sorted({1, 3, max(1, len(just_scored))}):
            _, ref_cols = reference_topk(to_predict, final, u, k)
            idx, val, avail = restate(ratings, final, k, users=[u])
            assert avail[0] == len(just_scored)
            n = min(k, len(just_scored))
            mine = idx[0, :n]
            assert np.all(idx[0, n:] == -1) and np.all(val[0, n:] == 0)
            assert np.array_equal(val[0, :n], final[u][ref_cols]), "value sequence differs (user %d, k %d)" % (u, k)
            # the index set is the same wherever no value is tied across the cut
            if n and (n == len(just_scored) or final[u][just_scored].tolist().count(val[0, n - 1]) ==
                      list(val[0, :n]).count(val[0, n - 1])):
                assert set(mine.tolist()) == set(ref_cols)
            # inside the restatement: value descending, index ascending among equal values
            for a in range(n - 1):
                assert val[0, a] > val[0, a + 1] or (val[0, a] == val[0, a + 1] and mine[a] < mine[a + 1])


def test_restatement_tie_order_and_padding():
    ratings = np.array([[0, 0, 5, 0, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]])
    pred = np.array([[7, 9, 5, 7, -3, 0], [2, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0]])
    idx, val, avail = restate(ratings, pred, 4)
    assert idx[0].tolist() == [1, 0, 3, 4] and val[0].tolist() == [9, 7, 7, -3] and avail[0] == 4
    assert idx[1].tolist() == [-1] * 4 and val[1].tolist() == [0] * 4 and avail[1] == 0
    assert avail[2] == 0


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    """distinct, 16-byte-aligned non-null addresses; the argument checks return before anything is dereferenced"""
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def _call(lib, k=10, m=4, nu=4, nq=100000, users=None, slices=1, outs=True, ws_bytes=None, lo=0):
    r, p, io, vo, ao, ws = _fake(6)
    need = lib.qrlsh_recommend_workspace_bytes(m, nq, k, slices) if ws_bytes is None else ws_bytes
    return lib.qrlsh_recommend_topk(r, p, nu, nq, users, m, k, lo, slices, io if outs else None, vo if outs else None,
                                    ao if outs else None, ws, need, None)


def test_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    for k in (0, 1025, -1):
        assert _call(lib, k=k) == _lib.QRLSH_EINVAL
        assert b"k=" in lib.qrlsh_last_error()
    assert _call(lib, m=-1, nu=4) == _lib.QRLSH_EINVAL
    assert _call(lib, nq=-1) == _lib.QRLSH_EINVAL
    assert _call(lib, nq=2**31) == _lib.QRLSH_EINVAL
    assert _call(lib, nu=-2) == _lib.QRLSH_EINVAL
    assert _call(lib, slices=257) == _lib.QRLSH_EINVAL
    assert _call(lib, slices=-1) == _lib.QRLSH_EINVAL
    assert _call(lib, m=3, nu=4) == _lib.QRLSH_EINVAL            # no user list: m must be nu
    assert _call(lib, outs=False) == _lib.QRLSH_EINVAL
    assert b"null output" in lib.qrlsh_last_error()
    need = lib.qrlsh_recommend_workspace_bytes(4, 100000, 10, 1)
    assert _call(lib, ws_bytes=need - 1) == _lib.QRLSH_EWORKSPACE
    assert b"workspace" in lib.qrlsh_last_error()
    # misaligned matrix base
    io, vo, ao, ws = _fake(4)
    rc = lib.qrlsh_recommend_topk(ctypes.c_void_p(0x100004), ctypes.c_void_p(0x200000), 4, 100000, None, 4, 10, 0, 1,
                                  io, vo, ao, ws, need, None)
    assert rc == _lib.QRLSH_EINVAL and b"aligned" in lib.qrlsh_last_error()
    # m = 0: nothing to do, outputs may be null
    assert lib.qrlsh_recommend_topk(None, None, 0, 10, None, 0, 5, 0, 0, None, None, None, None, 0, None) == _lib.QRLSH_OK
    with pytest.raises(_lib.QrlshError):
        _lib.check(_call(lib, k=0))


def test_abi_workspace_bytes():
    from qrlsh import _lib
    lib = _lib.load()
    w = lib.qrlsh_recommend_workspace_bytes
    assert w(4, 100000, 10, 1) > 0
    assert w(8, 100000, 10, 1) > w(4, 100000, 10, 1)                  # grows with m
    assert w(4, 100000, 10, 2) > w(4, 100000, 10, 1)                  # and with slices
    assert w(4, 100000, 1024, 1) > w(4, 100000, 10, 1)                # and with k
    assert w(2000, 100000, 28, 0) > 0 and w(8, 3000000, 1024, 0) > 0   # auto slicing
    assert w(100000, 64, 10, 0) == 0                                  # rows form: no workspace
    assert w(0, 100, 10, 1) == 0 and w(4, 0, 10, 1) == 0
    assert w(4, 100, 0, 1) == 0 and w(4, 100, 1025, 1) == 0 and w(4, 100, 10, 257) == 0


# ----------------------------------------------------------------------------------- host layer, before the device
def test_top_k_rejects_bad_arguments_before_the_device(monkeypatch):
    import qrlsh
    from qrlsh import recommend as R

    def no_device(*a, **kw):
        raise AssertionError("touched the device")
    monkeypatch.setattr(R, "_on_device", no_device)
    r = np.zeros((5, 7), dtype=np.int32)
    p = np.ones((5, 7), dtype=np.int32)
    for k in (0, 1025, -3, 2.5, True, "3", None):
        with pytest.raises(ValueError):
            qrlsh.top_k(r, p, k)
    with pytest.raises(ValueError):
        qrlsh.top_k(r, np.ones((5, 8), dtype=np.int32), 3)              # shapes differ
    with pytest.raises(ValueError):
        qrlsh.top_k(r[0], p[0], 3)                                      # not 2-D
    with pytest.raises(ValueError):
        qrlsh.top_k(r, p.astype(np.float64), 3)                         # not integers
    with pytest.raises(ValueError):
        qrlsh.top_k(r, p.astype(np.int64) * 2**33, 3)                   # outside int32
    for users in ([5], [-1], [0, 1, 99], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            qrlsh.top_k(r, p, 3, users=users)
    for slices in (-1, 257):
        with pytest.raises(ValueError):
            qrlsh.top_k(r, p, 3, slices=slices)
    with pytest.raises(ValueError):
        qrlsh.top_k(r, p, 3, lo=2**31)


def test_recommender_recommend_rejects_bad_arguments_before_the_device(monkeypatch):
    import recommender
    from qrlsh import recommend as R

    def no_device(*a, **kw):
        raise AssertionError("touched the device")
    monkeypatch.setattr(R, "_on_device", no_device)
    g = load("cfg2_scores")
    rec = recommender.Recommender()
    rec.ratings = g["ratings"]
    final = g["final"]
    with pytest.raises(ValueError):
        rec.recommend(final, 0)
    with pytest.raises(ValueError):
        rec.recommend(final, 1025)
    with pytest.raises(ValueError):
        rec.recommend(final[:, :-1], 5)
    with pytest.raises(ValueError):
        rec.recommend(final, 5, users=[0, final.shape[0]])
