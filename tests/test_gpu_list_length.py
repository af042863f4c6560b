"""Changing the list length of the live lists in place (qrlsh_lists_cut_*, qrlsh_lists_regrow_mark, qrlsh_index_pick_keys,
QueryIndex.set_list_length, UserLists.set_list_length, Recommender.set_list_lengths, tune(apply_cuts=True)): every
comparison is exact, against the oracle's lists at the new length, the numpy restatements of tests/list_length_cases.py
and the device's own full path -- never against the code under test."""
import ctypes

import numpy as np
import pytest
import torch

import list_length_cases as LL
import lists_update_cases as LC
import tune_cases as TC
import user_lists_cases as UC
from test_gpu_index_remove import (FORMATS, _assert_lists, _assert_snapshot, _dev, _device_full, _host, _index, _rows,
                                   _snapshot)

pytestmark = pytest.mark.gpu

B = LC.CROWDED["b"]


@pytest.fixture(scope="module")
def full():
    """(hi, K) -> the oracle's lists over LC.crowded(hi), computed once per setting and left unchanged"""
    memo = {}

    def get(hi, K):
        if (hi, K) not in memo:
            memo[(hi, K)] = LC.full_lists(LC.crowded(hi), B, K)
        return memo[(hi, K)]
    return get


@pytest.fixture(scope="module")
def popular_full():
    memo = {}

    def get(K):
        if K not in memo:
            memo[K] = _device_full(LC.popular(), LC.POPULAR["b"], K)
        return memo[K]
    return get


# ------------------------------------------------------------------------------------------------ 1. cuts
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("hi", [3, 40])
def test_cuts_are_the_lists_of_a_run_at_the_new_length(full, hi, compact):
    sig = LC.crowded(hi)
    for K_old, targets in ((4, (3, 2, 1)), (64, (63, 5, 1) if hi == 3 else ())):
        stored = full(hi, K_old)
        for K2 in targets:
            qi = _index(sig, B, K_old, compact, lists=stored)
            given = qi.lists
            snap = _snapshot(qi)
            assert qi.set_list_length(K2) == 0 and qi.last_picked == 0 and qi.lists_K == K2 and qi.K == K_old
            _assert_lists(qi.lists, full(hi, K2), (hi, K_old, K2, "oracle"))
            _assert_lists(qi.lists, LL.restate_cut(stored, K2), (hi, K_old, K2, "restatement"))
            assert all(a.data_ptr() != b.data_ptr() for a, b in zip(qi.lists, given))
            if K_old == 4:
                assert len(qi.lists[0]) == (LL.CUT_ENTRIES_40[K2] if hi == 40 else K2 * 323)
            qi.lists = given
            _assert_snapshot(qi, snap, "the index arrays, the rows and the tensors given are not written")
    # K2 == lists_K: nothing happens, the same object stays
    qi = _index(sig, B, 4, compact, lists=full(hi, 4))
    held = qi.lists
    assert qi.set_list_length(4) == 0 and qi.lists is held and qi.lists_K == 4


def test_cuts_across_many_tiles(popular_full):
    """5200 rows x 5 = 26 000 entries: rows straddle every tile boundary and many tiles reach the scan"""
    p = LC.POPULAR
    sig = LC.popular()
    stored = popular_full(5)
    assert len(stored[0]) == 26000
    for K2 in (4, 1):
        qi = _index(sig, p["b"], 5, lists=stored)
        qi.set_list_length(K2)
        _assert_lists(qi.lists, LL.restate_cut(stored, K2), (K2, "restatement"))
        _assert_lists(qi.lists, popular_full(K2), (K2, "full path"))


def test_cut_edges(full):
    from qrlsh import ops
    stored = full(3, 64)
    n = LC.CROWDED["N"]
    # 323 rows of exactly 64 entries: a row ends on every multiple of 64, the tile boundaries among them
    assert len(stored[0]) == 323 * 64 and (np.bincount(stored[0])[np.unique(stored[0])] == 64).all()
    # i < K2 at the first row: a list shorter than K2 altogether survives whole
    short = tuple(a[:3].copy() for a in full(40, 4))
    _assert_lists(ops.lists_cut(*_dev(short), n, 7, 5), short, "shorter than K2")
    e = torch.empty((0,), dtype=torch.int32, device="cuda")
    assert all(t.numel() == 0 and t.dtype == torch.int32 for t in ops.lists_cut(e, e, e, n, 4, 2))
    # inputs that do not start on 16 bytes are served
    d = _dev(tuple(np.concatenate((a[:1], a)) for a in full(40, 4)))
    _assert_lists(ops.lists_cut(*(t[1:] for t in d), n, 4, 2), full(40, 2), "unaligned")


# ------------------------------------------------------------------------------------------------ 2. regrows
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("case", sorted(LL.REGROWS))
def test_regrows_are_the_lists_of_a_run_at_the_new_length(full, case, compact):
    hi, K_old, K2 = case
    picked, before, after = LL.REGROWS[case]
    sig = LC.crowded(hi)
    stored = full(hi, K_old)
    qi = _index(sig, B, K_old, compact, lists=stored)
    given = qi.lists
    snap = _snapshot(qi)
    assert len(stored[0]) == before
    assert qi.set_list_length(K2) == picked == qi.last_picked and qi.lists_K == K2 and qi.K == K_old
    got = _host(qi.lists)
    _assert_lists(got, full(hi, K2), (case, "oracle"))
    assert len(got[0]) == after
    if K2 <= 64:
        _assert_lists(got, _device_full(sig, B, K2, compact), (case, "full path"))
    qi.lists = given
    _assert_snapshot(qi, snap, "the index arrays, the rows and the tensors given are not written")


def test_regrow_streams_a_popular_key_through_the_select(popular_full):
    p = LC.POPULAR
    sig = LC.popular()
    qi = _index(sig, p["b"], 5, lists=popular_full(5))
    assert qi.set_list_length(8) == 5200
    _assert_lists(qi.lists, popular_full(8), "full path")


@pytest.mark.parametrize("compact", FORMATS)
def test_regrow_takes_its_keys_from_the_index(compact):
    """with caller keys that all collide a recomputed key finds nothing"""
    c = LC.WIDE
    sig = LC.wide()
    N, b = c["N"], c["b"]
    stored, want = LC.full_lists(sig, b, 6), LC.full_lists(sig, b, 9)
    assert (np.bincount(stored[0], minlength=N) == 6).all()
    for collide in (False, True):
        keys = torch.zeros((b, N), dtype=torch.int64, device="cuda") if collide else None
        qi = _index(sig, b, 6, compact, lists=stored, keys=keys)
        assert qi.set_list_length(9) == N
        _assert_lists(qi.lists, want, (compact, collide))


# ------------------------------------------------------------------------------------------------ 3. the length sticks
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("K_old,K2", [(4, 3), (4, 6)])
def test_later_updates_keep_the_new_length(K_old, K2, compact):
    sig = LC.crowded(40)
    n, N = 300, LC.CROWDED["N"]
    qi = _index(sig[:n], B, K_old, compact, lists=LC.full_lists(sig[:n], B, K_old))
    qi.set_list_length(K2)
    _assert_lists(qi.lists, LC.full_lists(sig[:n], B, K2), "set")
    qi.append(_rows(sig[n:], compact), update_lists=True)
    rows = sig.copy()
    _assert_lists(qi.lists, LC.full_lists(rows, B, K2), "append")
    gone = np.random.default_rng(3).choice(N, 40, replace=False)
    qi.remove(gone, update_lists=True)
    rows = np.delete(rows, gone, axis=0)
    _assert_lists(qi.lists, LC.full_lists(rows, B, K2), "remove")
    ids = np.random.default_rng(4).choice(len(rows), 30, replace=False)
    new = LC.crowded(40, seed=99)[:30]
    qi.replace(ids, _rows(new, compact), update_lists=True)
    rows[ids] = new
    _assert_lists(qi.lists, LC.full_lists(rows, B, K2), "replace")
    assert qi.lists_K == K2 and qi.K == K_old


@pytest.mark.parametrize("hi", [3, 40])
def test_round_trip(full, hi):
    qi = _index(LC.crowded(hi), B, 4, lists=full(hi, 4))
    qi.set_list_length(2)
    _assert_lists(qi.lists, full(hi, 2), "cut")
    assert qi.set_list_length(4) == len(LL.full_rows(full(hi, 2)[0], 2)) > 0
    _assert_lists(qi.lists, full(hi, 4), "and back")


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_change_nothing(full):
    from qrlsh.index import MAX_K
    sig = LC.crowded(40)
    stored = full(40, 4)
    qi = _index(sig, B, 4, lists=stored)
    snap = _snapshot(qi)
    for bad in (0, MAX_K + 1, True, 2.0):
        with pytest.raises(ValueError):
            qi.set_list_length(bad)
    none = _index(sig, B, 4)
    with pytest.raises(ValueError, match="holds no lists"):
        none.set_list_length(3)
    # a row of K_old + 1 entries; src descending
    s = stored[0].copy()
    rows, counts = np.unique(s, return_counts=True)
    first = int(np.flatnonzero(counts == 4)[0])
    at = int(np.searchsorted(s, rows[first]))
    assert counts[first + 1] >= 1
    long_row = s.copy()
    long_row[at + 4] = rows[first]
    down = s.copy()
    down[[10, 200]] = down[[200, 10]]
    assert down[10] > down[11]
    for name, src in (("a row longer than K", long_row), ("src descending", down)):
        for K2 in (2, 6):
            broken = _index(sig, B, 4, lists=stored)           # the constructor checks the order itself: broken afterwards
            broken.lists = _dev((src, stored[1], stored[2]))
            held = broken.lists
            shot = _snapshot(broken)
            with pytest.raises(ValueError, match="stored lists"):
                broken.set_list_length(K2)
            assert broken.lists is held and broken.lists_K == 4, (name, K2)
            _assert_snapshot(broken, shot, (name, K2))
    assert qi.lists_K == 4
    _assert_snapshot(qi, snap, "after the refusals")


def test_c_abi(full):
    from qrlsh import _lib
    from qrlsh.ops import _ptr, _stream
    lib = _lib.load()
    stored = full(40, 4)
    src = _dev(stored)[0]
    n, E = LC.CROWDED["N"], len(stored[0])
    need = int(lib.qrlsh_lists_cut_workspace_bytes(E))
    assert need > 0 and lib.qrlsh_lists_cut_workspace_bytes(-1) == 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    total = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    for K_new, want in ((4, E), (9, E), (256, E), (3, LL.CUT_ENTRIES_40[3])):
        assert lib.qrlsh_lists_cut_count(_ptr(src), E, n, 4, K_new, _ptr(ws), need, _ptr(total), _stream()) == 0
        assert int(total.item()) == want, K_new
    assert lib.qrlsh_lists_cut_count(_ptr(src), E, n, 3, 2, _ptr(ws), need, _ptr(total), _stream()) == 0
    assert int(total.item()) == -1            # rows of 4 entries under K_old = 3: ~0
    assert lib.qrlsh_lists_cut_count(_ptr(src), E, 5, 4, 2, _ptr(ws), need, _ptr(total), _stream()) == 0
    assert int(total.item()) == -1            # ids outside [0, 5)
    null = ctypes.c_void_p()
    assert lib.qrlsh_lists_cut_count(_ptr(src), E, n, 4, 2, null, need, _ptr(total), _stream()) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_lists_cut_count(_ptr(src), E, n, 4, 2, _ptr(ws), need - 1, _ptr(total), _stream()) == _lib.QRLSH_EINVAL
    for K_old, K_new in ((0, 1), (4, 0), (257, 4), (4, 257)):
        assert lib.qrlsh_lists_cut_count(_ptr(src), E, n, K_old, K_new, _ptr(ws), need, _ptr(total), _stream()) \
            == _lib.QRLSH_EINVAL
    out = torch.empty((E,), dtype=torch.int32, device="cuda")
    assert lib.qrlsh_lists_cut_fill(_ptr(src), _ptr(src), _ptr(src), E, n, 4, 2, _ptr(ws), need, E + 1, _ptr(out), _ptr(out),
                                    _ptr(out), _stream()) == _lib.QRLSH_EINVAL
    assert b"total" in lib.qrlsh_last_error()


# ------------------------------------------------------------------------------------------------ 5. the user side
def _user_host(ul):
    return tuple(t.cpu().numpy() for t in (ul.idx, ul.milli, ul.len))


@pytest.fixture(scope="module")
def user_cases():
    return UC.build_cases()


@pytest.fixture(scope="module")
def user_refs(user_cases):
    memo = {}

    def get(name, K, new=False):
        key = (name, K, new)
        if key not in memo:
            c = user_cases[name]
            memo[key] = UC.reference_lists(c["new"] if new else c["ratings"], c["labels"], K)
        return memo[key]
    return get


@pytest.mark.parametrize("name", sorted(UC.build_cases()))
def test_user_lists_at_every_length(user_cases, user_refs, name):
    from qrlsh.userlists import UserLists
    c = user_cases[name]
    K = c["K"]
    cuts, grows = LL.user_targets(K)
    for K2 in cuts + grows:
        ul = UserLists.build(c["ratings"], c["labels"], K=K)
        held = (ul.idx, ul.milli, ul.len)
        before = [t.clone() for t in held]
        stored = _user_host(ul)
        want_n = 0 if K2 < K else int((stored[2] == K).sum())
        assert ul.set_list_length(K2) == want_n == ul.last_picked and ul.K == K2, (name, K2)
        got = _user_host(ul)
        assert got[0].shape == (ul.nu, K2) and ul.idx.is_contiguous() and ul.milli.is_contiguous()
        assert UC.same(got, user_refs(name, K2)), (name, K2, "reference")
        assert UC.same(got, LL.user_cut(stored, K2) if K2 < K else
                       LL.user_regrow(stored, c["ratings"], c["labels"], K, K2)[0]), (name, K2, "restatement")
        assert all(torch.equal(a, b) for a, b in zip(before, held)), "the old tensors are not written"
        if name in LL.USER_FULL and K2 > K:
            assert want_n == LL.USER_FULL[name][0]
        ul.rate(*c["edits"])
        assert UC.same(_user_host(ul), user_refs(name, K2, new=True)), (name, K2, "rate afterwards")
    ul = UserLists.build(c["ratings"], c["labels"], K=K)
    held = (ul.idx, ul.milli, ul.len)
    assert ul.set_list_length(K) == 0 and ul.idx is held[0]
    for bad in (0, 65, True):
        with pytest.raises(ValueError):
            ul.set_list_length(bad)
    assert ul.K == K and all(a is b for a, b in zip(held, (ul.idx, ul.milli, ul.len)))


# ------------------------------------------------------------------------------------------------ 6. Recommender
@pytest.fixture()
def served():
    from test_gpu_recommend import _recommender_on
    from qrlsh import users
    rec, g = _recommender_on("cfg1")
    rec.compute_querySimilarities()
    rec.live_user_similarities(labels=users.cluster_labels(rec.ratings))
    return rec


def test_recommender_serves_at_the_new_lengths(served):
    import qrlsh
    from qrlsh import predict, recommend
    rec = served
    ui = rec.user_index
    a, c = 3, 2
    assert rec.last_result.K > a and ui.K > c
    q_host = LL.restate_cut(_host(rec._live_lists()), a)
    u_host = LL.user_cut(_user_host(ui), c)
    ratings = rec.ratings.copy()
    assert rec.set_list_lengths(query_K=a, user_K=c) == (0, 0)
    assert rec._query_index.lists_K == a and ui.K == c and np.array_equal(rec.ratings, ratings)
    _assert_lists(rec._live_lists(), q_host, "the live query lists")
    assert UC.same(_user_host(ui), u_host)
    sims = rec.current_query_similarities()
    assert max(len(v["indexes"]) for v in sims.values()) == a
    user_sim = (torch.from_numpy(u_host[0]).cuda(), torch.from_numpy(u_host[1] / 1000.0).cuda(), c)
    serve = [0, 5, rec.ratings.shape[0] - 1]
    blend = dict(query_weight=rec.query_weight, user_weight=rec.user_weight, default_mean=rec.default_mean)
    want = predict.predict_users(rec.ratings, *_dev(q_host), user_sim, serve, sum_order=rec.sum_order, **blend)
    assert np.array_equal(rec.predict_users(serve).to_numpy(), want.cpu().numpy())
    idx, val, avail = (t.cpu().numpy() for t in recommend.for_users(rec.ratings, *_dev(q_host), user_sim, serve, 10,
                                                                     sum_order=rec.sum_order, **blend))
    out = rec.recommend_users(serve, 10)
    for row, u in enumerate(serve):
        k = min(10, int(avail[row]))
        assert np.array_equal(out[u]["indexes"], idx[row, :k]) and np.array_equal(out[u]["values"], val[row, :k])
        assert out[u]["available"] == avail[row]
    # a regrow through the same door restores the run's lists
    K_run = rec.last_result.K
    picked = rec.set_list_lengths(query_K=K_run)
    assert picked[0] > 0 and picked[1] is None
    _assert_lists(rec._live_lists(), _host((rec.last_result.src, rec.last_result.dst, rec.last_result.val)), "regrown")
    # refusals come before any change
    rec.remove_queries([1])                     # drops the live lists
    with pytest.raises(ValueError, match="dropped"):
        rec.set_list_lengths(query_K=2, user_K=1)
    assert ui.K == c
    for bad in (dict(query_K=0), dict(user_K=65), dict(query_K=True)):
        with pytest.raises(ValueError):
            rec.set_list_lengths(**bad)


WEIGHTS = [TC.DEFAULT] + [(qw, 1.0 - qw, dm) for qw in (0.2, 0.5, 0.8) for dm in (30.0, 45.0, 75.0)]


@pytest.mark.parametrize("holdout", [True, False])
def test_tune_applies_its_cuts_and_evaluate_agrees(served, holdout):
    rec = served
    ui = rec.user_index
    s = 3
    grid = rec.tune(WEIGHTS, q_cuts=[2, 4], u_cuts=[1, 3], fraction=0.5, seed=s, holdout=holdout, apply=True,
                    apply_cuts=True)
    q_cut, u_cut, triple, index = grid.best()
    assert (rec._query_index.lists_K, ui.K) == (q_cut, u_cut) and q_cut in (2, 4) and u_cut in (1, 3)
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == triple
    ev = rec.evaluate(fraction=0.5, seed=s, holdout=holdout)
    assert np.array_equal(TC.words8(ev.totals), grid.totals.reshape(-1, 8)[index]) and ev.n > 100


def test_tune_ranking_applies_its_cuts_and_evaluate_ranking_agrees(served):
    rec = served
    k, relevant, s = 7, 60, 11
    grid = rec.tune_ranking(k, relevant, WEIGHTS[:4], q_cuts=[2, 4], u_cuts=[1, 3], fraction=0.5, seed=s, apply=True,
                            apply_cuts=True)
    q_cut, u_cut, triple, index = grid.best()
    assert (rec._query_index.lists_K, rec.user_index.K) == (q_cut, u_cut)
    one = rec.evaluate_ranking(k, relevant, fraction=0.5, seed=s, candidates="heldout")
    assert np.array_equal(one.totals, grid.totals.reshape(-1, 16)[index])


def test_tune_refuses_before_it_changes_anything(served):
    rec = served
    ui = rec.user_index
    lists = rec._live_lists()
    held = (ui.idx, ui.milli, ui.len)
    blend = (rec.query_weight, rec.user_weight, rec.default_mean)

    def unchanged():
        return (all(a is b for a, b in zip(lists, rec._live_lists())) and ui.K == held[0].shape[1]
                and all(a is b for a, b in zip(held, (ui.idx, ui.milli, ui.len)))
                and blend == (rec.query_weight, rec.user_weight, rec.default_mean))
    # apply_cuts=False (the default): the cuts are only reported
    rec.tune(WEIGHTS, q_cuts=[2, 4], u_cuts=[1, 3], fraction=0.5, seed=3)
    assert unchanged()
    # cuts that do not shorten are left alone: tune never regrows
    rec.tune(WEIGHTS[:1], q_cuts=[200], u_cuts=[64], fraction=0.5, seed=3, apply_cuts=True)
    rec.tune(WEIGHTS[:1], fraction=0.5, seed=3, apply_cuts=True)
    assert unchanged()
    # a best setting with the query side switched off
    with pytest.raises(ValueError, match="switches the query side off"):
        rec.tune(WEIGHTS, q_cuts=[0], u_cuts=[1, 3], fraction=0.5, seed=3, apply=True, apply_cuts=True)
    assert unchanged()
    with pytest.raises(ValueError, match="switches the user side off"):
        rec.tune(WEIGHTS, q_cuts=[2, 4], u_cuts=[0], fraction=0.5, seed=3, apply=True, apply_cuts=True)
    assert unchanged()
    # a user cut with the index out of step
    rec.ratings = np.vstack((rec.ratings, rec.ratings[:1]))
    rec.usersIDs = np.concatenate((rec.usersIDs, rec.usersIDs[:1]))
    with pytest.raises(ValueError, match="in step"):
        rec.tune(WEIGHTS, q_cuts=[2, 4], u_cuts=[1, 3], fraction=0.5, seed=3, holdout=False,
                 user_sim=rec.compute_userSimilarities(), apply=True, apply_cuts=True)
    assert unchanged()
    with pytest.raises(ValueError, match="in step"):
        rec.set_list_lengths(query_K=2, user_K=1)
    assert unchanged()
