"""Diversified lists (qrlsh.diversify / for_users_diverse / list_redundancy, Recommender.recommend_users_diverse): what
needs no device.  The restatement the GPU tests hold the device to (diversify_cases.greedy_ref / redundancy_ref) against
an independent dense form on small cases; the identities of the rule; the conditions the case builders plant, asserted
on the restatement alone; determinism of the builders; the argument checks of the C ABI (fake pointers: each call fails
a check before anything is dereferenced) and of the host layer (before the library is loaded)."""
import ctypes
import importlib

import numpy as np
import pytest

import diversify_cases as DC


@pytest.fixture(scope="module")
def planted():
    return DC.planted_case()


@pytest.fixture(scope="module")
def main():
    return DC.main_case()


def _same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------------------------------- restatement vs brute form
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_greedy_ref_equals_the_dense_brute_form(seed):
    c = DC.small_case(seed)
    ci, cv, av = c.arrays()
    dense = DC.brute_sim(c.lists, c.nq)
    sim = DC.sim_both(DC.stored(c.lists))
    assert all(sim(a, b) == dense[a, b] for a in range(c.nq) for b in range(c.nq) if a != b)
    assert (dense > 0).sum() > 0 and (dense == dense.T).all()
    changed = 0
    for penalty, max_sim in ((0, 1001), (700, 1001), (1 << 20, 1001), (0, 1000), (0, 1), (300, 400)):
        want = DC.greedy_brute(ci, cv, av, dense, c.k, penalty, max_sim)
        got = DC.greedy_ref(ci, cv, av, c.lists, c.k, penalty, max_sim)
        _same(got, want)
        changed += int(not np.array_equal(got[0], DC.greedy_ref(ci, cv, av, c.lists, c.k, 0, 1001)[0]))
        # the redundancy restatement against the dense form
        words, totals = DC.redundancy_ref(got[0], c.lists)
        for x, row in enumerate(got[0]):
            cols = row[row >= 0].astype(np.int64)
            sub = np.triu(dense[np.ix_(cols, cols)], 1)
            assert words[x].tolist() == [len(cols), int((sub > 0).sum()), int(sub.sum()), int(sub.max()) if sub.size else 0]
        assert totals.tolist() == [words[:, 0].sum(), words[:, 1].sum(), words[:, 2].sum(), words[:, 3].max()]
    assert changed >= 3


# ------------------------------------------------------------------------------------------------------- identities
def test_identities_of_the_rule(planted, main):
    for c in (planted, main):
        ci, cv, av = c.arrays()
        n = np.clip(av, 0, c.N)
        # penalty 0, nothing excluded: the first k of the pool, red still filled
        idx, val, red, count = DC.greedy_ref(ci, cv, av, c.lists, c.k, 0, 1001)
        assert np.array_equal(count, np.minimum(n, c.k))
        for x in range(len(av)):
            assert np.array_equal(idx[x, :count[x]], ci[x, :count[x]]) and np.array_equal(val[x, :count[x]], cv[x, :count[x]])
            assert (idx[x, count[x]:] == -1).all() and (val[x, count[x]:] == 0).all() and (red[x, count[x]:] == 0).all()
        assert red.max() > 0
        # red[t] is the largest sim to the earlier picks, and its maximum is the list's largest sim
        sim = DC.sim_both(DC.stored(c.lists))
        for penalty, max_sim in DC.SETTINGS:
            idx, val, red, count = DC.greedy_ref(ci, cv, av, c.lists, c.k, penalty, max_sim)
            words, _ = DC.redundancy_ref(idx, c.lists)
            for x in range(len(av)):
                for t in range(count[x]):
                    assert red[x, t] == max([sim(int(idx[x, t]), int(idx[x, s])) for s in range(t)], default=0)
                    assert red[x, t] < max_sim
            assert np.array_equal(red.max(axis=1), words[:, 3]) and np.array_equal(words[:, 0], count)
            if max_sim == 1:   # no two entries are stored neighbours
                assert words[:, 1].sum() == 0 and red.max() == 0


# --------------------------------------------------------------------------------------------- the planted conditions
def test_rerank_changes_at_least_half_of_the_main_case(main):
    ci, cv, av = main.arrays()
    plain = DC.greedy_ref(ci, cv, av, main.lists, main.k, 0, 1001)
    moved = DC.greedy_ref(ci, cv, av, main.lists, main.k, DC.MODERATE, 1001)
    changed = sum(not np.array_equal(plain[0][x], moved[0][x]) for x in range(len(av)))
    assert len(av) == 300 and changed >= 150, changed
    sizes = np.clip(av, 0, main.N)
    assert (sizes == 0).any() and ((sizes > 0) & (sizes < main.k)).any() and (sizes == main.N).any()
    assert (av > main.N).any() and ((av >= main.k) & (av < main.N)).any()
    # the rerank lowers the redundancy it is there to lower
    assert DC.redundancy_ref(moved[0], main.lists)[1][2] < DC.redundancy_ref(plain[0], main.lists)[1][2]


def test_planted_structures_are_there(planted):
    c = planted
    ci, cv, av = c.arrays()
    fwd = DC.stored(c.lists)
    both = DC.sim_both(fwd)
    # hub: names nobody, named by every other candidate of its pool, served first
    x = c.notes["hub"]
    hub, others = int(ci[x, 0]), [int(q) for q in ci[x, 1:av[x]]]
    assert hub not in fwd and all(hub in fwd[q] for q in others) and len(others) == 199
    # reverse-only edges decide picks at step >= 2: reading the picked entry's own row alone gives other lists
    right = DC.greedy_ref(ci, cv, av, c.lists, c.k, DC.MODERATE, 1001)
    wrong = DC.greedy_ref(ci, cv, av, c.lists, c.k, DC.MODERATE, 1001, sim=DC.sim_picked_row_only(fwd))
    assert right[0][x, 0] == wrong[0][x, 0] == hub and not np.array_equal(right[0][x, 1:], wrong[0][x, 1:])
    assert right[2][x, 1:].max() > 0 and wrong[2][x].max() == 0
    # a row of 256 entirely inside the pool; rows of 1 and 0 beside it
    x = c.notes["row256"]
    pool = set(int(q) for q in ci[x, :av[x]])
    lens = sorted(len(fwd.get(q, {})) for q in pool)
    assert lens[-1] == 256 and set(fwd[int(ci[x, 0])]) <= pool and lens[0] == 0 and 1 in lens
    # one-directional edges, both pick orders
    for note, first in (("a_first", 0), ("b_first", 1)):
        x = c.notes[note]
        a, b = sorted(int(q) for q in ci[x, :2])
        assert b in fwd[a] and a not in fwd.get(b, {}) and both(a, b) == both(b, a) == 900
        assert right[0][x, 0] == (a, b)[first] and (a, b)[1 - first] in right[0][x].tolist()
        t = right[0][x].tolist().index((a, b)[1 - first])
        assert right[2][x, t] == 900 and t > 1   # the penalty moved it back
    # the tie runs: equal values and equal r on both sides of positions 63 / 64 and 255 / 256, taken in position order
    trace = []
    DC.greedy_ref(ci, cv, av, c.lists, c.k, DC.MODERATE, 1001, trace=trace)
    for note, edge in (("tie63", 63), ("tie255", 255)):
        x = c.notes[note]
        pos = [ci[x].tolist().index(q) for q in right[0][x]]
        assert pos[0] == 0 and pos[1:] == list(range(pos[1], pos[1] + 11)) and pos[1] < edge < edge + 1 < pos[-1]
        assert len(set(cv[x, pos[1:]].tolist())) == 1 and right[2][x, 1:].max() == 0
        assert sum(tied for (r, t, tied) in trace if r == x) >= 10
    # negative values, and penalties that drive scores negative
    x = c.notes["negative"]
    assert cv[x, :av[x]].max() < 0
    hard = DC.greedy_ref(ci, cv, av, c.lists, c.k, 1 << 20, 1001)
    assert not np.array_equal(hard[0][x], ci[x, :c.k])
    h = c.notes["hub"]    # positive values, every score after the hub's below zero
    assert hard[1][h].min() > 0 and hard[2][h, 1:].min() > 0
    assert (1000 * hard[1][h, 1:].astype(np.int64) - (1 << 20) * hard[2][h, 1:].astype(np.int64)).max() < 0
    # the clique: with penalty 0 and max_sim 1000 exactly one member survives
    x = c.notes["clique"]
    clique = set(int(q) for q in ci[x, :10])
    assert all(both(a, b) == 1000 for a in clique for b in clique if a != b)
    cut = DC.greedy_ref(ci, cv, av, c.lists, c.k, 0, 1000)
    assert len(clique & set(cut[0][x].tolist())) == 1 and cut[3][x] == c.k
    # max_sim = 1 exhausts the hub's pool before k
    lone = DC.greedy_ref(ci, cv, av, c.lists, c.k, 0, 1)
    assert lone[3][c.notes["hub"]] == 1 < c.k and (lone[3] < np.minimum(np.clip(av, 0, c.N), c.k)).sum() >= 2
    # a neighbour outside the pool does not count
    x = c.notes["outside"]
    a, b = int(ci[x, 0]), int(ci[x, 1])
    z = next(iter(fwd[a]))
    assert z not in ci[x].tolist() and both(a, z) == 1000 and both(z, b) == 1000 and both(a, b) == 0
    for out in (right, hard, cut, lone):
        assert out[2][x].max() == 0 and np.array_equal(out[0][x, :5], ci[x, :5])


def test_builders_are_deterministic_and_well_formed():
    for build in (DC.planted_case, DC.main_case, lambda: DC.size_case(65), DC.full_order_case, lambda: DC.small_case(2)):
        a, b = build(), build()
        _same(a.arrays(), b.arrays())
        _same(a.coo(), b.coo())
        ci, cv, av = a.arrays()
        for x in range(len(av)):
            n = min(a.N, max(int(av[x]), 0))
            cols, vals = ci[x, :n].astype(np.int64), cv[x, :n].astype(np.int64)
            assert len(set(cols.tolist())) == n and ((cols >= 0) & (cols < a.nq)).all()
            assert np.array_equal(np.lexsort((cols, -vals)), np.arange(n))      # served order
        for q, (ids, milli) in a.lists.items():
            assert len(ids) and q not in ids and len(set(ids.tolist())) == len(ids)
            assert milli.min() >= 1 and milli.max() <= 1000 and ((ids >= 0) & (ids < a.nq)).all()
            assert np.array_equal(np.lexsort((ids, -milli)), np.arange(len(ids)))
    assert [DC.size_case(n).N for n in DC.SIZES] == list(DC.SIZES)


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def _diversify(lib, m=4, N=64, nq=5000, k=10, penalty=0, max_sim=1001, flag=True, outs=True, lists=True, ws_bytes=None,
               ws_addr=None):
    ci, cv, av, qo, qi, qm, io, vo, ro, co, fl, ws = _fake(12)
    need = lib.qrlsh_diversify_workspace_bytes(m, N, 28) if ws_bytes is None else ws_bytes
    return lib.qrlsh_diversify(ci, cv, av, m, N, nq, qo if lists else None, qi, qm, k, penalty, max_sim,
                               io if outs else None, vo, ro, co, fl if flag else None,
                               ws if ws_addr is None else ctypes.c_void_p(ws_addr), need, None)


def _redundancy(lib, m=4, k=10, nq=5000, flag=True, outs=True, lists=True, ws_bytes=None):
    li, qo, qi, qm, wo, to, fl, ws = _fake(8)
    need = lib.qrlsh_diversify_workspace_bytes(m, k, 28) if ws_bytes is None else ws_bytes
    return lib.qrlsh_list_redundancy(li, m, k, nq, qo if lists else None, qi, qm, wo if outs else None, to,
                                     fl if flag else None, ws, need, None)


def test_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    for kw in (dict(N=0), dict(N=1025), dict(k=0), dict(k=65), dict(penalty=-1), dict(penalty=(1 << 20) + 1),
               dict(max_sim=-1), dict(max_sim=1002), dict(m=-1), dict(nq=-1), dict(nq=2**31), dict(flag=False),
               dict(outs=False), dict(lists=False), dict(ws_addr=0x100004)):
        assert _diversify(lib, **kw) == E, kw
    assert b"aligned" in lib.qrlsh_last_error()
    assert _diversify(lib, m=(1 << 24) + 1, ws_bytes=1 << 40) == _lib.QRLSH_EUNSUPPORTED
    assert _diversify(lib, ws_bytes=4 * 68 * 4 - 1) == _lib.QRLSH_EWORKSPACE
    assert b"workspace" in lib.qrlsh_last_error()
    assert _diversify(lib, m=0, outs=False, lists=False) == _lib.QRLSH_OK
    for kw in (dict(k=0), dict(k=1025), dict(m=-1), dict(nq=2**31), dict(flag=False), dict(outs=False), dict(lists=False)):
        assert _redundancy(lib, **kw) == E, kw
    assert _redundancy(lib, ws_bytes=4 * 12 * 4 - 1) == _lib.QRLSH_EWORKSPACE
    assert _redundancy(lib, m=0, outs=False, lists=False) == _lib.QRLSH_OK
    with pytest.raises(_lib.QrlshError):
        _lib.check(_diversify(lib, k=65))


def test_workspace_bytes():
    from qrlsh import _lib
    w = _lib.load().qrlsh_diversify_workspace_bytes
    # per request: N + 1 offsets rounded to four words, and 2 N min(max_row, N - 1) half-edges
    assert w(1, 1024, 28) == 4 * (1028 + 2 * 1024 * 28)
    assert w(2000, 1024, 28) == 2000 * w(1, 1024, 28) < 1 << 30
    assert w(1, 64, 500) == 4 * (68 + 2 * 64 * 63) == w(1, 64, 63)
    assert w(1, 1, 28) == 16 and w(3, 2, 0) == 3 * 16
    assert w(0, 64, 28) == 0 and w(4, 0, 28) == 0 and w(4, 1025, 28) == 0 and w(4, 64, -1) == 0
    assert w((1 << 24) + 1, 64, 28) == 0


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


def test_diversify_rejects_bad_arguments_before_the_library(no_library):
    import qrlsh
    ci, cv, av, src, dst, mil = _pools()
    for k in (0, 5, 1025, -3, 2.5, True, "3", None):          # 5 > N = 4
        with pytest.raises(ValueError):
            qrlsh.diversify(ci, cv, av, src, dst, mil, 7, k)
    for penalty in (-1, (1 << 20) + 1, 0.5, True, None):
        with pytest.raises(ValueError):
            qrlsh.diversify(ci, cv, av, src, dst, mil, 7, 2, penalty=penalty)
    for max_sim in (-1, 1002, 0.5, False):
        with pytest.raises(ValueError):
            qrlsh.diversify(ci, cv, av, src, dst, mil, 7, 2, max_sim=max_sim)
    for nq in (-1, 2**31, 7.0):
        with pytest.raises(ValueError):
            qrlsh.diversify(ci, cv, av, src, dst, mil, nq, 2)
    with pytest.raises(ValueError):
        qrlsh.diversify(ci[0], cv[0], av, src, dst, mil, 7, 2)                # not 2-D
    with pytest.raises(ValueError):
        qrlsh.diversify(ci, cv[:, :3], av, src, dst, mil, 7, 2)               # shapes differ
    with pytest.raises(ValueError):
        qrlsh.diversify(ci, cv, av[:1], src, dst, mil, 7, 2)
    with pytest.raises(ValueError):
        qrlsh.diversify(ci.astype(np.float64), cv, av, src, dst, mil, 7, 2)   # not integers
    with pytest.raises(ValueError):
        qrlsh.diversify(ci, cv, av, src, dst[:2], mil, 7, 2)                  # lists differ in length
    with pytest.raises(ValueError):
        qrlsh.diversify(ci, cv, av, src, dst, mil.astype(np.float32), 7, 2)
    wide = np.zeros((1, 1025), dtype=np.int32)
    with pytest.raises(ValueError):
        qrlsh.diversify(wide, wide, np.array([0]), src, dst, mil, 7, 2)       # N > 1024
    with pytest.raises(ValueError):
        qrlsh.list_redundancy(ci[0], src, dst, mil, 7)
    with pytest.raises(ValueError):
        qrlsh.list_redundancy(wide, src, dst, mil, 7)
    with pytest.raises(ValueError):
        qrlsh.list_redundancy(ci, src, dst, mil, -1)
    with pytest.raises(ValueError):
        qrlsh.list_redundancy(np.zeros((2, 0), dtype=np.int32), src, dst, mil, 7)


def test_for_users_diverse_rejects_bad_arguments_before_the_library(no_library):
    import qrlsh
    r = np.zeros((5, 7), dtype=np.int32)
    _, _, _, src, dst, mil = _pools()
    us = {0: {"indexes": np.array([1, 2]), "values": np.array([0.5, 0.25])}}
    for kw in (dict(k=0), dict(k=1025), dict(k=2.5), dict(k=3, pool=2), dict(k=3, pool=1025), dict(k=3, pool=0),
               dict(k=3, pool=4.0), dict(k=3, penalty=-1), dict(k=3, penalty=(1 << 20) + 1), dict(k=3, max_sim=1002),
               dict(k=3, max_sim=-1), dict(k=3, slices=257), dict(k=3, lo=2**31), dict(k=3, sum_order="kahan")):
        with pytest.raises(ValueError):
            qrlsh.for_users_diverse(r, src, dst, mil, us, [0], **kw)
    with pytest.raises(ValueError):
        qrlsh.for_users_diverse(r, src, dst, mil, us, [5], 3)
    with pytest.raises(ValueError):
        qrlsh.for_users_diverse(r[0], src, dst, mil, us, [0], 3)
    dv = importlib.import_module("qrlsh.diversify")
    assert [dv.default_pool(k) for k in (1, 10, 16, 17, 28, 256, 1024)] == [64, 64, 64, 68, 112, 1024, 1024]


def test_recommender_rejects_bad_arguments_before_the_library(no_library):
    import recommender
    from helpers import load
    rec = recommender.Recommender()
    rec.ratings = load("cfg2_scores")["ratings"]

    def no_similarities():
        raise AssertionError("computed user similarities")
    rec.compute_userSimilarities = no_similarities
    for kw in (dict(k=0, penalty=0), dict(k=1025, penalty=0), dict(k=5, penalty=-1), dict(k=5, penalty=0, max_sim=1002),
               dict(k=5, penalty=0, pool=4), dict(k=5, penalty=0, pool=2000)):
        with pytest.raises(ValueError):
            rec.recommend_users_diverse([0], **kw)
    with pytest.raises(ValueError, match="no live lists"):
        rec.recommend_users_diverse([0], 5, 1000)
    with pytest.raises(ValueError, match="no live lists"):
        rec.list_redundancy({0: {"indexes": np.array([1, 2])}})
