"""Serving new queries without a device: the numpy restatement of the probe contract checked against the C oracle and
against the reference's own output by holding queries out of the golden fixtures; the column-prediction restatement
and its knife-edge cells; every argument check of the C ABI and of the host layer."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import predict_cases as PC
import query_index_cases as QC
from helpers import load
from oracle import oracle as O


def test_restatement_equals_the_oracle_candidates_and_scores():
    for name, g, sig, b, K in QC.golden_sets():
        for h in QC.holdout_queries(sig, g["pairs"]):
            isig, x, _ = QC.holdout(sig, h)
            n = isig.shape[0]
            allsig = np.vstack([isig, x[None]])
            pairs = O.candidates_from_sig(allsig, b)
            mine = pairs[(pairs & np.uint64(0xFFFFFFFF)) == np.uint64(n)]      # pairs (i, x): x is the last id
            ids = (mine >> np.uint64(32)).astype(np.int64)
            assert np.array_equal(QC.restate_candidates(isig, b, x), ids), (name, h)
            if len(ids):
                want = O.score_pairs(allsig, mine)
                assert np.array_equal(QC.restate_scores(isig, ids, x), want), (name, h)
                src, dst, val = O.topk(mine, want, K)
                sel = src == n
                (got_ids, got_m, avail), = QC.restate_probe(isig, b, x, K)
                assert np.array_equal(got_ids, dst[sel]) and np.array_equal(got_m, val[sel]), (name, h)
                assert avail == len(ids)


def test_restatement_equals_the_reference_on_held_out_queries():
    """candidates = the golden pairs that involve the held-out query; lists = the golden top-K list (tie-aware)"""
    seen_lonely = seen_list = 0
    for name, g, sig, b, K in QC.golden_sets():
        for h in QC.holdout_queries(sig, g["pairs"]):
            isig, x, remap = QC.holdout(sig, h)
            want = QC.golden_candidates(g["pairs"], h, remap)
            assert np.array_equal(QC.restate_candidates(isig, b, x), want), (name, h)
            seen_lonely += len(want) == 0
            if "qs_q" in g:
                ref = QC.golden_list(g, h, remap)
                (ids, mi, avail), = QC.restate_probe(isig, b, x, K)
                if ref is None:
                    assert avail == 0
                else:
                    QC.check_list_tie_aware(ids, mi, *ref)
                    seen_list += 1
    assert seen_lonely >= 3 and seen_list >= 20


def test_lsh_edge_int16_wrap_and_empty_bands():
    g = load("lsh_edge")
    sig = (np.asarray(g["sig"]).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    b = int(g["b"])
    for h in range(sig.shape[0]):
        isig, x, remap = QC.holdout(sig, h)
        assert np.array_equal(QC.restate_candidates(isig, b, x), QC.golden_candidates(g["pairs"], h, remap)), h


# ---------------------------------------------------------------------------------------------- column prediction
def column_case(seed=11, nu=400, nq=2000, tu=24, tq=60):
    """new queries = the target lists of a predict_cases case (knife-edge query-only cells for the target users)"""
    c = PC.build_case(seed, nu=nu, nq=nq, tu=tu, tq=tq)
    lists = [c.qs[j] for j in range(tq) if j in c.qs]
    knife = [(int(i), js) for (i, j), br in zip(c.knife, c.branch) if br == "q"
             for js in [[jj for jj in range(tq) if jj in c.qs].index(int(j))]]
    return c, lists, knife


def restate_columns(ratings, lists, summation=O.np_sum_order, weights=(0.6, 0.4, 60)):
    """oracle.predict_cells over the matrix with one zero column appended per new query -> int64 [m][nu]"""
    nu, nq = ratings.shape
    m = len(lists)
    app = np.hstack([ratings, np.zeros((nu, m), dtype=ratings.dtype)])
    qs = {nq + x: {"indexes": np.asarray(l["indexes"]), "values": np.asarray(l["values"])} for x, l in enumerate(lists)}
    us = {u: {"indexes": np.zeros(0, dtype=np.int64), "values": np.zeros(0)} for u in range(nu)}
    cells = np.array([(u, nq + x) for x in range(m) for u in range(nu)], dtype=np.int64)
    out = O.predict_cells(app, qs, us, cells, summation, *weights)
    return out.reshape(m, nu)


def _qp_blend(row, lst, summation, fma=False, floor_round=False):
    qp = O.weighted_average(row, lst["indexes"], lst["values"], summation)
    if qp == 0:
        return 0
    a, c = O.QUERY_WEIGHT + (O.USER_WEIGHT * 0.5), O.DEFAULT_MEAN * (O.USER_WEIGHT * 0.5)
    v = float(Fraction(qp) * Fraction(a) + Fraction(c)) if fma else qp * a + c
    return int(np.floor(v + 0.5)) if floor_round else round(v)


def test_column_restatement_is_the_query_only_blend():
    c, lists, _ = column_case()
    want = restate_columns(c.ratings, lists)
    for x, l in enumerate(lists):
        for u in range(c.nu):
            assert want[x, u] == _qp_blend(c.ratings[u], l, O.np_sum_order)


def test_knife_cells_tell_order_rounding_and_fma_apart():
    """oracle only: the knife cells of the new columns change under the other summation order, under round-half-up
    and under one FMA in the blend"""
    c, lists, knife = column_case()
    assert len(knife) >= 100
    flips = {"order": 0, "floor": 0, "fma": 0}
    for u, x in knife:
        r = _qp_blend(c.ratings[u], lists[x], O.np_sum_order)
        flips["order"] += _qp_blend(c.ratings[u], lists[x], PC.sequential_sum) != r
        flips["floor"] += _qp_blend(c.ratings[u], lists[x], O.np_sum_order, floor_round=True) != r
        flips["fma"] += _qp_blend(c.ratings[u], lists[x], O.np_sum_order, fma=True) != r
    assert min(flips.values()) >= 5, flips


# ---------------------------------------------------------------------------------------------- C ABI, no device
def _fake(n):
    return [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(n)]


def test_abi_argument_checks_without_a_device():
    from qrlsh import _lib
    lib = _lib.load()
    E = _lib.QRLSH_EINVAL
    k, kt, i, it, d, ws = _fake(6)
    assert lib.qrlsh_index_build(k, kt, i, it, -1, 4, d, ws, 1 << 20, None) == E
    assert lib.qrlsh_index_build(k, kt, i, it, 2**32, 4, d, ws, 1 << 20, None) == E
    assert lib.qrlsh_index_build(k, kt, i, it, 100, 0, d, ws, 1 << 20, None) == E
    assert lib.qrlsh_index_build(k, kt, i, it, 100, 4, None, ws, 1 << 20, None) == E
    assert lib.qrlsh_index_build(None, kt, i, it, 100, 4, d, ws, 1 << 20, None) == E
    assert lib.qrlsh_index_build(k, kt, i, it, 4096, 2, d, ws, 1, None) == _lib.QRLSH_EWORKSPACE
    pk, tot = _fake(2)
    need = lib.qrlsh_index_probe_workspace_bytes(10, 4)
    assert lib.qrlsh_index_probe_count(k, d, 100, 4, 2, pk, 10, ws, need, None, None) == E        # no total_out
    assert lib.qrlsh_index_probe_count(k, d, 100, 4, 0, pk, 10, ws, need, tot, None) == E        # r = 0
    assert lib.qrlsh_index_probe_count(k, d, 100, 4, 2, pk, -1, ws, need, tot, None) == E
    assert lib.qrlsh_index_probe_count(k, d, 100, 4, 2, pk, 2**31, ws, 2**62, tot, None) == E     # m * b >= 2^32
    assert lib.qrlsh_index_probe_count(k, d, 100, 4, 2, None, 10, ws, need, tot, None) == E
    assert lib.qrlsh_index_probe_count(k, d, 100, 4, 2, pk, 10, ws, need - 1, tot, None) == _lib.QRLSH_EWORKSPACE
    assert lib.qrlsh_index_probe_fill(k, None, d, 100, 4, 2, pk, 10, ws, need, None, None) == E
    assert lib.qrlsh_index_probe_fill(k, i, d, 100, 4, 2, pk, 10, ws, need - 1, tot, None) == _lib.QRLSH_EWORKSPACE
    s, n2, ps, pn, pw, raw, off, ix, mi, av = _fake(10)
    fneed = lib.qrlsh_index_finish_workspace_bytes(10, 16, 50)

    def fin(K=16, n=100, m=10, n_raw=50, P=24, b=4, dtype=0, off_=off, ws_bytes=fneed, idx=ix):
        return lib.qrlsh_index_probe_finish(s, n2, n, ps, pn, dtype, P, b, m, pw, raw, n_raw, K, off_, idx, mi, av, ws,
                                            ws_bytes, None)
    for K in (0, 257, -1):
        assert fin(K=K) == E and b"K=" in lib.qrlsh_last_error()
    assert fin(P=25) == E                        # P % b
    assert fin(dtype=2) == E
    assert fin(off_=None) == E
    assert fin(idx=None) == E
    assert fin(n_raw=-1) == E
    assert fin(ws_bytes=fneed - 1) == _lib.QRLSH_EWORKSPACE
    # predict_columns
    r, o, x, mm, out, fl = _fake(6)
    pc = lib.qrlsh_predict_columns
    assert pc(r, 4, 10, o, x, mm, 2, 0.6, 0.4, 60.0, 2, out, fl, None) == E                   # sum order
    assert pc(r, 4, 10, o, x, mm, 2, 0.6, 0.4, 60.0, 0, out, None, None) == E                 # flags required
    assert pc(r, -1, 10, o, x, mm, 2, 0.6, 0.4, 60.0, 0, out, fl, None) == E
    assert pc(r, 65535 * 256 + 1, 10, o, x, mm, 2, 0.6, 0.4, 60.0, 0, out, fl, None) == E
    with pytest.raises(_lib.QrlshError):
        _lib.check(fin(K=0))


def test_abi_sizes():
    from qrlsh import _lib
    lib = _lib.load()
    assert lib.qrlsh_index_dir_bits(0) == 1 and lib.qrlsh_index_dir_bits(10**7) == 21
    assert lib.qrlsh_index_dir_bits(2**40) == 26
    for n in (1, 100, 10**6, 10**7):
        d = lib.qrlsh_index_dir_bits(n)
        assert lib.qrlsh_index_dir_words(n, 32) == 32 * (2**d + 1)
        assert 2**d <= max(n, 2)               # at least ~4 records per directory word past tiny sizes
    assert lib.qrlsh_index_probe_workspace_bytes(0, 4) == 0
    assert lib.qrlsh_index_probe_workspace_bytes(10, 4) >= 41 * 8
    assert lib.qrlsh_index_finish_workspace_bytes(10, 0, 5) == 0
    assert lib.qrlsh_index_finish_workspace_bytes(10, 257, 5) == 0
    assert lib.qrlsh_index_finish_workspace_bytes(10, 16, 100) > lib.qrlsh_index_finish_workspace_bytes(10, 16, 5)
    assert lib.qrlsh_index_build_workspace_bytes(4096, 2) == lib.qrlsh_sort_workspace_bytes(4096, 2)


# ---------------------------------------------------------------------------------------------- host layer
def test_query_index_rejects_bad_arguments_before_the_device():
    import torch
    from qrlsh.index import QueryIndex
    with pytest.raises(TypeError):
        QueryIndex(np.zeros((4, 12), dtype=np.int32), None, 3)               # not a tensor
    with pytest.raises(TypeError):
        QueryIndex(torch.zeros((4, 12), dtype=torch.float32), None, 3)
    with pytest.raises(TypeError):
        QueryIndex(torch.zeros((12,), dtype=torch.int32), None, 3)            # not 2-D
    # the checks that need a constructed index, on one built without touching a device
    qi = QueryIndex.__new__(QueryIndex)
    qi.sig, qi.n, qi.P, qi.b, qi.r, qi.K, qi.table = torch.zeros((5, 12), dtype=torch.int32), 5, 12, 3, 4, 3, None
    for K in (0, 257, 2.5, True, "3"):
        with pytest.raises(ValueError):
            qi.neighbours(torch.zeros((2, 12), dtype=torch.int32), K=K)
    with pytest.raises(ValueError):
        qi.neighbours(torch.zeros((2, 10), dtype=torch.int32))                # wrong P
    with pytest.raises(TypeError):
        qi.neighbours(np.zeros((2, 12), dtype=np.int32))
    with pytest.raises(ValueError):
        qi.signatures(None, None)                                             # no table
    e = torch.zeros((0,), dtype=torch.int32)
    with pytest.raises(ValueError):
        qi.predict_columns(np.zeros((3, 5), dtype=np.int32), e, e, e, sum_order="tree")
    with pytest.raises(ValueError):
        qi.predict_columns(np.zeros((3, 4), dtype=np.int32), e, e, e)         # columns != n
    with pytest.raises(ValueError):
        qi.predict_columns(np.zeros((3, 5), dtype=np.float64), e, e, e)
    with pytest.raises(ValueError):
        qi.predict_columns(np.full((3, 5), 2**40), e, e, e)
    with pytest.raises(ValueError):
        qi.predict_columns(np.zeros((3, 5), dtype=np.int32), np.zeros(2), e, e)
    with pytest.raises(ValueError):
        QueryIndex.top_users(np.zeros((2, 3), dtype=np.int32), 3)


def test_recommender_new_query_methods_need_a_run():
    import recommender
    rec = recommender.Recommender()
    rec.datasetFeatures = ["a", "b"]
    for call in (lambda: rec.similar_queries([["x", ""]]), lambda: rec.predict_new_queries([["x", ""]]),
                 lambda: rec.recommend_new_queries([["x", ""]], 3)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        rec.recommend_new_queries([["x", ""]], 0)
