"""List fidelity (qrlsh.edge_overlaps / list_fidelity, Recommender.list_fidelity): what needs no device.  The restatement
the GPU tests hold the kernels to is itself held to a second form, the cases to what makes them worth running; then
Python's argument checks, ListFidelity's ratios, the seeded sample and the exported group rule."""
import math
import os
import re

import numpy as np
import pytest

import fidelity_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FC.LSH_SHAPES, ids=lambda s: "n%d" % s["n"])
def test_restatement_against_dense_form_on_real_lists(shape):
    case = FC.lsh_case(**shape)
    ref = case.ref()
    FC.assert_lsh_case_is_telling(case, ref)
    FC.same_result(FC.fidelity_dense(case.offsets, case.rows, case.D, case.src, case.dst, case.nq, case.K), ref)
    print(case.name, dict(zip(FC.WORDS, ref["totals"].tolist())))


@pytest.mark.parametrize("D", [31, 32, 33, 200])
def test_restatement_against_dense_form_on_planted_lists(D):
    case = FC.planted_case(D)
    ref = case.ref()
    FC.assert_planted_case_is_telling(case, ref)
    FC.same_result(FC.fidelity_dense(case.offsets, case.rows, case.D, case.src, case.dst, case.nq, case.K), ref)
    chosen = [0, case.nq - 1, 7, 0, 8]
    for K in (1, 2, 64):
        sub = case.ref(chosen, K)
        FC.same_result(FC.fidelity_dense(case.offsets, case.rows, case.D, case.src, case.dst, case.nq, K, chosen), sub)
        assert np.array_equal(sub["words"][0], sub["words"][3])          # a repeated request repeats its words
        assert (sub["words"][:, 0] <= K).all()
    # query 0 at K = 3: five exact duplicates tie at J = 1 -- three of the listed ones are hits, none is sure
    w = dict(zip(FC.WORDS, ref["words"][0].tolist()))
    assert (w["listed"], w["hits"], w["sure"], w["disjoint"]) == (3, 2, 0, 1) and ref["equal"][0, 0] == 4


def test_overlap_case_by_hand():
    offsets, rows, src, dst, want = FC.overlap_case()
    sizes = np.diff(offsets)
    same = src == dst
    assert np.array_equal(want[same], sizes[src[same]])                 # src == dst gives |A|
    n = len(sizes)
    assert np.array_equal(want.reshape(n, n), want.reshape(n, n).T)
    assert (want <= np.minimum(sizes[src], sizes[dst])).all()


# ---- Python's checks come before the library is loaded -----------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from qrlsh import _lib

    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def test_argument_checks_precede_the_library(no_library):
    import qrlsh
    off, rows = np.array([0, 1, 2]), np.array([0, 1])
    e = np.zeros(0, dtype=np.int64)
    ok = dict(offsets=off, rows=rows, D=4, q_src=e, q_dst=e, q_milli=e, nq=2, K=3)
    for bad in (dict(K=0), dict(K=65), dict(K=True), dict(K=2.0), dict(nq=-1), dict(nq=3), dict(D=-1), dict(D=(1 << 20) + 1),
                dict(slices=-1), dict(slices=257), dict(queries=[2]), dict(queries=[-1]), dict(queries=[0.5]),
                dict(queries=[[0]]), dict(q_src=[0]), dict(q_dst=[0.5]), dict(offsets=[[0, 1, 2]]), dict(rows=[0.0, 1.0]),
                dict(offsets=[])):
        with pytest.raises(ValueError):
            qrlsh.list_fidelity(**dict(ok, **bad))
    for bad in (dict(src=[0, 1], dst=[0]), dict(src=[0.5], dst=[0]), dict(src=[[0]], dst=[[0]]), dict(offsets=[]),
                dict(rows=[[0, 1]])):
        with pytest.raises(ValueError):
            qrlsh.edge_overlaps(**dict(dict(offsets=off, rows=rows, src=[0], dst=[1]), **bad))


def test_recommender_checks_need_no_device(no_library):
    import recommender as R
    rec = R.Recommender()
    with pytest.raises(ValueError, match="no live lists"):
        rec.list_fidelity()
    with pytest.raises(ValueError, match="no live lists"):
        rec.edge_overlaps()


# ---- ListFidelity ------------------------------------------------------------------------------------------------------
def test_list_fidelity_ratios_and_nans():
    import qrlsh
    words = np.array([[4, 9, 7, 3, 2, 4, 1, 2], [2, 1, 1, 1, 1, 1, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int64)
    ent = {k: np.zeros((3, 64), dtype=np.int32) for k in ("inter", "union", "better", "equal")}
    lf = qrlsh.ListFidelity(4, [5, 0, 5], words, words.sum(axis=0), ent)
    assert lf.K == 4 and lf.queries.tolist() == [5, 0, 5] and lf.per_request.shape == (3, 8) and lf.entries is ent
    assert lf.totals.tolist() == [6, 10, 8, 4, 3, 5, 1, 3] and lf.pairs == 6 + 1
    assert lf.recall == 4 / 5 and lf.sure_recall == 3 / 5 and lf.disjoint_share == 1 / 6 and lf.inversion_share == 3 / 7
    assert "hits=4" in repr(lf)
    none = qrlsh.ListFidelity(4, [], np.zeros((0, 8)), np.zeros(8), ent)
    assert all(math.isnan(v) for v in (none.recall, none.sure_recall, none.disjoint_share, none.inversion_share))
    single = qrlsh.ListFidelity(1, [0], [[1, 3, 2, 1, 1, 1, 0, 0]], [1, 3, 2, 1, 1, 1, 0, 0], ent)
    assert single.recall == 1.0 and single.disjoint_share == 0.0 and math.isnan(single.inversion_share)


# ---- the seeded sample -------------------------------------------------------------------------------------------------
def test_sample_rule():
    import importlib
    from qrlsh import fidelity
    evaluate = importlib.import_module("qrlsh.evaluate")      # (qrlsh.evaluate the attribute is the function)
    xs = [0, 1, 2, 12345, 2**31 - 1, 2**63 + 17, 2**64 - 1]
    assert fidelity.mix64_array(np.array(xs, dtype=np.uint64)).tolist() == [evaluate.mix64(x) for x in xs]
    for nq, sample, seed in ((1000, 64, 0), (1000, 64, 9), (97, 1024, 0), (5, 5, 3), (0, 8, 0), (40, 0, 1)):
        got = fidelity.sample_positions(nq, sample, seed)
        want = sorted(sorted(range(nq), key=lambda p: (evaluate.mix64(seed ^ p), p))[:sample])
        assert got.dtype == np.int64 and got.tolist() == want, (nq, sample, seed)
    a, b = fidelity.sample_positions(1000, 64, 0), fidelity.sample_positions(1000, 64, 9)
    assert a.tolist() != b.tolist() and len(set(a.tolist())) == 64
    # a position's key does not depend on nq: growing nq only lets smaller keys in
    small, big = set(fidelity.sample_positions(500, 64, 0).tolist()), set(a.tolist())
    assert {p for p in big if p < 500} <= small
    for bad in (dict(nq=-1), dict(sample=-1), dict(sample=1.5), dict(seed=-1), dict(seed=2**64)):
        with pytest.raises(ValueError):
            fidelity.sample_positions(**dict(dict(nq=10, sample=4, seed=0), **bad))


# ---- the exported rule and the C surface -------------------------------------------------------------------------------
def test_group_rule():
    """G requests share a workgroup: G bits per table row, 256 words of entries per request and 128 fixed words within the
    160 KiB of LDS of a CU, G the largest power of two up to 32 that fits"""
    from qrlsh import fidelity

    def fits(D, g):
        return (D * g + 31) // 32 + 256 * g + 128 <= 160 * 1024 // 4

    def rule(D):
        return next((g for g in (32, 16, 8, 4, 2) if fits(D, g)), 1)
    steps = FC.group_steps(fidelity.group_size)
    assert [fidelity.group_size(d) for d in steps] == [32, 16, 8, 4, 2] and fidelity.group_size(1 << 20) == 1
    for d in [0, 1, 31, 32, 33, 32768, 1 << 20] + steps + [s + 1 for s in steps]:
        assert fidelity.group_size(d) == rule(d), d
    assert fits(1 << 20, 1)
    assert fidelity.group_size(-1) == 0 and fidelity.group_size((1 << 20) + 1) == 0
    assert fidelity.group_size(32768) >= 10          # "in the tens" at the bench table


def test_c_surface():
    from qrlsh import _lib
    hdr = open(os.path.join(ROOT, "include", "qrlsh.h")).read()
    for name in ("qrlsh_edge_overlaps", "qrlsh_list_fidelity", "qrlsh_list_fidelity_group"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qrlsh_edge_overlaps"][1]) == 9 and len(_lib.SIGNATURES["qrlsh_list_fidelity"][1]) == 18
    assert "#define QRLSH_FIDELITY_MAX_K %d" % _lib.FIDELITY_MAX_K in hdr
    lib = _lib.load()
    # argument errors come back before any device work (there is no device here)
    flag = (np.zeros(1, dtype=np.uint32)).ctypes.data
    assert lib.qrlsh_edge_overlaps(None, None, -1, None, None, 0, None, flag, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_edge_overlaps(None, None, 5, None, None, 0, None, None, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_edge_overlaps(None, None, 5, None, None, 0, None, flag, None) == _lib.QRLSH_OK
    assert lib.qrlsh_edge_overlaps(None, None, 5, None, None, 1 << 36, None, flag, None) == _lib.QRLSH_EINVAL   # null pointers
    tot = np.zeros(8, dtype=np.int64)
    args = dict(nq=5, D=10, m=0, K=3, slices=0)

    def call(**kw):
        a = dict(args, **kw)
        return lib.qrlsh_list_fidelity(None, None, a["nq"], a["D"], None, None, None, a["m"], a["K"], a["slices"], None,
                                       None, None, None, None, tot.ctypes.data, flag, None)
    assert call() == _lib.QRLSH_OK and not tot.any()
    for bad in (dict(K=0), dict(K=65), dict(nq=-1), dict(nq=1 << 31), dict(D=-1), dict(D=(1 << 20) + 1), dict(slices=-1),
                dict(slices=257), dict(m=-1), dict(m=6)):
        assert call(**bad) == _lib.QRLSH_EINVAL, bad
    assert call(m=(1 << 24) + 1, nq=1 << 30) == _lib.QRLSH_EUNSUPPORTED
    assert call(m=1) == _lib.QRLSH_EINVAL            # null pointers, still before any device work
