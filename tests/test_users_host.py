"""The references and checkers of the user-similarity step, on the host (tests/users_cases.py): the restated column
statistics equal scikit-learn's bit for bit, the Gram checker passes the reference and rejects four planted defects,
the Gram route to the PCA features gives scikit-learn's distances, the numpy pairs, scores and lists agree with the
oracle on labels of every kind, and the two C entry points refuse bad sizes before any device work.  No GPU."""
import ctypes

import numpy as np
import pytest

import users_cases as UC

STATS_CASES = UC.GRAM_CASES + [(nu, nq, False) for nu, nq in UC.PCA_SHAPES] + [(1, 1, False), (385, 1000, False)]


# --------------------------------------------------------------------------------------------- 1. column statistics
@pytest.mark.parametrize("case", STATS_CASES, ids=UC.case_id)
def test_stats_ref_equals_standard_scaler_bit_for_bit(case):
    from sklearn.preprocessing import StandardScaler
    r, (mean, scale) = UC.gram_case(*case)
    nu, nq = r.shape
    sc = StandardScaler().fit(r)
    assert np.array_equal(mean, sc.mean_) and np.array_equal(scale, sc.scale_)
    cols = UC.planted_columns(nq)
    assert bool(cols) == (nq >= 4) and len(set(cols)) == len(cols)
    if cols:
        assert (r[:, cols[0]] == 7).all() and mean[cols[0]] == 7.0 and scale[cols[0]] == 1.0
        assert (r[:, cols[1]] == 0).all() and mean[cols[1]] == 0.0 and scale[cols[1]] == 1.0
        assert np.count_nonzero(r[:, cols[2]]) == 1
        assert set(r[:, cols[3]].tolist()) <= {0, 100}
        if nu >= 2:
            assert scale[cols[2]] != 1.0 and scale[cols[3]] != 1.0
        if nu % 2 == 0:
            assert mean[cols[3]] == 50.0 and scale[cols[3]] == 50.0
    if nu == 1:
        assert (scale == 1.0).all() and np.array_equal(mean, r[0].astype(np.float64))
    if case[2]:
        assert r.max() > 500_000 and (r < 0).sum() > 10


# ------------------------------------------------------------------------------------------------------ 2. the Gram
def test_the_gram_cases_are_the_shapes_that_take_another_path():
    shapes = {(nu, nq) for nu, nq, _ in UC.GRAM_CASES}
    assert {nq for nu, nq in shapes if nu == 129} == set(UC.GRAM_NQ)
    for nq in (33, 4097):
        assert {nu for nu, q in shapes if q == nq} == set(UC.GRAM_NU)
    assert (257, 65537) in shapes and len(UC.GRAM_CASES) == 22 and sum(big for _, _, big in UC.GRAM_CASES) == 1
    assert [UC.slices_of(nq) for nq in (4095, 4096, 65535, 65536)] == [1, 4, 4, 16]
    for nq in UC.GRAM_NQ:           # every slice starts inside the matrix; past the thresholds the last one is short
        ns, sc = UC.slices_of(nq), UC.slice_cols_of(nq)
        assert sc % UC.GR_K == 0 and (ns - 1) * sc < nq <= ns * sc
    assert UC.slice_cols_of(4097) == 1056 and 4097 - 3 * 1056 < 1056
    assert UC.sampled_rows(1) == [0] and UC.sampled_rows(129) == [0, 1, 63, 64, 127, 128]
    assert UC.sampled_rows(257) == [0, 1, 63, 64, 127, 128, 256]


@pytest.mark.parametrize("case", UC.GRAM_CASES, ids=UC.case_id)
def test_check_gram_passes_the_reference_products(case):
    """numpy's float64 product, whole and slice by slice, stays inside the derived bound with room -- the references
    alone do not use the tolerance up"""
    r, (mean, scale) = UC.gram_case(*case)
    z = UC.standardized(r, mean, 1.0 / scale)
    G = z @ z.T
    w64, wld = UC.check_gram(np.triu(G) + np.triu(G, 1).T, z)
    assert w64 <= 0.25 and wld <= 0.25
    w64, wld = UC.check_gram(UC.gram_by_slices(z), z)
    assert w64 <= 0.25 and wld <= 0.25
    if r.shape[0] == 1:
        assert np.array_equal(UC.gram_by_slices(z), [[0.0]])


@pytest.mark.parametrize("kind", UC.DEFECTS)
def test_check_gram_rejects_a_planted_defect(kind):
    z, G = UC.defect_case(kind)
    assert np.array_equal(G, G.T) and np.isfinite(G).all()       # only the values give the defect away
    with pytest.raises(AssertionError, match="bounds from"):
        UC.check_gram(G, z)


def test_check_gram_rejects_unwritten_and_unsymmetric_entries():
    r, (mean, scale) = UC.gram_case(129, 33)
    z = UC.standardized(r, mean, 1.0 / scale)
    G = UC.gram_by_slices(z)
    UC.check_gram(G, z)
    bad = G.copy()
    bad[128, 128] = np.nan
    with pytest.raises(AssertionError, match="finite"):
        UC.check_gram(bad, z)
    bad = G.copy()
    bad[3, 128] = np.nextafter(bad[3, 128], np.inf)
    with pytest.raises(AssertionError, match="symmetric"):
        UC.check_gram(bad, z)
    # the constant columns carry nothing: two users that differ only there have the same row of G
    c7 = UC.planted_columns(33)[0]
    assert (z[:, c7] == 0).all()


# ------------------------------------------------------------------------------------------------- 3. PCA features
@pytest.mark.parametrize("shape", UC.PCA_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gram_route_gives_scikit_learns_distances(shape):
    r, (_, scale) = UC.gram_case(*shape)
    nu, nq = shape
    err = UC.check_pca(UC.pca_from_gram(r), r, UC.pca_reference(r))
    # Where every kept component has a real eigenvalue the route leaves the tolerance unused.  Where k exceeds the rank
    # of the standardized matrix (centring takes one dimension, each constant column another) the kept null eigenvalues
    # are rounding noise of size eps * lambda_max, and the square root turns it into ~1e-7 of feature: users with
    # equal rows then lie ~3e-8 apart instead of 0, which is what the absolute part of the tolerance is for
    rank = min(nu - 1, int((scale != 1.0).sum()))
    assert err < (1e-10 if min(nu, nq, 200) <= rank else 1e-6)


# ------------------------------------------------------------------ 4. cluster pairs, scores and lists by any label
def test_label_case_holds_what_it_says():
    r, labels = UC.label_case()
    assert r.shape == (UC.LABEL_NU, UC.LABEL_NQ) and (UC.LABEL_NQ + 3) // 4 * 4 - UC.LABEL_NQ == 3
    vals, counts = np.unique(labels, return_counts=True)
    assert dict(zip(vals.tolist(), counts.tolist())) == dict(UC.LABEL_SIZES)
    assert {1, 2, 17, 300} <= set(counts.tolist()) and dict(UC.LABEL_SIZES)[-1] >= 17
    assert labels.dtype == np.int64 and labels.min() == -2 ** 63 and labels.max() == 2 ** 63 - 1
    assert 1000 ^ 1001 == 1 and 5 ^ (5 + 2 ** 62) == 1 << 62
    assert UC.max_candidates(UC.LABEL_NU) == 16                   # the cluster of 17: every other member, uncut
    assert not r[0].any() and np.count_nonzero(r[1]) == 1 and r[2].tolist()[:4] == [1, 2, 2, 0] and not r[2, 3:].any()
    c = UC.centred(r)
    assert not c[2].any() and not c[1].any() and not c[0].any()
    assert np.floor(r[2, :3] - 5 / 3).tolist() == [-1.0, 0.0, 0.0]   # floor would have left a norm
    assert labels[0] == labels[2] == -1 and labels[1] == 0


@pytest.mark.filterwarnings("ignore:Mean of empty slice", "ignore:invalid value encountered")   # the oracle's mean of an unrated row
def test_numpy_references_agree_with_the_oracle_on_every_kind_of_label():
    from oracle import oracle as O
    r, labels = UC.label_case()
    nu = r.shape[0]
    K = UC.max_candidates(nu)
    pairs = UC.pairs_ref(labels)
    u, v = pairs >> 32, pairs & 0xFFFFFFFF
    assert (u < v).all() and (np.diff(pairs) > 0).all() and (labels[u] == labels[v]).all()
    assert pairs.size == sum(n * (n - 1) // 2 for _, n in UC.LABEL_SIZES)
    assert (labels[u] == -1).sum() == 40 * 39 // 2
    milli = UC.scores_ref(r, pairs)
    assert np.array_equal(milli, UC.scores_ref(r, pairs, product_last=True))
    assert milli.min() < 0 < milli.max() <= 1000 and (milli[(u == 0) | (u == 1) | (u == 2)] == 0).all()
    # the scores against scikit-learn's cosine of the oracle's own centred block, pair by pair
    from sklearn.metrics.pairwise import cosine_similarity
    sim = np.around(cosine_similarity(UC.centred(r)), 3)
    assert np.array_equal(milli.astype(np.float64) / 1000.0, sim[u, v])
    lists = UC.lists_ref(r, labels, K)
    ref = O.user_similarities_from_labels(r, labels)
    UC.check_user_sims_tie_aware(UC.lists_to_dict(lists), ref, K)
    assert lists[2][labels == -1].max() == K and (lists[2][labels == 1000] == 0).all()
    assert (lists[2][labels == UC.I64_MIN] <= 16).all() and lists[2][labels == UC.I64_MIN].max() > 3
    # a dropped cluster does not pass
    dropped = tuple(a.copy() for a in lists)
    dropped[0][labels == -1], dropped[1][labels == -1], dropped[2][labels == -1] = -1, 0, 0
    with pytest.raises(AssertionError):
        UC.check_user_sims_tie_aware(UC.lists_to_dict(dropped), ref, K)
    # the dense form and the COO form are one another's inverse
    idx, mil, ln = lists
    keep = np.arange(K)[None, :] < ln[:, None]
    src = np.repeat(np.arange(nu), ln)
    UC.assert_lists(UC.dense_from_coo(src, idx[keep], mil[keep], nu, K), lists, "round trip")


def test_add_users_case_moves_two_clusters_out_and_back():
    r, labels = UC.label_case()
    base, base_labels, rows, row_labels = UC.add_users_case()
    assert rows.shape[0] == 42 and set(row_labels.tolist()) == {-1, UC.I64_MAX}
    assert not (set(base_labels.tolist()) & {-1, UC.I64_MAX}) and base.shape[0] + rows.shape[0] == r.shape[0]


# ---------------------------------------------------------------------------------------- 6. what belongs with it
def test_user_gram_and_center_rows_refuse_bad_sizes_before_any_device_work():
    from qrlsh import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float64)             # host memory: every call below returns before it is touched
    p = ctypes.c_void_p(buf.ctypes.data)
    for nu, nq in ((0, 5), (5, 0), (5, 2 ** 24 + 1), (2 ** 20, 5), (-1, 5), (5, -1)):
        assert lib.qrlsh_user_gram(p, nu, nq, p, p, p, p, 1 << 40, None) == _lib.QRLSH_EINVAL, (nu, nq)
        assert b"qrlsh_user_gram" in lib.qrlsh_last_error()
    assert lib.qrlsh_user_gram(None, 5, 5, p, p, p, p, 1 << 40, None) == _lib.QRLSH_EINVAL
    for nu, nq in ((5, 7), (129, 4096), (2, 65536), (2 ** 20 - 1, 2 ** 24)):
        need = lib.qrlsh_user_gram_workspace_bytes(nu, nq)
        assert lib.qrlsh_user_gram(p, nu, nq, p, p, p, p, need - 1, None) == _lib.QRLSH_EWORKSPACE, (nu, nq)
        assert b"workspace" in lib.qrlsh_last_error()
    assert not buf.any()
    assert lib.qrlsh_center_rows(p, 5, 8, 7, p, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_center_rows(p, 5, 8, 4, p, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_center_rows(p, -1, 8, 8, p, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_center_rows(None, 0, 8, 8, None, None) == _lib.QRLSH_OK       # nothing to do
    for nu in (1, 129, 2000):
        for nq, slices in ((1, 1), (4095, 1), (4096, 4), (4097, 4), (65535, 4), (65536, 16), (65537, 16), (2 ** 24, 16)):
            assert UC.slices_of(nq) == slices
            assert lib.qrlsh_user_gram_workspace_bytes(nu, nq) == slices * nu * nu * 8, (nu, nq)


def test_max_candidates_and_the_matrix_without_columns():
    import math
    import torch
    from qrlsh import users
    assert [users.max_candidates(nu) for nu in (1, 2, 3, 100, 2000)] == [0, 2, 3, 11, 19]
    for nu in (1, 2, 3, 100, 2000):
        assert users.max_candidates(nu) == round(math.log(nu, 1.5)) == UC.max_candidates(nu)
    # no columns: nobody is similar, and no kernel runs
    out = users.user_similarities(np.zeros((5, 0), dtype=np.int64), np.zeros(5, dtype=np.int64), device="cpu")
    assert all(t.dtype == torch.int32 and t.numel() == 0 for t in out) and len(out) == 3
