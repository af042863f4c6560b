"""The user-similarity step on the device (csrc/users.hip, qrlsh/users.py) against tests/users_cases.py: the column
statistics exactly, the matrix-core Gram entry by entry inside a derived rounding bound at every tile, step and slice
edge, the PCA features by the distances BIRCH reads, and the pairs, scores and lists of the clusters exactly under
labels of every kind (-1, the two ends of int64, neighbours in one bit).  The kernels write into NaN-filled buffers
between guard pads; nothing is compared with itself."""
import functools

import numpy as np
import pytest
import torch

import users_cases as UC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402,F401
from qrlsh import _lib, ops, users  # noqa: E402
from qrlsh.ops import _ptr  # noqa: E402
from qrlsh.userlists import UserLists  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
PAD = 64          # float64 words before and behind every output


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)           # (a copy: the cases are read-only)


def _padded(n):
    buf = torch.full((PAD + n + PAD,), float("nan"), dtype=torch.float64, device=DEV)
    return buf, ops._vp(buf.data_ptr() + 8 * PAD)


def _middle(buf, n):
    b = buf.cpu().numpy()
    assert np.isnan(b[:PAD]).all() and np.isnan(b[PAD + n:]).all(), "written before or behind the output"
    return b[PAD:PAD + n]


@functools.lru_cache(maxsize=None)
def device_gram(case):
    """qrlsh_user_gram through the C ABI on a case of users_cases: outputs and workspace pre-filled with NaN, so an
    entry or a partial sum that no workgroup writes cannot pass.  -> (mean, inv_scale, gram) on the host"""
    lib = _lib.load()
    r, _ = UC.gram_case(*case)
    nu, nq = r.shape
    rd = dev(r)
    mb, mp = _padded(nq)
    ib, ip = _padded(nq)
    gb, gp = _padded(nu * nu)
    nbytes = int(lib.qrlsh_user_gram_workspace_bytes(nu, nq))
    assert nbytes == UC.slices_of(nq) * nu * nu * 8
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.qrlsh_user_gram(_ptr(rd), nu, nq, mp, ip, gp, _ptr(ws), nbytes, ops._stream()))
    torch.cuda.synchronize()
    out = _middle(mb, nq), _middle(ib, nq), _middle(gb, nu * nu).reshape(nu, nu)
    # the library's own wrapper (uninitialised outputs, its own workspace) gives the same bits
    mean, inv, gram = users.standardized_gram(rd)
    for a, b in zip(out, (mean, inv, gram)):
        assert np.array_equal(a, b.cpu().numpy())
    return out


# --------------------------------------------------------------------------------------------- 1. column statistics
@pytest.mark.parametrize("case", UC.GRAM_CASES, ids=UC.case_id)
def test_column_statistics_equal_the_restated_standard_scaler(case):
    """mean bit for bit, 1 / inv_scale within rtol = 1e-15 of scikit-learn's scale (tests/test_users_host.py holds the
    restatement to StandardScaler bit for bit), from 1 and 2 rows on, with constant, all-zero, single-entry and
    alternating columns, and on values up to 10^6 with negative ones"""
    _, ref = UC.gram_case(*case)
    mean, inv, _ = device_gram(case)
    UC.check_stats(mean, inv, ref)
    const = ref[1] == 1.0
    assert np.array_equal(inv[const], np.ones(int(const.sum())))


# ------------------------------------------------------------------------------------------------------ 2. the Gram
@pytest.mark.parametrize("case", UC.GRAM_CASES, ids=UC.case_id)
def test_gram_matches_the_products_entry_by_entry(case):
    """G against z z^T with z = (x - mean) * inv formed in numpy from the device's own (checked) statistics: every
    entry within 2 g S of the float64 product and the rows {0, 1, 63, 64, 127, 128, last} within g S of a longdouble
    product, g = n u / (1 - n u), n = nq + 16, S = sum |z_i| |z_j| -- a bound that holds for any order of the sums, so
    one missing, doubled or misplaced term (0.2 and more against a tolerance below 1e-6) cannot pass; exactly
    symmetric; [[0]] for a single user.  Shapes: 1, 2, 127, 128, 129 and 257 users (three tiles, the pair (0, 2), a
    last tile of one row), fewer columns than a step, and both sides of the 4- and 16-slice thresholds."""
    r, ref = UC.gram_case(*case)
    mean, inv, gram = device_gram(case)
    UC.check_stats(mean, inv, ref)
    w64, wld = UC.check_gram(gram, UC.standardized(r, mean, inv))
    print("gram %s: largest error %.3g of the float64 bound 2 g S, %.3g of the longdouble bound g S"
          % (UC.case_id(case), w64, wld))
    if r.shape[0] == 1:
        assert np.array_equal(gram, [[0.0]])


# ------------------------------------------------------------------------------------------------- 3. PCA features
@pytest.mark.parametrize("shape", UC.PCA_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pca_features_give_scikit_learns_distances(shape):
    """users.pca_features against StandardScaler + PCA(svd_solver="full"): shape, components by descending variance,
    all pairwise distances within rtol = 1e-7, atol = 1e-6; two users, fewer columns than users (k = nq), k cut to 200,
    four column slices"""
    r, _ = UC.gram_case(*shape)
    f = users.pca_features(dev(r), DEV)
    assert f.dtype == torch.float64 and f.is_cuda
    err = UC.check_pca(f.cpu().numpy(), r, UC.pca_reference(r))
    print("pca %dx%d: largest distance error %.3g" % (shape + (err,)))


# ------------------------------------------------------------------ 4. cluster pairs, scores and lists by any label
@functools.lru_cache(maxsize=None)
def label_refs():
    r, labels = UC.label_case()
    K = UC.max_candidates(r.shape[0])
    pairs = UC.pairs_ref(labels)
    return r, labels, K, pairs, UC.scores_ref(r, pairs), UC.lists_ref(r, labels, K)


def _dense(ul):
    torch.cuda.synchronize()
    return ul.idx.cpu().numpy(), ul.milli.cpu().numpy(), ul.len.cpu().numpy()


def test_cluster_pairs_and_scores_are_exact_under_every_kind_of_label():
    """every u < v of every cluster -- the one labelled -1 (the bucket machinery's reserved key), the two ends of
    int64, labels that differ in bit 0 or bit 62 only, clusters of 1, 2, 17 and 300 -- with the score of the truncated
    centred rows; host labels, device labels and a relabelling of the same partition give the same arrays"""
    r, labels, K, pairs, milli, _ = label_refs()
    got_p, got_m = users.cluster_pair_scores(r, labels, DEV)
    assert got_p.dtype == torch.int64 and got_m.dtype == torch.int32
    gp = got_p.cpu().numpy()
    missing = np.setdiff1d(pairs, gp)
    assert missing.size == 0, "no pairs for the clusters labelled %s" % np.unique(labels[missing >> 32]).tolist()
    assert np.array_equal(gp, pairs) and np.array_equal(got_m.cpu().numpy(), milli)
    dp, dm = users.cluster_pair_scores(dev(r), torch.from_numpy(labels.copy()).to(DEV), DEV)
    assert torch.equal(dp, got_p) and torch.equal(dm, got_m)
    plain = np.unique(labels, return_inverse=True)[1].astype(np.int64) * 3 + 11       # labels that always worked
    pp, pm = users.cluster_pair_scores(r, plain, DEV)
    assert torch.equal(pp, got_p) and torch.equal(pm, got_m)
    # the centred rows behind the scores: truncation toward zero, zeros in the three padding columns
    c = users.center_rows(dev(r)).cpu().numpy()
    assert c.shape == (UC.LABEL_NU, 40) and not c[:, UC.LABEL_NQ:].any()
    assert np.array_equal(c[:, :UC.LABEL_NQ], UC.centred(r))


@pytest.mark.filterwarnings("ignore:Mean of empty slice", "ignore:invalid value encountered")   # the oracle's mean of an unrated row
def test_user_similarities_and_build_give_the_lists_of_every_cluster():
    r, labels, K, _, _, lists = label_refs()
    nu = r.shape[0]
    src, dst, val = users.user_similarities(r, labels, K, DEV)
    got = UC.dense_from_coo(src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy(), nu, K)
    UC.assert_lists(got, lists, "user_similarities")
    assert got[2][labels == -1].max() == K and got[2][labels == UC.I64_MIN].min() > 0
    UC.check_user_sims_tie_aware(users.sims_to_dict(src, dst, val, nu), O.user_similarities_from_labels(r, labels), K)
    ul = UserLists.build(r, labels, K)
    UC.assert_lists(_dense(ul), lists, "UserLists.build")
    assert np.array_equal(ul.user_labels(), labels)
    s2, d2, v2 = ul.coo()
    assert torch.equal(s2, src) and torch.equal(d2, dst) and torch.equal(v2, val)


def test_add_users_with_labels_minus_one_and_int64_max_ends_as_a_fresh_build():
    """the users labelled -1 and 2^63 - 1 join a UserLists built without them: the lists end element for element as a
    fresh build over all rows gives them, and as numpy does"""
    base, base_labels, rows, row_labels = UC.add_users_case()
    K = UC.max_candidates(UC.LABEL_NU)
    ul = UserLists.build(base, base_labels, K)
    UC.assert_lists(_dense(ul), UC.lists_ref(base, base_labels, K), "build without the two clusters")
    assert np.array_equal(ul.add_users(rows, labels=row_labels), row_labels)
    new, new_labels = np.concatenate((base, rows)), np.concatenate((base_labels, row_labels))
    assert np.array_equal(ul.user_labels(), new_labels)
    want = UC.lists_ref(new, new_labels, K)
    assert want[2][new_labels == -1].max() == K
    UC.assert_lists(_dense(ul), want, "add_users")
    UC.assert_lists(_dense(UserLists.build(new, new_labels, K)), want, "fresh build")
    src, dst, val = users.user_similarities(new, ul.user_labels(), K, DEV)
    a, b, c = ul.coo()
    assert torch.equal(a, src) and torch.equal(b, dst) and torch.equal(c, val)


# ---------------------------------------------------------------------------------------- 6. what belongs with it
def test_no_columns_and_a_single_user_give_empty_lists():
    for ratings, labels in ((np.zeros((5, 0), dtype=np.int64), np.array([-1, -1, 0, 0, 0])),
                            (np.array([[3, 0, 5, 100]]), np.array([-1])),
                            (np.array([[3, 0, 5, 100]]), np.array([4]))):
        out = users.user_similarities(ratings, labels, device=DEV)
        assert len(out) == 3 and all(t.dtype == torch.int32 and t.numel() == 0 and t.is_cuda for t in out)
    p, m = users.cluster_pair_scores(np.array([[3, 0, 5, 100]]), np.array([-1]), DEV)
    assert p.numel() == 0 and m.numel() == 0 and m.dtype == torch.int32
