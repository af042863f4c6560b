"""The live user lists on the device (csrc/userlists.hip, qrlsh.UserLists, Recommender.rate): every check is exact.
The pair kernel is held bit for bit to the route that existed before (center_rows + row_norms + score_pairs) and to
numpy; rate() element for element to a full recompute on the device (users.user_similarities over the edited matrix),
to the numpy lists and to the restated update rule (tests/user_lists_cases.py) -- never to itself."""
import ctypes

import numpy as np
import pytest
import torch

import user_lists_cases as UC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib, ops, users, userlists  # noqa: E402
from qrlsh.userlists import UserLists  # noqa: E402

DEV = "cuda"


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def dense(ul):
    torch.cuda.synchronize()
    return ul.idx.cpu().numpy(), ul.milli.cpu().numpy(), ul.len.cpu().numpy()


def assert_lists(got, want, what):
    for name, g, w in zip(("idx", "milli", "len"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            raise AssertionError("%s: %s differs in rows %s" % (what, name, np.unique(np.argwhere(g != w)[:, 0])[:8].tolist()))


# ------------------------------------------------------------------------------------------------------ 1. pair kernel
PAIR_NU = 23


def _pair_matrix(nq):
    """rows 0 .. 22: row 0 all zero, row 1 a single rating (centred: all zero), row 2 = [1, 2, 2, ...] whose mean is
    fractional with a negative centred value (truncation toward zero is not floor), the rest random at mixed fill"""
    rng = np.random.default_rng(nq)
    r = (rng.integers(1, 101, size=(PAIR_NU, nq)) * (rng.random((PAIR_NU, nq)) < rng.random((PAIR_NU, 1)))).astype(np.int64)
    r[0] = 0
    r[1] = 0
    r[1, nq // 2] = 40
    r[2] = 0
    r[2, :min(nq, 3)] = [1, 2, 2][:min(nq, 3)]
    return r


def _pairs(n, rng):
    """runs of one pair and runs of many pairs sharing a first row, a and b in either order, the special rows in"""
    a_of, out = [], []
    while len(a_of) < n:
        run = 1 if rng.random() < 0.5 else int(rng.integers(2, 40))
        a_of += [int(rng.integers(0, PAIR_NU))] * run
    for k, a in enumerate(a_of[:n]):
        b = int(rng.integers(0, PAIR_NU))
        if k < 6:
            a, b = ((0, 5), (5, 1), (1, 0), (2, 7), (7, 7), (22, 2))[k] if n > 1 else (9, 4)
        out.append((a, b))
    return out


@pytest.fixture(scope="module")
def pair_refs():
    """per nq: the matrix on the device, its stats, and the old route's rows and norms -- computed once"""
    cache = {}

    def get(nq):
        if nq not in cache:
            r = _pair_matrix(nq)
            rd = dev(r)
            rows = users.center_rows(rd)
            cache[nq] = (r, rd, rows, ops.row_norms(rows), userlists.rows_stats(rd))
        return cache[nq]
    return get


@pytest.mark.parametrize("n", [1, 17, 1000])
@pytest.mark.parametrize("nq", [1, 3, 255, 256, 257, 4099, 70001])
def test_pair_kernel_bit_for_bit(pair_refs, nq, n):
    r, rd, rows, norms, (mean, norm2) = pair_refs(nq)
    pairs = _pairs(n, np.random.default_rng(1000 * nq + n))
    pd = dev(np.array([(a << 32) | b for a, b in pairs], dtype=np.int64), np.int64)
    want = ops.score_pairs(rows, norms, pd)[0]
    got = userlists.pairs_score(rd, mean, norm2, pd)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and torch.equal(got, want), (nq, n, torch.nonzero(got != want)[:5].tolist())
    assert torch.equal(norm2, norms)
    if nq <= 4099 and n <= 17:
        g = got.cpu().numpy()
        assert np.array_equal(g, UC.pair_milli(r, pairs)), (nq, n)
        if n == 17:
            assert g[0] == 0 and g[1] == 0 and g[2] == 0      # the all-zero row and the single-rating row score 0
            assert g[4] == (1000 if int(norms[7]) else 0)                # a row against itself


def test_row_stats_truncate_toward_zero():
    r = np.zeros((3, 5), dtype=np.int64)
    r[0, :3] = [1, 2, 2]            # mean 5/3: centred (-0.67, 0.33, 0.33) -> (0, 0, 0), floor would give (-1, 0, 0)
    r[1, :4] = [1, 1, 1, 5]         # mean 2: centred (-1, -1, -1, 3)
    mean, norm2 = userlists.rows_stats(dev(r))
    assert mean.cpu().tolist() == [5.0 / 3.0, 2.0, 0.0] and norm2.cpu().tolist() == [0, 12, 0]
    # chosen rows only: the others keep what they held
    mean[:] = -1.0
    norm2[:] = -1
    userlists.rows_stats(dev(r), dev([1]), mean, norm2)
    assert mean.cpu().tolist() == [-1.0, 2.0, -1.0] and norm2.cpu().tolist() == [-1, 12, -1]


# ------------------------------------------------------------------------------------------------------------ 2. rate
CASES = sorted(UC.build_cases()) + ["big_cluster"]


@pytest.fixture(scope="module")
def cases():
    c = UC.build_cases()
    c["big_cluster"] = UC.big_cluster_case()
    return c


@pytest.mark.parametrize("name", CASES)
def test_rate_equals_full_recompute_and_restatement(cases, name):
    c = cases[name]
    K, nu = c["K"], c["ratings"].shape[0]
    ul = UserLists.build(c["ratings"], c["labels"], K=K, device=DEV)
    before = UC.reference_lists(c["ratings"], c["labels"], K)
    assert_lists(dense(ul), before, (name, "build"))
    n = ul.rate(*c["edits"])
    got = dense(ul)
    assert_lists(got, UC.reference_lists(c["new"], c["labels"], K), (name, "numpy lists of the edited matrix"))
    src, dst, val = users.user_similarities(c["new"], c["labels"], K, DEV)
    assert_lists(got, UC.from_coo(src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy(), nu, K), (name, "full recompute"))
    want, picked = UC.restated_update(before, c["new"], c["labels"], K, c["R"])
    assert_lists(got, want, (name, "restatement"))
    assert ul.last_picked == len(picked) and n == len(c["R"]) + len(picked), (name, ul.last_picked, len(picked), n)
    if name in ("full_row_loses_an_entry", "ties_at_the_cut", "mixed_K19"):
        assert ul.last_picked > 0
    # the matrix and the row statistics follow
    assert np.array_equal(ul.ratings.cpu().numpy(), c["new"])
    mean, norm2 = userlists.rows_stats(ul.ratings)
    assert torch.equal(mean, ul.mean) and torch.equal(norm2, ul.norm2)
    # the COO form is what a full recompute returns
    for g, w in zip(ul.coo(), (src, dst, val)):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    u_idx, u_val, ku = ul.as_user_sims()
    assert ku == K and u_val.dtype == torch.float64 and torch.equal(u_idx, ul.idx)
    assert np.array_equal(u_val.cpu().numpy(), got[1].astype(np.float64) / 1000.0)


def test_three_batches_equal_one_build(cases):
    c = cases["mixed_K19"]
    u, q, v = c["edits"]
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    cuts = [0, len(u) // 3, 2 * len(u) // 3, len(u)]
    for a, b in zip(cuts, cuts[1:]):
        ul.rate(u[a:b], q[a:b], v[a:b])
    fresh = UserLists.build(c["new"], c["labels"], K=c["K"], device=DEV)
    assert_lists(dense(ul), dense(fresh), "three batches")
    assert torch.equal(ul.ratings, fresh.ratings) and torch.equal(ul.mean, fresh.mean) and torch.equal(ul.norm2, fresh.norm2)


def test_empty_batch_changes_nothing(cases):
    c = cases["two_clusters_at_once"]
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    names = ("ratings", "idx", "milli", "len", "mean", "norm2", "label", "c_off", "c_mem", "c_pos")
    held = {k: getattr(ul, k).clone() for k in names}
    ptrs = {k: getattr(ul, k).data_ptr() for k in names}
    assert ul.rate([], [], []) == 0 and ul.last_picked is None
    torch.cuda.synchronize()
    for k in names:
        t = getattr(ul, k)
        assert t.data_ptr() == ptrs[k] and torch.equal(t.view(torch.uint8), held[k].view(torch.uint8)), k


def test_device_matrix_is_edited_where_it_is(cases):
    c = cases["R_is_a_whole_cluster"]
    rd = dev(c["ratings"])
    ul = UserLists.build(rd, c["labels"], K=c["K"], device=DEV)
    assert ul.ratings.data_ptr() == rd.data_ptr()
    ul.rate(*c["edits"])
    assert np.array_equal(rd.cpu().numpy(), c["new"])


def test_host_layer_errors_and_repeated_cells(cases):
    c = cases["two_clusters_at_once"]
    nu, nq = c["ratings"].shape
    with pytest.raises(ValueError):
        UserLists.build(c["ratings"], c["labels"], K=65, device=DEV)
    with pytest.raises(ValueError):
        UserLists.build(c["ratings"], c["labels"], K=0, device=DEV)
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    before, held = dense(ul), ul.ratings.clone()
    for bad in (([nu], [0], [5]), ([-1], [0], [5]), ([0], [nq], [5]), ([0], [-1], [5]), ([0, 1], [0, 0], [5, -1])):
        with pytest.raises(ValueError):
            ul.rate(*bad)
    assert_lists(dense(ul), before, "after refused batches")
    assert torch.equal(ul.ratings, held)
    # a repeated cell is no error: the last value wins
    ul.rate([1, 4, 1, 1], [2, 0, 2, 2], [9, 50, 0, 77])
    new = c["ratings"].copy()
    new[1, 2], new[4, 0] = 77, 50
    assert np.array_equal(ul.ratings.cpu().numpy(), new)
    assert_lists(dense(ul), UC.reference_lists(new, c["labels"], c["K"]), "repeated cell")


def test_c_abi_refuses_bad_list_lengths():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first
    for K in (0, 65, -1):
        rc = lib.qrlsh_user_lists_mark(one, one, 4, K, one, one, one, 1, one, one, None)
        assert rc == _lib.QRLSH_EINVAL and b"K=" in lib.qrlsh_last_error(), K
        rc = lib.qrlsh_user_lists_apply(one, one, one, 4, K, one, one, 1, one, one, one, one, 1, one, one, 0, None)
        assert rc == _lib.QRLSH_EINVAL and b"K=" in lib.qrlsh_last_error(), K
    assert lib.qrlsh_user_pairs_score(one, 1 << 31, 4, one, one, one, 1, one, one, 1 << 20, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_ratings_set(one, 4, 1 << 31, one, one, one, 1, one, None) == _lib.QRLSH_EINVAL
    # empty batches return at once, whatever the pointers
    assert lib.qrlsh_ratings_set(None, 4, 4, None, None, None, 0, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_user_rows_stats(None, 4, 4, one, 0, None, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_user_pairs_score(None, 4, 4, None, None, None, 0, None, None, 0, None) == _lib.QRLSH_OK
    assert lib.qrlsh_user_cluster_pairs_count(None, 0, None, None, 4, 1, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_user_cluster_pairs_fill(None, 0, None, None, None, None, 4, 1, None, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_user_lists_apply(None, None, None, 4, 3, None, None, 0, None, None, None, None, 1, None, None, 0,
                                      None) == _lib.QRLSH_OK


# ----------------------------------------------------------------------------------------------------- 3. Recommender
def test_recommender_rate_then_recommend_users():
    from test_gpu_recommend import _recommender_on
    from test_gpu_recommend_users import _same_answers
    rec, g = _recommender_on("cfg2")
    nu, nq = rec.ratings.shape
    with pytest.raises(ValueError, match="no user index"):
        rec.rate([0], [0], [5])
    rec.compute_querySimilarities()
    labels = users.cluster_labels(rec.ratings)
    K = users.max_candidates(nu)
    assert rec.live_user_similarities(labels=labels) is rec.user_index and rec.user_index.K == K
    rng = np.random.default_rng(7)
    us, qs, vs = rng.integers(0, nu, size=40), rng.integers(0, nq, size=40), rng.integers(0, 101, size=40)
    want_r = rec.ratings.copy()
    want_r[us, qs] = vs
    assert rec.rate(us, qs, vs) >= len(np.unique(us))
    assert np.array_equal(rec.ratings, want_r) and np.array_equal(rec.user_index.ratings.cpu().numpy(), want_r)
    fresh = UserLists.build(want_r, labels, K=K, device=DEV)
    assert_lists(dense(rec.user_index), dense(fresh), "Recommender.rate")
    lists = rec._live_lists()
    chosen = [0, nu - 1, 7, 7, int(us[0])]
    idx, val, avail = qrlsh.for_users(want_r, lists[0], lists[1], lists[2], fresh.as_user_sims(), np.asarray(chosen), 7,
                                      sum_order=rec.sum_order, device=DEV)
    idx, val, avail = (t.cpu().numpy() for t in (idx, val, avail))
    want = {u: {"indexes": idx[i, :min(7, avail[i])].astype(np.int64), "values": val[i, :min(7, avail[i])].astype(np.int64),
                "available": int(avail[i])} for i, u in enumerate(chosen)}
    _same_answers(rec.recommend_users(chosen, 7), want)
    assert sum(e["available"] for e in want.values()) > 0
    rows = rec.predict_users(chosen)
    full = qrlsh.predict_users(want_r, lists[0], lists[1], lists[2], fresh.as_user_sims(), np.asarray(chosen),
                               sum_order=rec.sum_order, device=DEV)
    assert np.array_equal(rows.to_numpy(), full.cpu().numpy())
