"""The live user lists follow appended, removed and re-rated queries (csrc/usercolumns.hip, qrlsh.UserLists.add_columns
/ remove_columns / set_columns, Recommender.add_queries / remove_queries / replace_queries): every check is exact.  The
two kernels are held to numpy through the C ABI; the operations element for element to the numpy lists of the new
matrix, to a full recompute on the device and to the restated update rule with R by the changed-values rule
(tests/user_columns_cases.py) -- never to themselves."""
import numpy as np
import pytest
import torch

import user_columns_cases as CC
import user_lists_cases as UC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib, ops, users, userlists  # noqa: E402
from qrlsh.ops import _ptr  # noqa: E402
from qrlsh.userlists import UserLists  # noqa: E402

DEV = "cuda"
SENTINEL = -7
PAD = 64    # int32 words before and behind the output: the base stays 16-byte aligned


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


# ---------------------------------------------------------------------------------------------- 1. and 2. the kernels
def _matrix(nu, nq):
    rng = np.random.default_rng(1000 * nu + nq)
    return (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < 0.4)).astype(np.int64)


def _ops(r):
    """(name, op, cols, block) at the sizes where head, tail, vector count and tile edge change between nq and nq2"""
    nu, nq = r.shape
    rng = np.random.default_rng(nq)
    out = []
    for m in (1, 2, 3, 5):
        out.append(("append %d" % m, "add", None, (rng.integers(1, 101, size=(nu, m)) * (rng.random((nu, m)) < 0.5))))
    every_other = list(range(0, nq, 2))
    scattered = sorted({nq // 5, nq // 2, (4 * nq) // 5})
    for name, cols in (("first", [0]), ("last", [nq - 1]), ("every other", every_other), ("scattered", scattered),
                       ("all but one", [q for q in range(nq) if q != nq // 3]), ("all", list(range(nq)))):
        out.append(("remove " + name, "remove", cols, None))
    at = sorted({0, nq - 1, nq // 2})
    b = r[:, at].copy()
    b[::2] = rng.integers(0, 101, size=b[::2].shape)
    out.append(("overwrite", "set", at, b))
    return out


def _src(nq, op, cols, block):
    """(src, cols of the changed kernel, m) as UserLists builds them"""
    if op == "add":
        m = block.shape[1]
        return np.concatenate((np.arange(nq), -1 - np.arange(m))), np.full(m, -1), m
    if op == "remove":
        c = np.unique(np.asarray(cols, dtype=np.int64))
        keep = np.ones(nq, dtype=bool)
        keep[c] = False
        return np.flatnonzero(keep), c, c.size
    src = np.arange(nq)
    src[cols] = -1 - np.arange(len(cols))
    return src, np.asarray(cols), len(cols)


def _move(rd, nq, src, block, m):
    """qrlsh_ratings_columns_move into the middle of a sentinel-filled buffer -> (rc, the whole buffer, flag)"""
    lib = _lib.load()
    nu, nq2 = rd.shape[0], len(src)
    buf = torch.full((PAD + nu * nq2 + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    flag = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    sd = dev(src) if nq2 else None
    bd = None if block is None else dev(block)
    rc = lib.qrlsh_ratings_columns_move(_ptr(rd), nu, nq, _ptr(sd), nq2, _ptr(bd), m, ops._vp(buf.data_ptr() + 4 * PAD),
                                        _ptr(flag), ops._stream())
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), int(flag.item())


def _changed(rd, nq, cols, block, m):
    """qrlsh_ratings_columns_changed -> (the rows of the map by qrlsh_idmap_list, out2)"""
    lib = _lib.load()
    nu = rd.shape[0]
    rmap = ops._ws(lib.qrlsh_idmap_workspace_bytes(nu), DEV)
    out2 = torch.full((2,), 99, dtype=torch.int64, device=DEV)
    bd = None if block is None else dev(block)
    _lib.check(lib.qrlsh_ratings_columns_changed(_ptr(rd), nu, nq, _ptr(dev(cols)), _ptr(bd), m, _ptr(rmap), _ptr(out2),
                                                 ops._stream()))
    ids = torch.full((nu,), -1, dtype=torch.int32, device=DEV)
    _lib.check(lib.qrlsh_idmap_list(_ptr(rmap), nu, _ptr(ids), ops._stream()))
    torch.cuda.synchronize()
    ids = ids.cpu().numpy()
    return ids[ids >= 0], out2.cpu().tolist()


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 255, 256, 257, 4099])
@pytest.mark.parametrize("nu", [1, 7, 70])
def test_both_kernels_against_numpy(nu, nq):
    r = _matrix(nu, nq)
    rd = dev(r)
    for name, op, cols, block in _ops(r):
        new, R = CC.apply_op(r, op, cols, block)
        src, ccols, m = _src(nq, op, cols, block)
        rc, buf, flag = _move(rd, nq, src, block, m)
        assert rc == _lib.QRLSH_OK, (name, rc)
        if m == 0:           # nothing to do: returned at once, nothing written
            assert (buf == SENTINEL).all() and flag == 99, name
            continue
        assert flag == 0, name
        assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + new.size:] == SENTINEL).all(), name
        assert np.array_equal(buf[PAD:PAD + new.size].reshape(new.shape), new), name
        got, out2 = _changed(rd, nq, ccols, block, m)
        assert got.tolist() == R.tolist() and out2 == [len(R), 0], (name, out2)
    assert np.array_equal(rd.cpu().numpy(), r)
    # a removal may name a column twice
    if nq >= 3:
        got, out2 = _changed(rd, nq, np.array([nq - 1, 0, nq - 1, nq - 1]), None, 4)
        assert got.tolist() == np.flatnonzero(r[:, [0, nq - 1]].any(axis=1)).tolist() and out2[1] == 0


def test_changed_kernel_on_a_map_of_five_words():
    r, _ = CC.mixed_matrix()
    rd = dev(r)
    cases, top = CC.build_cases(), []
    for name in ("mixed_K19_add", "mixed_K19_remove", "mixed_K19_set"):
        c = cases[name]
        block = None if c["op"] == "remove" else c["block"]
        _, ccols, m = _src(r.shape[1], c["op"], c["cols"], block)
        got, out2 = _changed(rd, r.shape[1], ccols, block, m)
        assert got.tolist() == c["R"].tolist() and out2 == [len(c["R"]), 0], name
        top.append(int(got.max()))
    assert max(top) >= 128       # the map's fifth word
    # nobody differs: an empty map
    got, out2 = _changed(rd, r.shape[1], np.array([3, 9]), r[:, [3, 9]], 2)
    assert got.size == 0 and out2 == [0, 0]


def test_a_column_outside_range_sets_the_flag():
    nu, nq = 7, 257
    r = _matrix(nu, nq)
    rd = dev(r)
    for bad in (nq, nq + 1000, -2):
        got, out2 = _changed(rd, nq, np.array([5, bad, 9]), None, 3)
        assert out2[1] == 1, bad
        assert got.tolist() == np.flatnonzero(r[:, [5, 9]].any(axis=1)).tolist()      # the others are still looked at
    # the move: refused src values in the scalar head, inside a vector and at the tail leave their columns' sentinels
    m = 2
    block = np.arange(1, nu * m + 1).reshape(nu, m)
    src = np.concatenate((np.arange(nq), -1 - np.arange(m)))
    want = np.hstack((r, block))
    for pos, val in ((0, nq), (1, -1 - m), (130, 1 << 30), (len(src) - 1, -(1 << 30)), (7, nq)):
        s = src.copy()
        s[pos] = val
        rc, buf, flag = _move(rd, nq, s, block, m)
        assert rc == _lib.QRLSH_OK and flag == 1, (pos, val)
        got = buf[PAD:PAD + want.size].reshape(want.shape)
        w = want.copy()
        w[:, pos] = SENTINEL
        assert np.array_equal(got, w), (pos, val)
        assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + want.size:] == SENTINEL).all()
    # without a block the values of ~k are zero
    rc, buf, flag = _move(rd, nq, src, None, m)
    assert rc == _lib.QRLSH_OK and flag == 0
    assert np.array_equal(buf[PAD:PAD + want.size].reshape(want.shape), np.hstack((r, np.zeros((nu, m), dtype=np.int64))))


# --------------------------------------------------------------------------------------------------- 3. every case
CASES = sorted(CC.build_cases())
FIELDS = ("idx", "milli", "len", "mean", "norm2")


@pytest.fixture(scope="module")
def cases():
    return CC.build_cases()


@pytest.mark.parametrize("name", CASES)
def test_operation_equals_full_recompute_and_restatement(cases, name):
    c = cases[name]
    K, nu = c["K"], c["ratings"].shape[0]
    given = dev(c["ratings"])
    ul = UserLists.build(given, c["labels"], K=K, device=DEV)
    before = UC.reference_lists(c["ratings"], c["labels"], K)
    assert_lists(dense(ul), before, (name, "build"))
    held = {k: (getattr(ul, k).data_ptr(), getattr(ul, k).clone()) for k in FIELDS}
    n = CC.run(ul, c)
    got = dense(ul)
    assert_lists(got, UC.reference_lists(c["new"], c["labels"], K), (name, "numpy lists of the new matrix"))
    src, dst, val = users.user_similarities(c["new"], c["labels"], K, DEV)
    assert_lists(got, UC.from_coo(src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy(), nu, K), (name, "full recompute"))
    want, picked = UC.restated_update(before, c["new"], c["labels"], K, c["R"])
    assert_lists(got, want, (name, "restatement"))
    assert ul.last_picked == len(picked) and n == len(c["R"]) + len(picked), (name, ul.last_picked, len(picked), n)
    if name in CC.PICKS:
        assert ul.last_picked > 0
    # the matrix, its shape and the row statistics follow
    assert (ul.nu, ul.nq) == c["new"].shape == tuple(ul.ratings.shape) and ul.ratings.dtype == torch.int32
    assert ul.ratings.is_contiguous() and ul.ratings.data_ptr() % 16 == 0
    assert np.array_equal(ul.ratings.cpu().numpy(), c["new"])
    mean, norm2 = userlists.rows_stats(ul.ratings)
    assert torch.equal(mean, ul.mean) and torch.equal(norm2, ul.norm2)
    for g, w in zip(ul.coo(), (src, dst, val)):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    if name in CC.R_EMPTY:       # only the matrix moved
        assert n == 0
        for k in FIELDS:
            t = getattr(ul, k)
            assert t.data_ptr() == held[k][0] and torch.equal(t.view(torch.uint8), held[k][1].view(torch.uint8)), (name, k)
    # the tensor given to build is as it was
    assert np.array_equal(given.cpu().numpy(), c["ratings"])


def test_device_block_and_int_block_are_taken(cases):
    c = cases["block_appended_two_users_rated"]
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    assert ul.add_columns(dev(c["block"])) == len(c["R"]) + ul.last_picked
    assert_lists(dense(ul), UC.reference_lists(c["new"], c["labels"], c["K"]), "device block")
    assert np.array_equal(ul.ratings.cpu().numpy(), c["new"])
    assert ul.add_columns(0) == 0 and ul.nq == c["new"].shape[1]
    assert ul.set_columns([1, 0], dev(c["new"][:, [1, 0]])) == 0


# ------------------------------------------------------------------------------------------------------ 4. sequence
def test_sequence_of_operations_equals_one_build(cases):
    r, lab = CC.mixed_matrix()
    nu, K = r.shape[0], 19
    rng = np.random.default_rng(44)
    ul = UserLists.build(r, lab, K=K, device=DEV)
    cur = r.copy()
    add = (rng.integers(1, 101, size=(nu, 5)) * (rng.random((nu, 5)) < 0.05)).astype(np.int64)
    ul.add_columns(add)
    cur = np.hstack((cur, add))
    u, q, v = rng.integers(0, nu, size=9), rng.integers(0, cur.shape[1], size=9), rng.integers(0, 101, size=9)
    ul.rate(u, q, v)
    cur[u, q] = v
    gone = [40, 3, 3, 17]
    ul.remove_columns(gone)
    cur = np.delete(cur, gone, axis=1)
    cols = [cur.shape[1] - 1, 2]
    b = cur[:, cols].copy()
    b[rng.integers(0, nu, size=6), rng.integers(0, 2, size=6)] = rng.integers(0, 101, size=6)
    ul.set_columns(cols, b)
    cur[:, cols] = b
    u, q, v = rng.integers(0, nu, size=9), rng.integers(0, cur.shape[1], size=9), rng.integers(0, 101, size=9)
    ul.rate(u, q, v)
    cur[u, q] = v
    fresh = UserLists.build(cur, lab, K=K, device=DEV)
    assert_lists(dense(ul), dense(fresh), "the sequence")
    assert_lists(dense(ul), UC.reference_lists(cur, lab, K), "the sequence against numpy")
    assert (ul.nu, ul.nq) == cur.shape
    assert torch.equal(ul.ratings, fresh.ratings) and torch.equal(ul.mean, fresh.mean) and torch.equal(ul.norm2, fresh.norm2)


# -------------------------------------------------------------------------------------------- 5. refused arguments
def test_refused_arguments_leave_every_field(cases):
    c = cases["two_clusters_at_once"]
    nu, nq = c["ratings"].shape
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    names = ("ratings",) + FIELDS + ("label", "c_off", "c_mem", "c_pos")
    held = {k: (getattr(ul, k).data_ptr(), getattr(ul, k).clone()) for k in names}
    ok = np.zeros((nu, 2), dtype=np.int64)
    neg, big = ok.copy(), ok.copy()
    neg[3, 1], big[0, 0] = -1, 2**31
    refused = [
        lambda: ul.add_columns(np.zeros((nu + 1, 2), dtype=np.int64)),
        lambda: ul.add_columns(np.zeros(nu, dtype=np.int64)),
        lambda: ul.add_columns(np.zeros((nu, 2))),                       # floats
        lambda: ul.add_columns(neg),
        lambda: ul.add_columns(big),
        lambda: ul.add_columns(-1),
        lambda: ul.add_columns(torch.zeros((nu, 2), dtype=torch.int64, device=DEV)),
        lambda: ul.remove_columns([0, nq]),
        lambda: ul.remove_columns([-1]),
        lambda: ul.remove_columns([0.5]),
        lambda: ul.set_columns([0, nq], ok),
        lambda: ul.set_columns([-1, 2], ok),
        lambda: ul.set_columns([4, 4], ok),
        lambda: ul.set_columns([4, 5, 6], ok),
        lambda: ul.set_columns([4, 5], neg),
        lambda: ul.set_columns([4, 5], big),
        lambda: ul.set_columns([4, 5], np.zeros((nu - 1, 2), dtype=np.int64)),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert (ul.nu, ul.nq) == (nu, nq), i
        for k in names:
            t = getattr(ul, k)
            assert t.data_ptr() == held[k][0] and torch.equal(t.view(torch.uint8), held[k][1].view(torch.uint8)), (i, k)


# ---------------------------------------------------------------------------------------------------- 6. Recommender
def test_recommender_user_index_follows_the_queries():
    from test_gpu_recommend import _recommender_on
    from test_gpu_recommend_users import _same_answers
    from qrlsh import pipeline
    rec, g = _recommender_on("cfg2")
    N, nu = rec.queriesIDs.size, rec.usersIDs.size
    n0 = N - 9
    block = rec.ratings[:, n0:].copy()
    rest, ids = np.asarray(rec.queries, dtype=object)[n0:], rec.queriesIDs[n0:]
    rec.queries, rec.queriesIDs, rec.ratings = rec.queries[:n0], rec.queriesIDs[:n0], rec.ratings[:, :n0]
    rec.max_candidates = pipeline.max_candidates(N)
    np.random.seed(int(g["seed"]))
    rec.compute_querySimilarities()
    labels = users.cluster_labels(rec.ratings)
    K = users.max_candidates(nu)
    rec.live_user_similarities(labels=labels)

    def raises():
        raise AssertionError("compute_userSimilarities ran: the user index did not serve")
    rec.compute_userSimilarities = raises
    chosen = [0, nu - 1, 7, 7, 3]
    rng = np.random.default_rng(11)

    def check(what):
        ui = rec.user_index
        assert (ui.nu, ui.nq) == rec.ratings.shape, what
        assert np.array_equal(ui.ratings.cpu().numpy(), rec.ratings), what
        fresh = UserLists.build(rec.ratings, labels, K=K, device=DEV)
        assert_lists(dense(ui), dense(fresh), what)
        assert torch.equal(ui.mean, fresh.mean) and torch.equal(ui.norm2, fresh.norm2), what
        lists = rec._live_lists()
        idx, val, avail = qrlsh.for_users(rec.ratings, lists[0], lists[1], lists[2], fresh.as_user_sims(), np.asarray(chosen),
                                          7, sum_order=rec.sum_order, device=DEV)
        idx, val, avail = (t.cpu().numpy() for t in (idx, val, avail))
        want = {u: {"indexes": idx[i, :min(7, avail[i])].astype(np.int64), "values": val[i, :min(7, avail[i])].astype(np.int64),
                    "available": int(avail[i])} for i, u in enumerate(chosen)}
        _same_answers(rec.recommend_users(chosen, 7), want)
        assert sum(e["available"] for e in want.values()) > 0, what
        full = qrlsh.predict_users(rec.ratings, lists[0], lists[1], lists[2], fresh.as_user_sims(), np.asarray(chosen),
                                   sum_order=rec.sum_order, device=DEV)
        assert np.array_equal(rec.predict_users(chosen).to_numpy(), full.cpu().numpy()), what

    def rate_then_check(what):
        check(what)
        us, qs, vs = rng.integers(0, nu, size=12), rng.integers(0, rec.ratings.shape[1], size=12), rng.integers(0, 101, size=12)
        assert rec.rate(us, qs, vs) >= len(np.unique(us)), what
        check(what + ", then rate")

    rate_then_check("after the build")
    rec.add_queries(rest, ratings=block, ids=ids, update_lists=True)
    assert rec.ratings.shape == (nu, N) and block.any()
    rate_then_check("after add_queries")
    rec.remove_queries([0, N // 2, N - 1, 0], update_lists=True)
    assert rec.ratings.shape == (nu, N - 3)
    rate_then_check("after remove_queries")
    pos = [5, N - 5, 1]
    texts = np.asarray(rec.queries, dtype=object)[[8, 9, 10]]
    newb = rng.integers(0, 101, size=(nu, 3)) * (rng.random((nu, 3)) < 0.3)
    rec.replace_queries(pos, texts, ratings=newb, update_lists=True)
    assert np.array_equal(rec.ratings[:, pos], newb)
    rate_then_check("after replace_queries with ratings")
    ptr = rec.user_index.ratings.data_ptr()
    rec.replace_queries([2, 6], np.asarray(rec.queries, dtype=object)[[11, 12]], update_lists=True)
    assert rec.user_index.ratings.data_ptr() == ptr
    rate_then_check("after replace_queries without ratings")
    # an unrated batch appends unrated columns
    rec.add_queries(np.asarray(rec.queries, dtype=object)[[0, 1]], update_lists=True)
    assert rec.ratings.shape == (nu, N - 1) and not rec.ratings[:, -2:].any()
    check("after add_queries without ratings")
    # an index that is out of step is left alone, and rate says so
    rec.user_index.remove_columns([0])
    held = rec.user_index.ratings
    rec.add_queries(np.asarray(rec.queries, dtype=object)[[3]], update_lists=True)
    assert rec.user_index.ratings is held and rec.user_index.nq == N - 2
    with pytest.raises(ValueError, match="queries were added or removed"):
        rec.rate([0], [0], [5])
