"""Users join and leave the live user lists (csrc/userrows.hip, qrlsh.UserLists.add_users / remove_users / nearest,
Recommender.add_users / remove_users): every check is exact.  The three kernels are held to numpy through the C ABI,
their outputs inside sentinel-filled buffers; the operations element for element to the numpy lists of the new matrix,
to a full recompute on the device and to the restated rules (tests/user_rows_cases.py) -- never to themselves."""
import numpy as np
import pytest
import torch

import user_lists_cases as UC
import user_rows_cases as RC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib, ops, users, userlists  # noqa: E402
from qrlsh.ops import _ptr  # noqa: E402
from qrlsh.userlists import UserLists  # noqa: E402

DEV = "cuda"
SENTINEL = -7
PAD = 64    # int32 words before and behind an output: the base stays 16-byte aligned


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


def padded(n, fill=SENTINEL):
    """an int32 buffer of n words between two pads -> (the whole buffer, a pointer to its middle)"""
    buf = torch.full((PAD + n + PAD,), fill, dtype=torch.int32, device=DEV)
    return buf, ops._vp(buf.data_ptr() + 4 * PAD)


def middle(buf, n):
    b = buf.cpu().numpy()
    assert (b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all(), "written before or behind the output"
    return b[PAD:PAD + n]


# -------------------------------------------------------------------------------------------------- 1. the kernels
def _matrix(nu, nq, scale=1):
    """ratings with an unrated row and a row of one rating (zero norms) where there is room"""
    rng = np.random.default_rng(1000 * nu + nq)
    r = (rng.integers(1, 101, size=(nu, nq)) * scale * (rng.random((nu, nq)) < 0.6)).astype(np.int64)
    if nu >= 7:
        r[3] = 0
        r[5] = 0
        r[5, nq // 2] = 40 * scale
    return r


def _new_rows(r, m):
    nu, nq = r.shape
    rng = np.random.default_rng(7 * nu + nq + m)
    rows = (rng.integers(1, 101, size=(m, nq)) * (rng.random((m, nq)) < 0.6)).astype(np.int64)
    rows[0] = r[nu // 2]                              # a copy of an existing user
    if m >= 7:
        rows[2] = 0                                   # zero norms on this side too
        rows[4] = 0
        rows[4, 0] = 9
        rows[6] = r[0]
    return rows


def _nearest(rd, mean, norm2, rows, want_all):
    """qrlsh_user_rows_nearest with every output in a sentinel-filled buffer -> (user, milli, every score or None)"""
    lib = _lib.load()
    nu, nq = rd.shape
    m = rows.shape[0]
    rows_d = dev(rows)
    rmean, rnorm2 = userlists.rows_stats(rows_d)
    ub, up = padded(m)
    mb, mp = padded(m)
    ab, ap = padded(m * nu)
    ws = ops._ws(lib.qrlsh_user_rows_nearest_workspace_bytes(nu, m), DEV)
    ws.fill_(0x5A)                                    # the call clears its own workspace
    _lib.check(lib.qrlsh_user_rows_nearest(_ptr(rd), nu, nq, _ptr(mean), _ptr(norm2), _ptr(rows_d), m, _ptr(rmean),
                                           _ptr(rnorm2), up, mp, ap if want_all else None, _ptr(ws), ws.numel(),
                                           ops._stream()))
    torch.cuda.synchronize()
    every = middle(ab, m * nu)
    if not want_all:
        assert (every == SENTINEL).all()
    return middle(ub, m), middle(mb, m), every.reshape(m, nu) if want_all else None


NQS = [1, 3, 4, 5, 255, 256, 257, 4099]        # 4099: five slices of 1024 columns, the last of three
NUS = [1, 7, 70, 600]                          # 600: more than the 4 x 128 existing rows of one workgroup


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("nu", NUS)
def test_nearest_kernel_against_numpy(nu, nq):
    r = _matrix(nu, nq)
    rd = dev(r)
    mean, norm2 = userlists.rows_stats(rd)
    for m in (1, 7, 8, 9):                     # one row; below, at and above the tile of 8 new rows
        rows = _new_rows(r, m)
        wu, wm, wall = RC.nearest_rule(r, rows)
        user, milli, every = _nearest(rd, mean, norm2, rows, True)
        assert np.array_equal(every, wall), (m, np.argwhere(every != wall)[:5].tolist())
        assert np.array_equal(user, wu) and np.array_equal(milli, wm), m
        user, milli, _ = _nearest(rd, mean, norm2, rows, False)
        assert np.array_equal(user, wu) and np.array_equal(milli, wm), (m, "without milli_out")
    assert np.array_equal(rd.cpu().numpy(), r)


def test_nearest_kernel_needs_64_bit_sums():
    nu, nq, m = 70, 4099, 9
    r = _matrix(nu, nq, scale=10007)           # values near 10^6: one product is near 10^12
    assert r.max() > 900000
    rows = _new_rows(r, m)
    rows[1] = (np.random.default_rng(3).integers(1, 101, size=nq) * 9973)
    rd = dev(r)
    mean, norm2 = userlists.rows_stats(rd)
    wu, wm, wall = RC.nearest_rule(r, rows)
    user, milli, every = _nearest(rd, mean, norm2, rows, True)
    assert np.array_equal(every, wall) and np.array_equal(user, wu) and np.array_equal(milli, wm)
    assert (wm > 0).any() and (wall < 0).any()


def test_nearest_kernel_ties_go_to_the_lowest_id():
    nu, nq = 70, 257
    r = _matrix(nu, nq)
    r[61] = r[9]
    r[33] = r[9]
    rd = dev(r)
    mean, norm2 = userlists.rows_stats(rd)
    user, milli, _ = _nearest(rd, mean, norm2, r[[61]], False)
    assert (user.tolist(), milli.tolist()) == ([9], [1000])


def _move(rd, src, block, block_offset=0):
    """qrlsh_ratings_rows_move into the middle of a sentinel-filled buffer -> (rc, the output rows, flag)"""
    lib = _lib.load()
    nu, nq = rd.shape
    nu2 = len(src)
    buf, out = padded(nu2 * nq)
    flag = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    m, bp = 0, None
    if block is not None:
        m = block.shape[0]
        hold = torch.zeros((block.size + 8,), dtype=torch.int32, device=DEV)   # block_offset words off 16 bytes
        hold[block_offset:block_offset + block.size] = dev(block).reshape(-1)
        bp = ops._vp(hold.data_ptr() + 4 * block_offset)
    sd = dev(src)
    rc = lib.qrlsh_ratings_rows_move(_ptr(rd), nu, nq, _ptr(sd), nu2, bp, m, out, _ptr(flag), ops._stream())
    torch.cuda.synchronize()
    return rc, middle(buf, nu2 * nq).reshape(nu2, nq), int(flag.item())


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("nu", [1, 7, 70])
def test_rows_move_kernel_against_numpy(nu, nq):
    r = _matrix(nu, nq)
    rd = dev(r)
    block = np.arange(1, 3 * nq + 1, dtype=np.int64).reshape(3, nq)
    both = np.vstack((r, block))
    for off in (0, 1):                         # the block on and off a 16-byte boundary
        src = np.concatenate((np.arange(nu), -1 - np.arange(3)))
        rc, out, flag = _move(rd, src, block, off)
        assert rc == _lib.QRLSH_OK and flag == 0 and np.array_equal(out, both), ("append", off)
    removals = {"first": np.arange(1, nu), "last": np.arange(nu - 1), "every other": np.arange(1, nu, 2),
                "all but one": np.array([nu // 2])}
    for name, src in removals.items():
        if src.size == 0:                      # nobody left: returned at once
            continue
        rc, out, flag = _move(rd, src, None)
        assert rc == _lib.QRLSH_OK and flag == 0 and np.array_equal(out, r[src]), name
    # any order and repeats, rows of the block between rows of the matrix
    src = np.array([-2, nu - 1, 0, -1, nu // 2, -3, 0])
    rc, out, flag = _move(rd, src, block, 1)
    assert rc == _lib.QRLSH_OK and flag == 0 and np.array_equal(out, both[np.where(src >= 0, src, nu + ~src)])
    assert np.array_equal(rd.cpu().numpy(), r)


def test_rows_move_refuses_a_row_outside_range():
    nu, nq = 7, 257
    r = _matrix(nu, nq)
    rd = dev(r)
    block = np.arange(1, 2 * nq + 1, dtype=np.int64).reshape(2, nq)
    src = np.concatenate((np.arange(nu), -1 - np.arange(2)))
    want = np.vstack((r, block))
    for pos, val in ((0, nu), (4, -3), (4, 1 << 30), (len(src) - 1, -(1 << 30)), (len(src) - 1, nu + 5)):
        s = src.copy()
        s[pos] = val
        rc, out, flag = _move(rd, s, block)
        assert rc == _lib.QRLSH_OK and flag == 1, (pos, val)
        w = want.copy()
        w[pos] = SENTINEL
        assert np.array_equal(out, w), (pos, val)
    rc, out, flag = _move(rd, np.array([2, -1, 3]), None)      # without a block nothing negative is in range
    assert flag == 1 and np.array_equal(out[[0, 2]], r[[2, 3]]) and (out[1] == SENTINEL).all()


def _renumber(lists, nu, K, src, new_pos):
    lib = _lib.load()
    nu2 = len(src)
    ib, ip = padded(nu2 * K)
    mb, mp = padded(nu2 * K)
    lb, lp = padded(nu2)
    flag = torch.full((1,), 99, dtype=torch.int32, device=DEV)
    idx, mil, ln, sd, pd = (dev(a) for a in lists + (src, new_pos))      # held until the kernel has run
    _lib.check(lib.qrlsh_user_lists_renumber(_ptr(idx), _ptr(mil), _ptr(ln), nu, K, _ptr(sd), nu2, _ptr(pd), ip, mp, lp,
                                             _ptr(flag), ops._stream()))
    torch.cuda.synchronize()
    return (middle(ib, nu2 * K).reshape(nu2, K), middle(mb, nu2 * K).reshape(nu2, K), middle(lb, nu2)), int(flag.item())


@pytest.mark.parametrize("K", [1, 19, 64])
def test_renumber_kernel_against_numpy(K):
    r, lab = RC.mixed_matrix()
    nu = r.shape[0]
    lists = UC.reference_lists(r, lab, K)
    # a removal whose rows name no removed user: a whole cluster leaves
    gone = np.flatnonzero(lab == lab[np.flatnonzero(lab != 0)[0]])
    new_pos, keep = RC.new_positions(nu, gone)
    src = np.flatnonzero(keep)
    want = UC.empty_lists(len(src), K)
    for u2, s in enumerate(src):
        L = lists[2][s]
        want[0][u2, :L], want[1][u2, :L], want[2][u2] = new_pos[lists[0][s, :L]], lists[1][s, :L], L
    got, flag = _renumber(lists, nu, K, src, new_pos)
    assert flag == 0
    assert_lists(got, want, "a cluster leaves")
    # empty rows where src is negative
    src2, holes = src.copy(), UC.empty_lists(len(src), K)
    src2[[0, 7]] = -1
    for a, w in zip(holes, want):
        a[:] = w
        a[[0, 7]] = a[0].dtype.type(-1 if a is holes[0] else 0)
    got, flag = _renumber(lists, nu, K, src2, new_pos)
    assert flag == 0
    assert_lists(got, holes, "empty rows")
    # an entry whose target is gone, a length and an index outside range, a row outside range: the flag
    named = int(lists[0][np.flatnonzero(lists[2] > 0)[0], 0])
    bad_pos = np.arange(nu)
    bad_pos[named] = -1
    assert _renumber(lists, nu, K, np.arange(nu), bad_pos)[1] == 1
    bad_pos[named] = nu
    assert _renumber(lists, nu, K, np.arange(nu), bad_pos)[1] == 1
    for k, v in ((2, K + 1), (2, -1)):
        broken = tuple(a.copy() for a in lists)
        broken[k][7] = v
        assert _renumber(broken, nu, K, np.arange(nu), np.arange(nu))[1] == 1, (k, v)
    full = int(np.flatnonzero(lists[2] > 0)[0])
    for v in (nu, -2):
        broken = tuple(a.copy() for a in lists)
        broken[0][full, 0] = v
        assert _renumber(broken, nu, K, np.arange(nu), np.arange(nu))[1] == 1, v
    assert _renumber(lists, nu, K, np.array([0, nu]), np.arange(nu))[1] == 1
    assert _renumber(lists, nu, K, np.arange(nu), np.arange(nu))[1] == 0


def test_entry_points_check_their_sizes():
    lib = _lib.load()
    z = torch.zeros((64,), dtype=torch.int64, device=DEV)
    p = _ptr(z)
    st = ops._stream()
    assert lib.qrlsh_user_rows_nearest(p, 1 << 31, 4, p, p, p, 1, p, p, p, p, None, p, 512, st) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_user_rows_nearest(p, 1 << 20, 4, p, p, p, 1 << 12, p, p, p, p, None, p, 512, st) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_user_rows_nearest(p, 4, 4, p, p, p, 4, p, p, p, p, None, p, 4 * 4 * 8 - 1, st) == _lib.QRLSH_EWORKSPACE
    assert lib.qrlsh_user_rows_nearest_workspace_bytes(4, 4) == 4 * 4 * 8
    assert lib.qrlsh_ratings_rows_move(p, 4, 1 << 31, p, 4, None, 0, p, p, st) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_ratings_rows_move(p, 4, 4, p, 1 << 31, None, 0, p, p, st) == _lib.QRLSH_EINVAL
    for K in (0, 65):
        assert lib.qrlsh_user_lists_renumber(p, p, p, 4, K, p, 4, p, p, p, p, p, st) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_user_lists_renumber(p, p, p, 1 << 31, 4, p, 4, p, p, p, p, p, st) == _lib.QRLSH_EINVAL
    torch.cuda.synchronize()
    assert not z.any()


# --------------------------------------------------------------------------------------------------- 2. every case
CASES = sorted(RC.build_cases())
FIELDS = ("idx", "milli", "len", "mean", "norm2")
STRUCTURE = ("label", "c_off", "c_mem", "c_pos")


@pytest.fixture(scope="module")
def cases():
    return RC.build_cases()


def assert_structure(ul, labels):
    """members ascending within a cluster, c_pos consistent, c_off cumulative; the partition is that of `labels`"""
    torch.cuda.synchronize()
    label, c_off, c_mem, c_pos = (getattr(ul, k).cpu().numpy() for k in STRUCTURE)
    nu = len(labels)
    assert ul.nu == nu == label.size == c_mem.size == c_pos.size and c_off.size == ul.nc + 1
    assert np.array_equal(ul.user_labels(), labels) and ul.user_labels().dtype == np.int64
    assert label.min() == 0 and label.max() == ul.nc - 1 == len(set(labels.tolist())) - 1
    assert len({(int(a), int(b)) for a, b in zip(label, labels)}) == ul.nc          # one dense number per label value
    assert c_off[0] == 0 and np.array_equal(np.diff(c_off), np.bincount(label, minlength=ul.nc)) and (np.diff(c_off) > 0).all()
    for c in range(ul.nc):
        mem = c_mem[c_off[c]:c_off[c + 1]]
        assert np.array_equal(mem, np.flatnonzero(label == c)), c
        assert np.array_equal(c_pos[mem], np.arange(mem.size)), c
    assert np.array_equal(ul._sizes, np.diff(c_off)) and np.array_equal(ul._dense_host, label)


@pytest.mark.parametrize("name", CASES)
def test_operation_equals_full_recompute_and_restatement(cases, name):
    c = cases[name]
    K = c["K"]
    nu2 = c["new"].shape[0]
    given = dev(c["ratings"])
    ul = UserLists.build(given, c["labels"], K=K, device=DEV)
    before, want, picked = RC.restated(c)
    assert_lists(dense(ul), before, (name, "build"))
    assert_structure(ul, c["labels"])
    ret = RC.run(ul, c)
    got = dense(ul)
    assert_lists(got, UC.reference_lists(c["new"], c["all_labels"], K), (name, "numpy lists of the new matrix"))
    src, dst, val = users.user_similarities(c["new"], c["all_labels"], K, DEV)
    assert_lists(got, UC.from_coo(src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy(), nu2, K), (name, "full recompute"))
    assert_lists(got, want, (name, "restatement"))
    assert ul.last_picked == len(picked), (name, ul.last_picked, picked)
    assert isinstance(ret, np.ndarray) and ret.dtype == np.int64
    assert np.array_equal(ret, c["returned"] if c["op"] == "add" else c["new_pos"]), (name, ret)
    if name in RC.PICKS:
        assert ul.last_picked > 0
    # the matrix, its shape, the row statistics and the cluster structure follow
    assert (ul.nu, ul.nq) == c["new"].shape == tuple(ul.ratings.shape) and ul.ratings.dtype == torch.int32
    assert ul.ratings.is_contiguous() and ul.ratings.data_ptr() % 16 == 0
    assert np.array_equal(ul.ratings.cpu().numpy(), c["new"])
    mean, norm2 = userlists.rows_stats(ul.ratings)
    assert torch.equal(mean, ul.mean) and torch.equal(norm2, ul.norm2)
    assert_structure(ul, c["all_labels"])
    for g, w in zip(ul.coo(), (src, dst, val)):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    # the tensor given to build is as it was
    assert np.array_equal(given.cpu().numpy(), c["ratings"])


def test_nearest_and_device_rows(cases):
    c = cases["mixed_K19_add_nearest"]
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    held = {k: (getattr(ul, k).data_ptr(), getattr(ul, k).clone()) for k in ("ratings",) + FIELDS + STRUCTURE}
    some = np.vstack((c["rows"], np.zeros((1, c["rows"].shape[1]), dtype=np.int64)))       # the last one rated nothing
    wu, wm, _ = RC.nearest_rule(c["ratings"], some)
    for rows in (some, dev(some), torch.from_numpy(some)):
        user, milli = ul.nearest(rows)
        assert user.dtype == milli.dtype == torch.int32 and user.is_cuda
        assert np.array_equal(user.cpu().numpy(), wu) and np.array_equal(milli.cpu().numpy(), wm)
    assert (wm > 0).any() and (wu < 0).any()
    user, milli = ul.nearest(np.zeros((0, ul.nq), dtype=np.int64))
    assert user.numel() == 0 and milli.numel() == 0
    for k, (p, t) in held.items():             # nobody was inserted
        assert getattr(ul, k).data_ptr() == p and torch.equal(getattr(ul, k), t), k
    # device rows are taken as they are; no rows rebind nothing
    assert np.array_equal(ul.add_users(dev(c["rows"])), c["returned"])
    assert_lists(dense(ul), UC.reference_lists(c["new"], c["all_labels"], c["K"]), "device rows")
    ptr = ul.ratings.data_ptr()
    assert ul.add_users(np.zeros((0, ul.nq), dtype=np.int64)).size == 0 and ul.ratings.data_ptr() == ptr
    assert np.array_equal(ul.remove_users([]), np.arange(ul.nu)) and ul.ratings.data_ptr() == ptr


# ------------------------------------------------------------------------------------------------------ 3. sequence
def test_sequence_of_operations_equals_one_build():
    r, lab = RC.mixed_matrix()
    K = 19
    rng = np.random.default_rng(45)
    ul = UserLists.build(r, lab, K=K, device=DEV)
    cur, labels = r.copy(), lab.copy()

    def rated(n):
        u, q, v = rng.integers(0, cur.shape[0], size=n), rng.integers(0, cur.shape[1], size=n), rng.integers(0, 101, size=n)
        ul.rate(u, q, v)
        cur[u, q] = v

    taste = cur[np.flatnonzero(labels == 0)[:2]]
    rows = np.vstack((np.where(rng.random(taste.shape) < 0.8, taste, 0), UC._random(rng, 2, cur.shape[1])))
    assert np.array_equal(ul.add_users(rows, labels=[0, 0, 3, 500]), [0, 0, 3, 500])
    cur, labels = np.vstack((cur, rows)), np.concatenate((labels, [0, 0, 3, 500]))
    rated(9)
    gone = [151, 7, 7, 60, 0]
    new_pos = ul.remove_users(gone)
    keep = new_pos >= 0
    assert np.array_equal(new_pos, RC.new_positions(cur.shape[0], gone)[0])
    cur, labels = np.ascontiguousarray(cur[keep]), labels[keep]
    add = (rng.integers(1, 101, size=(cur.shape[0], 3)) * (rng.random((cur.shape[0], 3)) < 0.1)).astype(np.int64)
    ul.add_columns(add)
    cur = np.hstack((cur, add))
    rows = np.vstack((cur[5], np.zeros((1, cur.shape[1]), dtype=np.int64), UC._random(rng, 2, cur.shape[1])))
    user, milli, _ = RC.nearest_rule(cur, rows)
    want = RC.assign_labels(labels, user, milli)
    assert want[0] == labels[user[0]] and milli[0] == 1000 and want[1] == labels.max() + 1
    assert np.array_equal(ul.add_users(rows), want)
    cur, labels = np.vstack((cur, rows)), np.concatenate((labels, want))
    cols = [38, 2, 2]
    ul.remove_columns(cols)
    cur = np.delete(cur, cols, axis=1)
    gone = np.flatnonzero(labels == 3)[:2].tolist() + [cur.shape[0] - 1]
    new_pos = ul.remove_users(gone)
    keep = new_pos >= 0
    cur, labels = np.ascontiguousarray(cur[keep]), labels[keep]
    rated(5)
    assert np.array_equal(ul.user_labels(), labels)
    fresh = UserLists.build(cur, ul.user_labels(), K=K, device=DEV)
    assert_lists(dense(ul), dense(fresh), "the sequence")
    assert_lists(dense(ul), UC.reference_lists(cur, labels, K), "the sequence against numpy")
    assert (ul.nu, ul.nq) == cur.shape
    assert torch.equal(ul.ratings, fresh.ratings) and torch.equal(ul.mean, fresh.mean) and torch.equal(ul.norm2, fresh.norm2)
    assert_structure(ul, labels)


# -------------------------------------------------------------------------------------------- 4. refused arguments
def test_refused_arguments_leave_every_field(cases):
    c = cases["two_clusters_and_a_new_label"]
    nu, nq = c["ratings"].shape
    ul = UserLists.build(c["ratings"], c["labels"], K=c["K"], device=DEV)
    names = ("ratings",) + FIELDS + STRUCTURE
    held = {k: (getattr(ul, k).data_ptr(), getattr(ul, k).clone()) for k in names}
    ok = np.zeros((2, nq), dtype=np.int64)
    neg, big = ok.copy(), ok.copy()
    neg[1, 3], big[0, 0] = -1, 2**31
    huge = np.broadcast_to(np.zeros((1, nq), dtype=np.int64), (2**31 - nu, nq))       # no memory behind it
    refused = [
        lambda: ul.add_users(np.zeros((2, nq + 1), dtype=np.int64)),
        lambda: ul.add_users(np.zeros(nq, dtype=np.int64)),
        lambda: ul.add_users(np.zeros((2, nq))),                          # floats
        lambda: ul.add_users(neg),
        lambda: ul.add_users(big),
        lambda: ul.add_users(huge),
        lambda: ul.add_users(torch.zeros((2, nq), dtype=torch.int64, device=DEV)),
        lambda: ul.add_users(ok, labels=[0]),
        lambda: ul.add_users(ok, labels=[0, 1, 2]),
        lambda: ul.add_users(ok, labels=[0.5, 1.0]),
        lambda: ul.nearest(np.zeros((2, nq - 1), dtype=np.int64)),
        lambda: ul.nearest(neg),
        lambda: ul.remove_users([0, nu]),
        lambda: ul.remove_users([-1]),
        lambda: ul.remove_users([0.5]),
        lambda: ul.remove_users(list(range(nu)) + [0]),                   # nobody would be left
    ]
    for i, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert (ul.nu, ul.nq) == (nu, nq), i
        assert np.array_equal(ul.user_labels(), c["labels"]), i
        for k in names:
            t = getattr(ul, k)
            assert t.data_ptr() == held[k][0] and torch.equal(t.view(torch.uint8), held[k][1].view(torch.uint8)), (i, k)


# ---------------------------------------------------------------------------------------------------- 5. Recommender
def test_recommender_users_join_and_leave():
    from test_gpu_recommend import _recommender_on
    from test_gpu_recommend_users import _same_answers
    rec, g = _recommender_on("cfg2")
    nu, N = rec.ratings.shape
    rec.compute_querySimilarities()
    labels = users.cluster_labels(rec.ratings)
    rec.live_user_similarities(labels=labels)
    ui = rec.user_index
    K = ui.K

    def raises():
        raise AssertionError("compute_userSimilarities ran: the user index did not serve")
    rec.compute_userSimilarities = raises

    def check(chosen, what):
        assert ui is rec.user_index and (ui.nu, ui.nq) == rec.ratings.shape == (rec.usersIDs.size, N), what
        assert np.array_equal(ui.ratings.cpu().numpy(), rec.ratings), what
        fresh = UserLists.build(rec.ratings, ui.user_labels(), K=K, device=DEV)
        assert_lists(dense(ui), dense(fresh), what)
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
        got = rec.predict_users(chosen)
        assert np.array_equal(got.to_numpy(), full.cpu().numpy()), what
        assert list(got.index) == list(rec.usersIDs[np.asarray(chosen)]), what

    check([0, nu - 1, 7], "after the build")
    # three newcomers: two share most ratings with users 2 and 5 (whose lists then change), one rated nothing
    rng = np.random.default_rng(12)
    block = np.vstack((np.where(rng.random(N) < 0.9, rec.ratings[2], 0), np.where(rng.random(N) < 0.9, rec.ratings[5], 0),
                       np.zeros(N, dtype=np.int64)))
    before = dense(ui)
    old_ids = rec.usersIDs.copy()
    pos = rec.add_users(block)
    assert pos.tolist() == [nu, nu + 1, nu + 2] and rec.ratings.shape == (nu + 3, N)
    assert rec.usersIDs.size == nu + 3 and rec.usersIDs.dtype == old_ids.dtype and np.array_equal(rec.usersIDs[:nu], old_ids)
    after = dense(ui)
    changed = [v for v in range(nu) if not np.array_equal(before[0][v], after[0][v, :])]
    assert changed and all(int(np.max(after[0][v])) >= nu for v in changed)
    assert ui.user_labels()[nu] == labels[2] or after[2][nu] > 0
    check([nu, nu + 1, nu + 2, changed[0], 0], "after add_users")
    us, qs, vs = rng.integers(0, nu + 3, size=12), rng.integers(0, N, size=12), rng.integers(0, 101, size=12)
    assert rec.rate(us, qs, vs) >= len(np.unique(us))
    check([nu + 1, changed[0], 3], "after add_users, then rate")
    ids_before = rec.usersIDs.copy()
    gone = sorted({changed[0], 1, nu})
    new_pos = rec.remove_users(gone + [1])
    keep = new_pos >= 0
    assert keep.sum() == nu + 3 - len(gone) and np.array_equal(new_pos, RC.new_positions(nu + 3, gone)[0])
    assert np.array_equal(rec.usersIDs, ids_before[keep]) and rec.ratings.shape == (keep.sum(), N)
    nu = int(keep.sum())
    check([0, nu - 1, int(new_pos[nu + 1]), 4], "after remove_users")
    # labels given; ids under usersIDs' dtype rule
    ids = np.asarray([10**6]) if rec.usersIDs.dtype.kind in "iu" else np.asarray(["newcomer"])
    pos = rec.add_users(block[:1], ids=ids, labels=[int(labels[0])])
    assert rec.usersIDs[-1] == ids.astype(rec.usersIDs.dtype)[0] and ui.user_labels()[-1] == labels[0]
    check([int(pos[0]), 0], "after add_users with labels and ids")
    with pytest.raises(ValueError):
        rec.add_users(block[:1], ids=[1, 2])
    with pytest.raises(ValueError):
        rec.add_users(np.zeros((1, N + 1), dtype=np.int64))
    with pytest.raises(ValueError):
        rec.remove_users([rec.usersIDs.size])
    check([int(pos[0]), 0], "after refused calls")
    # an index that is out of step is left alone
    ui.remove_users([0])
    held, n_now = ui.ratings, rec.usersIDs.size
    rec.add_users(block[:1])
    assert ui.ratings is held and ui.nu == n_now - 1 and rec.ratings.shape[0] == n_now + 1
    rec.remove_users([0])
    assert ui.ratings is held and rec.ratings.shape[0] == n_now
    with pytest.raises(ValueError):
        rec.rate([0], [0], [5])
