"""Keeping the top-K lists current when queries are appended (qrlsh_index_probe_finish_indexed, qrlsh_lists_update_*,
QueryIndex.append(update_lists=True) / neighbours_of, Recommender.add_queries(update_lists=True)): every check is
exact.  The device is held to the numpy restatement (tests/lists_update_cases.py), to the oracle, and to the existing
full path over all rows -- pipeline.query_similarities where the input is answer sets, the same sequence of ops from the
band keys on where the input is a signature matrix -- never to the update itself."""
import ctypes

import numpy as np
import pytest
import torch

import lists_update_cases as LC
import query_index_cases as QC

pytestmark = pytest.mark.gpu

FORMATS = [False, True]      # int32 rows, compact uint16 rows


def _rows(sig, compact=False):
    t = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.int32)).cuda()
    if compact:
        t = t.bitwise_and(0xFFFF).to(torch.int16)
    return t


def _dev(lists):
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in lists)


def _host(lists):
    return tuple(t.cpu().numpy() for t in lists)


def _index(sig, b, K, compact=False, lists=None, keys=None):
    from qrlsh.index import QueryIndex
    return QueryIndex(_rows(sig, compact), None, b, keys=keys, K=K, lists=None if lists is None else _dev(lists))


def _device_full(sig, b, K, compact=False):
    """the full path over all rows from a signature matrix: what pipeline.query_similarities runs after MinHash"""
    from qrlsh import ops
    rows = _rows(sig, compact)
    n, P = rows.shape
    keys, norm2 = ops.band_keys(ops.sig_to_int32(rows), b, want_norm=True)
    pairs = ops.candidate_pairs(keys, P // b, sig=rows)
    ib = ops.id_bits_for(n)
    milli, rev = ops.score_pairs_rev(rows, norm2, pairs, ib)
    return _host(ops.topk_select(pairs, milli, rev, K, ib, n))


def _updated(sig, b, K, bounds, compact=False, stored=None, keys=None):
    """lists of sig[:bounds[0]] (the oracle's, or `stored`) held by an index, then one append per further bound"""
    n = bounds[0]
    kk = (lambda lo, hi: None) if keys is None else (lambda lo, hi: keys[:, lo:hi].contiguous())
    qi = _index(sig[:n], b, K, compact, LC.full_lists(sig[:n], b, K) if stored is None else stored, keys=kk(0, n))
    for e in bounds[1:]:
        assert qi.append(_rows(sig[n:e], compact), keys=kk(n, e), update_lists=True) == (n, e - n)
        n = e
    assert qi.n == n and qi.lists_K == K
    return qi


def _assert_lists(got, want, what):
    got = _host(got) if isinstance(got[0], torch.Tensor) else got
    for g, w, name in zip(got, want, ("src", "dst", "val")):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


# ------------------------------------------------------------------------------------------------ 1. crowded rows
@pytest.fixture(scope="module")
def crowded_refs():
    """per shape: (sig, the oracle's lists over all rows, the device's full path over all rows per row format)"""
    out = {}
    c = LC.CROWDED
    for hi in (3, 40):
        sig = LC.crowded(hi)
        out[hi] = (sig, LC.full_lists(sig, c["b"], c["K"]), {f: _device_full(sig, c["b"], c["K"], f) for f in FORMATS})
    return out


@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("hi", [3, 40])
@pytest.mark.parametrize("n", [0, 40, 300, 339])
def test_crowded_and_sparse_rows(crowded_refs, n, hi, compact):
    c = LC.CROWDED
    sig, oracle_all, device_all = crowded_refs[hi]
    _assert_lists(device_all[compact], oracle_all, "the full path itself")
    qi = _updated(sig, c["b"], c["K"], [n, c["N"]], compact)
    stored = LC.full_lists(sig[:n], c["b"], c["K"])
    _assert_lists(qi.lists, LC.restate_update(stored, sig, n, c["N"] - n, c["b"], c["K"]), "restatement")
    _assert_lists(qi.lists, device_all[compact], "full path")


@pytest.mark.parametrize("compact", FORMATS)
def test_one_batch_three_batches_and_forty_single_appends(crowded_refs, compact):
    c = LC.CROWDED
    for hi in (3, 40):
        sig, oracle_all, device_all = crowded_refs[hi]
        for bounds in ([300, 340], [300, 313, 326, 340], list(range(300, 341))):
            qi = _updated(sig, c["b"], c["K"], bounds, compact)
            _assert_lists(qi.lists, oracle_all, (hi, len(bounds)))
            _assert_lists(qi.lists, device_all[compact], (hi, len(bounds)))


# ------------------------------------------------------------------------------------------------ 2. a popular key
@pytest.fixture(scope="module")
def popular_ref():
    """(sig, the stored lists of the old rows, the restated update, new neighbours of old rows 0 .. 2): computed once"""
    p = LC.POPULAR
    sig = LC.popular()
    n, m, b, K = p["n"], p["m"], p["b"], p["K"]
    stored = LC.full_lists(sig[:n], b, K)
    s, d, v = LC.new_pairs(sig, n, m, b, K)
    want = LC.cut(np.concatenate((stored[0], s)), np.concatenate((stored[1], d)), np.concatenate((stored[2], v)), K)
    return sig, stored, want, [int(((s == i) & (d >= n)).sum()) for i in range(3)]


@pytest.mark.parametrize("compact", FORMATS)
def test_popular_key_in_both_directions(popular_ref, compact):
    p = LC.POPULAR
    n, m, b, K = p["n"], p["m"], p["b"], p["K"]
    sig, stored, want, met = popular_ref
    # old rows 0 .. 2 meet 4200 new queries under the planted key: reverse runs beyond the 4096 keys of the select image
    assert all(c > 4200 for c in met)
    qi = _updated(sig, b, K, [n, n + m], compact, stored=stored)
    _assert_lists(qi.lists, want, "restatement")
    _assert_lists(qi.lists, _device_full(sig, b, K, compact), "full path")


# ------------------------------------------------------------------------------------------------ 3. wide bands
@pytest.mark.parametrize("collide", [False, True])
@pytest.mark.parametrize("compact", FORMATS)
def test_wide_bands_and_colliding_caller_keys(compact, collide):
    c = LC.WIDE
    sig = LC.wide()
    n, N, b, K = c["n"], c["N"], c["b"], c["K"]
    keys = torch.zeros((b, N), dtype=torch.int64, device="cuda") if collide else None
    qi = _updated(sig, b, K, [n, N], compact, keys=keys)
    _assert_lists(qi.lists, LC.restate_update(LC.full_lists(sig[:n], b, K), sig, n, N - n, b, K), "restatement")
    _assert_lists(qi.lists, _device_full(sig, b, K, compact), "full path")


# ------------------------------------------------------------------------------------------------ 4. goldens
@pytest.mark.parametrize("name", QC.HOLDOUT_SETS)
def test_golden_holdouts(name):
    g, sig, b, K = next((g, sig, b, K) for nm, g, sig, b, K in QC.golden_sets() if nm == name)
    N = sig.shape[0]
    want = LC.full_lists(sig, b, K)
    fits = sig.min() >= -1 and sig.max() < 65535       # wrap fixtures: int32 rows only
    for compact in (FORMATS if fits else [False]):
        full = _device_full(sig, b, K, compact)
        _assert_lists(full, want, (name, "the full path itself"))
        for h in (1, 3, N // 2):
            qi = _updated(sig, b, K, [N - h, N], compact)
            _assert_lists(qi.lists, want, (name, compact, h, "oracle"))
            _assert_lists(qi.lists, full, (name, compact, h, "full path"))
            if h <= 3:
                stored = LC.full_lists(sig[:N - h], b, K)
                _assert_lists(qi.lists, LC.restate_update(stored, sig, N - h, h, b, K), (name, compact, h, "restatement"))


# ------------------------------------------------------------------------------------------------ 5. tile boundaries
@pytest.mark.parametrize("compact", FORMATS)
def test_stored_lists_that_end_on_a_tile_boundary(compact):
    """the fill works the stored entries in steps of 1024 (4 per lane, 256 lanes): lists trimmed to 255, 256, 257 entries
    (the sparse shape) and to 1023, 1024, 1025 (the crowded one); a trimmed list is still a list, its last row shorter"""
    c = LC.CROWDED
    n, N, b, K = 300, c["N"], c["b"], c["K"]
    for hi, sizes in ((40, (255, 256, 257)), (3, (1023, 1024, 1025))):
        sig = LC.crowded(hi)
        stored = LC.full_lists(sig[:n], b, K)
        assert len(stored[0]) > max(sizes)
        for E in sizes:
            cutl = tuple(a[:E] for a in stored)
            qi = _updated(sig, b, K, [n, N], compact, stored=cutl)
            _assert_lists(qi.lists, LC.restate_update(cutl, sig, n, N - n, b, K), (hi, E))


# ------------------------------------------------------------------------------------------------ 6. self exclusion
@pytest.mark.parametrize("compact", FORMATS)
def test_neighbours_of_indexed_queries_leave_the_query_itself_out(compact):
    rng = np.random.default_rng(31)
    P, b, K = 32, 8, 6
    sig = rng.integers(0, 5, size=(900, P)).astype(np.int32)
    sig[100:110] = sig[50]                               # duplicate rows, different ids
    sig[7] = -1
    qi = _index(sig, b, K, compact)
    first, m = 40, 80
    off, idx, milli, avail = (t.cpu().numpy() for t in qi.neighbours_of(first, m))
    plain = [t.cpu().numpy() for t in qi.neighbours(_rows(sig[first:first + m], compact))]
    for x in range(m):
        q = first + x
        ids = QC.restate_candidates(sig, b, sig[q])
        assert q in ids
        ids = ids[ids != q]
        mi = QC.restate_scores(sig, ids, sig[q])
        order = np.lexsort((ids, -mi))[:K]
        assert avail[x] == len(ids) == plain[3][x] - 1, q
        assert np.array_equal(idx[off[x]:off[x + 1]], ids[order]) and np.array_equal(milli[off[x]:off[x + 1]], mi[order]), q
    # duplicates stay each other's neighbours at 1000, the query itself is gone
    x = 50 - first
    got = idx[off[x]:off[x + 1]].tolist()
    assert got == list(range(100, 100 + K)) and (milli[off[x]:off[x + 1]] == 1000).all() and 50 not in got
    # a query without a non-empty band finds nothing, itself included
    o7 = [t.cpu().numpy() for t in qi.neighbours_of(7, 1)]
    assert o7[3][0] == 0 and o7[0].tolist() == [0, 0]
    # the plain probe is what it was
    want = QC.restate_probe(sig, b, sig[first:first + m], K)
    for x, (wi, wm, wa) in enumerate(want):
        assert plain[3][x] == wa and np.array_equal(plain[1][plain[0][x]:plain[0][x + 1]], wi) and \
            np.array_equal(plain[2][plain[0][x]:plain[0][x + 1]], wm)
    assert wi[0] == first + m - 1 and wm[0] == 1000      # a plain probe with an indexed row still finds it
    with pytest.raises(ValueError):
        qi.neighbours_of(890, 20)
    with pytest.raises(ValueError):
        qi.neighbours_of(0, 5, K=257)


# ------------------------------------------------------------------------------------------------ 7. volume
def test_a_million_indexed_and_16384_appended_in_four_batches():
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    nq, extra, D, P, b = 1 << 20, 16384, 20000, 128, 32
    offsets, rows = synth.synth_csr(nq + extra, D, seed=5)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=9))
    K = pipeline.max_candidates(nq)
    off_h = offsets.cpu().numpy()
    sub = lambda lo, hi: ((offsets[lo:hi + 1] - offsets[lo]).contiguous(), rows[int(off_h[lo]):int(off_h[hi])].contiguous())
    res = pipeline.query_similarities(*sub(0, nq), table, b, K)
    held = (res.src.clone(), res.dst.clone(), res.val.clone())
    qi = QueryIndex.from_result(res, table, lists=True)
    assert qi.lists[0] is res.src and qi.lists_K == K
    step = extra // 4
    for lo in range(nq, nq + extra, step):
        assert qi.add(*sub(lo, lo + step), update_lists=True) == (lo, step)
    assert all(torch.equal(a, h) for a, h in zip((res.src, res.dst, res.val), held))     # the run's tensors are not written
    del res, held
    full = pipeline.query_similarities(offsets, rows, table, b, K)
    for a, f, name in zip(qi.lists, (full.src, full.dst, full.val), ("src", "dst", "val")):
        assert a.dtype == f.dtype and a.shape == f.shape and torch.equal(a, f), name
    assert int((full.src >= nq).sum()) > 0 and qi.K == pipeline.max_candidates(nq)


# ------------------------------------------------------------------------------------------------ 8. Recommender
def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for q in a:
        assert a[q]["indexes"].dtype == b[q]["indexes"].dtype and np.array_equal(a[q]["indexes"], b[q]["indexes"]), q
        assert np.array_equal(a[q]["values"], b[q]["values"]), q


@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_keeps_its_lists_current(sub):
    from test_gpu_recommend import _recommender_on
    from qrlsh import pipeline
    full, g = _recommender_on(sub)
    N, nu = full.queriesIDs.size, full.usersIDs.size
    K = pipeline.max_candidates(N)
    full.max_candidates = K
    seed = int(g["seed"])
    want_sims = full.compute_querySimilarities()
    np.random.seed(seed)
    want_scores = full.compute_scores()

    def first_queries(n0):
        rec, _ = _recommender_on(sub)
        block = rec.ratings[:, n0:].copy()
        rest, ids = np.asarray(rec.queries, dtype=object)[n0:], rec.queriesIDs[n0:]
        rec.queries, rec.queriesIDs, rec.ratings = rec.queries[:n0], rec.queriesIDs[:n0], rec.ratings[:, :n0]
        rec.max_candidates = K
        np.random.seed(seed)
        return rec, rest, ids, block

    n0 = N - 9
    rec, rest, ids, block = first_queries(n0)
    with pytest.raises(ValueError):
        rec.current_query_similarities()                 # no run yet
    run = rec.compute_querySimilarities()
    _same_dict(rec.current_query_similarities(), run)    # before any append: the run's own lists
    res = rec.last_result
    held = (res.src.clone(), res.dst.clone(), res.val.clone())
    rec.add_queries(rest[:4], ratings=block[:, :4], ids=ids[:4], update_lists=True)
    rec.add_queries(rest[4:], ratings=block[:, 4:], ids=ids[4:], update_lists=True)
    assert rec.last_result is res and all(torch.equal(a, h) for a, h in zip((res.src, res.dst, res.val), held))
    assert rec.queriesIDs.size == N and np.array_equal(rec.ratings, full.ratings)
    _same_dict(rec.current_query_similarities(), want_sims)
    got = rec.compute_scores(reuse_lists=True)
    assert rec.last_result is res                        # no new run happened
    assert np.array_equal(got[0], want_scores[0]) and np.array_equal(got[2], want_scores[2])
    assert np.array_equal(got[1].to_numpy(), want_scores[1].to_numpy())
    assert list(got[1].columns) == list(want_scores[1].columns)
    # without the flag: as before, the live lists are dropped, and a later update raises
    rec, rest, ids, block = first_queries(n0)
    rec.compute_querySimilarities()
    rec.add_queries(rest[:4], ratings=block[:, :4], ids=ids[:4])
    assert rec._query_index.n == n0 + 4 and rec._query_index.lists is None and rec.last_result.src.numel() > 0
    with pytest.raises(ValueError):
        rec.add_queries(rest[4:], ratings=block[:, 4:], ids=ids[4:], update_lists=True)
    assert rec._query_index.n == n0 + 4 and rec.queriesIDs.size == n0 + 4
    with pytest.raises(ValueError):
        rec.current_query_similarities()


# ------------------------------------------------------------------------------------------------ 9. arguments
def test_argument_errors():
    from qrlsh import _lib, ops
    c = LC.CROWDED
    sig = LC.crowded(40)
    n, N, b, K = 300, c["N"], c["b"], c["K"]
    stored = LC.full_lists(sig[:n], b, K)
    new = _rows(sig[n:])
    # an index without lists; lists dropped by a plain append
    qi = _index(sig[:n], b, K)
    with pytest.raises(ValueError):
        qi.append(new, update_lists=True)
    assert qi.n == n
    qi = _index(sig[:n], b, K, lists=stored)
    qi.append(_rows(sig[n:n + 5]))
    assert qi.lists is None
    with pytest.raises(ValueError):
        qi.append(_rows(sig[n + 5:]), update_lists=True)
    # m = 0: the lists stay the same tensors
    qi = _index(sig[:n], b, K, lists=stored)
    held = qi.lists
    assert qi.append(_rows(sig[:0]), update_lists=True) == (n, 0) and qi.lists is held
    # lists the constructor refuses: not ordered by src, ids outside [0, n), dtype, device, K
    s, d, v = stored
    for bad in ((s[::-1].copy(), d, v), (s, np.where(d == d[0], n, d), v), (np.where(s == s[-1], n, s), d, v),
                (np.where(s == s[0], -1, s), d, v), (s[:-1], d, v)):
        with pytest.raises(ValueError):
            _index(sig[:n], b, K, lists=bad)
    from qrlsh.index import QueryIndex
    dl = _dev(stored)
    with pytest.raises(TypeError):
        QueryIndex(_rows(sig[:n]), None, b, K=K, lists=(dl[0].to(torch.int64), dl[1], dl[2]))
    with pytest.raises((TypeError, ValueError)):
        QueryIndex(_rows(sig[:n]), None, b, K=K, lists=(dl[0].cpu(), dl[1], dl[2]))
    with pytest.raises(ValueError):
        QueryIndex(_rows(sig[:n]), None, b, K=257, lists=dl)
    # the library itself: the same refusals on the device, through the one word that is read back
    qi = _index(sig, b, K)
    m = N - n
    keys = ops.band_keys(new, b)
    raw, pws = ops.index_probe(qi.keys, qi.ids, qi.dir, qi.r, keys)
    off, idx, milli, _, skeys = ops.index_finish(qi.sig, qi.norm2, new, None, b, pws, raw, K, first_id=n)
    args = (n, m, b, K, raw, skeys, off, idx, milli)
    want = LC.restate_update(stored, sig, n, m, b, K)
    _assert_lists(ops.lists_update(*dl, *args), want, "ops.lists_update")
    for bad in ((s[::-1].copy(), d, v), (s, np.where(d == d[0], n, d), v), (np.where(s == s[-1], n, s), d, v)):
        with pytest.raises(ValueError):
            ops.lists_update(*_dev(bad), *args)
    with pytest.raises(ValueError):
        ops.lists_update(*dl, n, m, b, 257, raw, skeys, off, idx, milli)
    with pytest.raises(TypeError):
        ops.lists_update(dl[0].to(torch.int64), dl[1], dl[2], *args)
    with pytest.raises((TypeError, ValueError)):
        ops.lists_update(dl[0].cpu(), dl[1], dl[2], *args)
    with pytest.raises(ValueError):
        ops.lists_update(dl[0], dl[1][:-1], dl[2], *args)
    same = ops.lists_update(*dl, n, 0, b, K, raw[:0], skeys[:0], off[:1], idx[:0], milli[:0])
    assert all(a is h for a, h in zip(same, dl))
    lib = _lib.load()
    vp = ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())
    total = torch.zeros((1,), dtype=torch.int64, device="cuda")
    rc = lib.qrlsh_lists_update_count(vp(), vp(), vp(), 0, 10, 5, 4, 257, vp(), vp(), 0, vp(), vp(), 0, p(total), vp())
    assert rc == _lib.QRLSH_EINVAL and b"K=257" in lib.qrlsh_last_error()
    rc = lib.qrlsh_lists_update_count(vp(), vp(), vp(), 0, 2**31 - 3, 5, 4, 8, vp(), vp(), 0, vp(), vp(), 0, p(total), vp())
    assert rc == _lib.QRLSH_EINVAL and b"2^31" in lib.qrlsh_last_error()
    ws = torch.empty((lib.qrlsh_lists_update_workspace_bytes(n, m, len(s), raw.numel()),), dtype=torch.uint8, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    rc = lib.qrlsh_lists_update_count(p(dl[0]), p(dl[1]), p(dl[2]), len(s), n, m, b, K, p(raw), p(skeys), raw.numel(), p(off),
                                      p(ws), ws.numel() - 1, p(total), st)
    assert rc == _lib.QRLSH_EWORKSPACE
    rc = lib.qrlsh_index_probe_finish_indexed(vp(), vp(), 10, vp(), vp(), 0, 16, 8, 5, 6, vp(), vp(), 0, 4, p(off), vp(), vp(),
                                              vp(), vp(), 0, st)
    assert rc == _lib.QRLSH_EINVAL and b"indexed" in lib.qrlsh_last_error()
