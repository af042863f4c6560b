"""Removing queries from a built index (qrlsh_idmap_*, qrlsh_rows_remove, qrlsh_index_remove, qrlsh_lists_remove_*,
qrlsh_index_probe_finish_rows, QueryIndex.remove, Recommender.remove_queries): every check is exact.  The device is held
to the numpy restatements (tests/index_remove_cases.py, tests/index_append_cases.py), to the oracle's lists over the
surviving rows, and to a fresh build / full run over them -- never to the removal itself."""
import ctypes

import numpy as np
import pytest
import torch

import index_append_cases as AC
import index_remove_cases as RC
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


def _assert_lists(got, want, what):
    got = _host(got) if isinstance(got[0], torch.Tensor) else got
    for g, w, name in zip(got, want, ("src", "dst", "val")):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


def _assert_layout(qi, layout, what):
    sk, ids, dirw = layout
    for t, w, name in ((qi.keys, sk, "keys"), (qi.ids, ids, "ids"), (qi.dir, dirw, "dir")):
        g = t.cpu().numpy().view(w.dtype)
        assert t.is_contiguous() and g.shape == w.shape and np.array_equal(g, w), (what, name, g.shape, w.shape)


def _assert_index(qi, sig, compact, what, keys=None):
    """the arrays of a fresh index over the rows `sig`: the restated layout of their band keys, the rows, their norms"""
    assert qi.n == sig.shape[0], what
    _assert_layout(qi, AC.restate_layout(AC.np_band_keys(sig, qi.b) if keys is None else keys), what)
    assert qi.sig.is_contiguous() and torch.equal(qi.sig, _rows(sig, compact)), (what, "sig")
    s = np.asarray(sig, dtype=np.int64)
    assert np.array_equal(qi.norm2.cpu().numpy(), (s * s).sum(axis=1)), (what, "norm2")


def _snapshot(qi):
    return {k: getattr(qi, k).clone() for k in ("keys", "ids", "dir", "sig", "norm2")}, tuple(t.clone() for t in qi.lists)


def _assert_snapshot(qi, snap, what):
    arrays, lists = snap
    for k, w in arrays.items():
        g = getattr(qi, k)
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape) and torch.equal(g, w), (what, k)
    _assert_lists(qi.lists, _host(lists), what)


# ------------------------------------------------------------------------------------------------ 1. crowded rows
@pytest.fixture(scope="module")
def crowded_refs():
    c = LC.CROWDED
    return {hi: (LC.crowded(hi), LC.full_lists(LC.crowded(hi), c["b"], c["K"])) for hi in (3, 40)}


@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("hi", [3, 40])
def test_index_byte_for_byte_and_lists_element_for_element(crowded_refs, hi, compact):
    c = LC.CROWDED
    N, b, K = c["N"], c["b"], c["K"]
    sig, stored = crowded_refs[hi]
    for name, given in RC.removal_sets(N).items():
        what = (hi, name, compact)
        pos = RC.new_positions(N, given)
        stay = pos >= 0
        qi = _index(sig, b, K, compact, lists=stored)
        new_pos = qi.remove(given if name != "even" else torch.from_numpy(given).cuda(), update_lists=True)
        assert new_pos.dtype == torch.int64 and new_pos.is_cuda and np.array_equal(new_pos.cpu().numpy(), pos), what
        _assert_index(qi, sig[stay], compact, what)
        want, picked = RC.restate_remove_lists(stored, sig, given, b, K)
        _assert_lists(qi.lists, want, (what, "restatement"))
        _assert_lists(qi.lists, LC.full_lists(sig[stay], b, K), (what, "oracle over the survivors"))
        assert qi.last_picked == len(picked) and qi.lists_K == K, (what, qi.last_picked, len(picked))
        # both branches are taken: full rows that are probed again, short rows that only lose entries
        if (hi, name) in RC.PICKED:
            assert len(picked) == RC.PICKED[(hi, name)] and (hi != 3 or len(picked) > 0), what
        if (hi, name) in RC.SHORT_LOST:
            assert RC.short_rows_that_lose(stored, N, given, K) == RC.SHORT_LOST[(hi, name)] > 0, what
        if name == "even":
            assert AC.dir_bits(N) == 6 and AC.dir_bits(qi.n) == 5 and qi.dir.numel() == b * 33
        if name == "all":
            assert qi.n == 0 and all(t.numel() == 0 for t in qi.lists)
            assert qi.append(_rows(sig[:50], compact), update_lists=True) == (0, 50)      # an empty index refills
            _assert_index(qi, sig[:50], compact, (what, "refilled"))
            _assert_lists(qi.lists, LC.full_lists(sig[:50], b, K), (what, "refilled"))
    # without the flag the lists are dropped, as append drops them
    qi = _index(sig, b, K, compact, lists=stored)
    qi.remove([5, 6])
    assert qi.lists is None and qi.n == N - 2 and qi.last_picked is None
    _assert_index(qi, np.delete(sig, [5, 6], axis=0), compact, (hi, compact, "no lists"))


# ------------------------------------------------------------------------------------------------ 2. round trips
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("hi", [3, 40])
def test_round_trips(crowded_refs, hi, compact):
    c = LC.CROWDED
    N, b, K = c["N"], c["b"], c["K"]
    sig, stored = crowded_refs[hi]
    n = 300
    # append a batch, remove exactly that batch: what it was before
    qi = _index(sig[:n], b, K, compact, lists=LC.full_lists(sig[:n], b, K))
    snap = _snapshot(qi)
    qi.append(_rows(sig[n:], compact), update_lists=True)
    new_pos = qi.remove(np.arange(n, N), update_lists=True)
    assert np.array_equal(new_pos.cpu().numpy(), np.concatenate((np.arange(n), np.full(N - n, -1))))
    _assert_snapshot(qi, snap, (hi, compact, "append then remove"))
    # remove, then append: a full run over the resulting rows
    given = RC.removal_sets(n)["random40"]
    stay = RC.new_positions(n, given) >= 0
    qi.remove(given, update_lists=True)
    qi.append(_rows(sig[n:], compact), update_lists=True)
    rows = np.concatenate((sig[:n][stay], sig[n:]))
    _assert_index(qi, rows, compact, (hi, compact, "remove then append"))
    _assert_lists(qi.lists, LC.full_lists(rows, b, K), (hi, compact, "remove then append"))
    # one call equals three successive calls, positions translated through new_pos
    given = np.unique(RC.removal_sets(N)["random40"])
    one = _index(sig, b, K, compact, lists=stored)
    one.remove(given, update_lists=True)
    three = _index(sig, b, K, compact, lists=stored)
    now = torch.arange(N, dtype=torch.int64, device="cuda")          # old id -> current id
    for part in (given[:13], given[13:26], given[26:]):
        step = three.remove(now[torch.from_numpy(part).cuda()], update_lists=True)
        now = torch.where(now >= 0, step[now.clamp(min=0)], now)
    assert np.array_equal(now.cpu().numpy(), RC.new_positions(N, given))
    _assert_snapshot(three, _snapshot(one), (hi, compact, "three calls"))


# ------------------------------------------------------------------------------------------------ 3. caller keys
@pytest.mark.parametrize("compact", FORMATS)
def test_wide_bands_and_colliding_caller_keys(compact):
    """the re-probe takes its keys from the index: with caller keys that all collide a recomputed key finds nothing"""
    c = LC.WIDE
    sig = LC.wide()
    N, b, K = c["N"], c["b"], c["K"]
    given = np.random.default_rng(5).choice(N, 60, replace=False)
    stay = RC.new_positions(N, given) >= 0
    stored = LC.full_lists(sig, b, K)
    want = LC.full_lists(sig[stay], b, K)
    for collide in (False, True):
        keys = torch.zeros((b, N), dtype=torch.int64, device="cuda") if collide else None
        qi = _index(sig, b, K, compact, lists=stored, keys=keys)
        qi.remove(given, update_lists=True)
        assert qi.last_picked > 0
        _assert_index(qi, sig[stay], compact, (compact, collide),
                      keys=np.zeros((b, int(stay.sum())), dtype=np.uint64) if collide else None)
        _assert_lists(qi.lists, want, (compact, collide, "oracle"))
        _assert_lists(qi.lists, _device_full(sig[stay], b, K, compact), (compact, collide, "full path"))


# ------------------------------------------------------------------------------------------------ 4. a popular key
def test_picked_rows_whose_candidates_stream_through_the_select():
    p = LC.POPULAR
    sig = LC.popular()
    N, b, K = p["n"] + p["m"], p["b"], p["K"]
    stored = _device_full(sig, b, K)
    planted = np.nonzero((sig[:, 2] == 7) & (sig[:, 3] == 9))[0]
    is_planted = np.zeros(N, dtype=bool)
    is_planted[planted] = True
    s, d = stored[0].astype(np.int64), stored[1].astype(np.int64)
    named = np.bincount(d[is_planted[s] & is_planted[d]], minlength=N)
    given = np.argsort(-named, kind="stable")[:50]           # the planted rows most often stored as neighbours
    assert named[given].min() > 0 and is_planted[given].all()
    stay = RC.new_positions(N, given) >= 0
    assert is_planted[stay].sum() - 1 > 4096                 # what a planted survivor meets under the planted key alone
    qi = _index(sig, b, K, lists=stored)
    qi.remove(given, update_lists=True)
    length = np.bincount(s, minlength=N)
    lost = np.bincount(s[~stay[d]], minlength=N)
    picked = (length == K) & (lost > 0) & stay
    assert qi.last_picked == picked.sum() and (picked & is_planted).sum() > 0
    _assert_lists(qi.lists, _device_full(sig[stay], b, K), "full path")


# ------------------------------------------------------------------------------------------------ 5. tile boundaries
@pytest.mark.parametrize("shift", [-1, 0, 1, "2T"])
def test_band_records_on_tile_boundaries(shift):
    """the band compaction works tiles of REMOVE_TILE records (8 per lane, 256 lanes); the rows move one 16-byte piece per
    lane, without a tile"""
    from qrlsh import _lib
    T = _lib.REMOVE_TILE
    n = 2 * T if shift == "2T" else T + shift
    P, b = 8, 4
    sig = np.random.default_rng(40 + n % 7).integers(0, 50, size=(n, P)).astype(np.int32)
    layout = AC.restate_layout(AC.np_band_keys(sig, b))
    band0 = layout[1][0].astype(np.int64)
    last = min(T, n) - 1
    for what, given in (("first record of a tile", band0[:1]), ("last record of a tile", band0[last:last + 1]),
                        ("first record of the second tile", band0[T:T + 1]), ("a whole tile", band0[:T])):
        if len(given) == 0:
            continue
        qi = _index(sig, b, 4)
        new_pos = qi.remove(given)
        assert np.array_equal(new_pos.cpu().numpy(), RC.new_positions(n, given)), (n, what)
        if len(given) == n:
            assert qi.n == 0
            continue
        _assert_layout(qi, RC.restate_remove_layout(layout, given), (n, what, "restatement"))
        _assert_index(qi, sig[RC.new_positions(n, given) >= 0], False, (n, what))


@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("P", [180, 6, 3, 1, 8])
def test_rows_of_every_width(P, compact):
    """rows move as the widest vector that divides their width: 16 bytes (P = 8 int32, 180 int32 = 720), 8 (P = 180 compact =
    360, P = 6 int32 = 24), 4 (P = 6 compact = 12, P = 3 and 1 int32), 2 (P = 3 and 1 compact); more than one block"""
    from qrlsh import ops
    n = 3000
    rng = np.random.default_rng(P)
    sig = rng.integers(-1, 60000, size=(n, P)).astype(np.int32)
    given = rng.choice(n, 700, replace=False)
    stay = RC.new_positions(n, given) >= 0
    rows = _rows(sig, compact)
    norm2 = torch.arange(n, dtype=torch.int64, device="cuda") * 7
    removed = ops.idmap_build(torch.from_numpy(given.astype(np.int32)).cuda(), n)
    got, gnorm = ops.rows_remove(rows, norm2, removed)
    keep = torch.from_numpy(stay).cuda()
    assert got.dtype == rows.dtype and got.is_contiguous() and torch.equal(got, rows[keep]) and torch.equal(gnorm, norm2[keep])
    qi = _index(sig, 1, 4, compact)          # and through the index
    qi.remove(given)
    _assert_index(qi, sig[stay], compact, (P, compact))


@pytest.mark.parametrize("compact", FORMATS)
def test_stored_lists_that_end_on_a_tile_boundary(compact):
    from qrlsh import _lib
    T = _lib.REMOVE_TILE
    N, P, b, K = 900, 16, 8, 4
    sig = np.random.default_rng(17).integers(0, 3, size=(N, P)).astype(np.int32)
    stored = LC.full_lists(sig, b, K)
    assert len(stored[0]) > T + 1
    for E in (T - 1, T, T + 1):
        cutl = tuple(a[:E] for a in stored)       # a trimmed list is still a list, its last row shorter
        for what, given in (("src of the first entry", cutl[0][:1]), ("dst of the tile's last entry", cutl[1][T - 2:T - 1]),
                            ("src of the last entry", cutl[0][-1:]), ("every row of the first 300", np.arange(300)),
                            ("a random 30", np.random.default_rng(E).choice(N, 30, replace=False))):
            qi = _index(sig, b, K, compact, lists=cutl)
            qi.remove(given, update_lists=True)
            want, picked = RC.restate_remove_lists(cutl, sig, given, b, K)
            assert qi.last_picked == len(picked), (E, what)
            _assert_lists(qi.lists, want, (E, what))


# ------------------------------------------------------------------------------------------------ 6. self exclusion
@pytest.mark.parametrize("compact", FORMATS)
def test_finish_rows_leaves_every_scattered_row_out_of_its_own_list(compact):
    from qrlsh import ops
    rng = np.random.default_rng(31)
    P, b, K = 32, 8, 6
    sig = rng.integers(0, 5, size=(900, P)).astype(np.int32)
    sig[100:110] = sig[50]                               # duplicate rows, different ids
    sig[7] = -1
    qi = _index(sig, b, K, compact)
    ids = np.array([899, 50, 105, 7, 0, 432, 100, 51])
    rows = torch.from_numpy(ids).cuda()
    psig, pnorm2 = qi.sig[rows], qi.norm2[rows]
    keys = ops.band_keys(ops.sig_to_int32(psig), b)
    raw, pws = ops.index_probe(qi.keys, qi.ids, qi.dir, qi.r, keys)
    off, idx, milli, avail = (t.cpu().numpy() for t in ops.index_finish_rows(qi.sig, qi.norm2, psig, pnorm2, b, pws, raw, K,
                                                                             rows.to(torch.int32)))
    for x, q in enumerate(ids.tolist()):
        cand = QC.restate_candidates(sig, b, sig[q])
        cand = cand[cand != q]
        mi = QC.restate_scores(sig, cand, sig[q])
        order = np.lexsort((cand, -mi))[:K]
        assert avail[x] == len(cand), q
        assert np.array_equal(idx[off[x]:off[x + 1]], cand[order]) and np.array_equal(milli[off[x]:off[x + 1]], mi[order]), q
        assert q not in idx[off[x]:off[x + 1]]
    x = 1                                                # row 50: its duplicates stay, at 1000
    assert idx[off[x]:off[x + 1]].tolist() == list(range(100, 100 + K)) and (milli[off[x]:off[x + 1]] == 1000).all()
    x = 2                                                # row 105: row 50 and the other duplicates, not itself
    assert idx[off[x]:off[x + 1]].tolist() == [50, 100, 101, 102, 103, 104]
    assert avail[3] == 0 and off[3] == off[4]            # no non-empty band: nothing, itself included


# ------------------------------------------------------------------------------------------------ 7. volume
def test_a_million_indexed_and_16384_removed():
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    nq, gone, D, P, b = 1 << 20, 16384, 20000, 128, 32
    offsets, rows = synth.synth_csr(nq, D, seed=5)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=9))
    K = pipeline.max_candidates(nq)
    res = pipeline.query_similarities(offsets, rows, table, b, K)
    held = (res.src.clone(), res.dst.clone(), res.val.clone())
    qi = QueryIndex.from_result(res, table, lists=True)
    given = torch.from_numpy(np.random.default_rng(3).choice(nq, gone, replace=False)).cuda()
    new_pos = qi.remove(given, update_lists=True)
    assert all(torch.equal(a, h) for a, h in zip((res.src, res.dst, res.val), held))     # the run's tensors are not written
    keep = torch.ones((nq,), dtype=torch.bool, device="cuda")
    keep[given] = False
    assert torch.equal(new_pos, torch.where(keep, torch.cumsum(keep, 0) - 1, torch.full_like(new_pos, -1)))
    assert qi.n == nq - gone and qi.last_picked > 0
    del res, held
    sizes = offsets[1:] - offsets[:-1]
    off2 = torch.cat((torch.zeros((1,), dtype=offsets.dtype, device="cuda"), torch.cumsum(sizes[keep], 0))).to(offsets.dtype)
    rows2 = rows[torch.repeat_interleave(keep, sizes)].contiguous()
    full = pipeline.query_similarities(off2.contiguous(), rows2, table, b, K)
    for a, f, name in zip(qi.lists, (full.src, full.dst, full.val), ("src", "dst", "val")):
        assert a.dtype == f.dtype and a.shape == f.shape and torch.equal(a, f), name
    fresh = QueryIndex.from_result(full, table)
    for name in ("keys", "ids", "dir", "sig", "norm2"):
        a, f = getattr(qi, name), getattr(fresh, name)
        assert a.dtype == f.dtype and tuple(a.shape) == tuple(f.shape) and torch.equal(a, f), name


# ------------------------------------------------------------------------------------------------ 8. Recommender
def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for q in a:
        assert a[q]["indexes"].dtype == b[q]["indexes"].dtype and np.array_equal(a[q]["indexes"], b[q]["indexes"]), q
        assert np.array_equal(a[q]["values"], b[q]["values"]), q


@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_serves_the_shrunk_set(sub):
    from test_gpu_recommend import _recommender_on
    from qrlsh import pipeline
    rec, g = _recommender_on(sub)
    N = rec.queriesIDs.size
    K = pipeline.max_candidates(N)
    seed = int(g["seed"])
    given = np.array([0, N // 2, 3, N - 1, 3, N // 3])
    pos = RC.new_positions(N, given)
    keep = pos >= 0
    fresh, _ = _recommender_on(sub)
    fresh.queries, fresh.queriesIDs = np.asarray(fresh.queries, dtype=object)[keep], fresh.queriesIDs[keep]
    fresh.ratings = np.ascontiguousarray(fresh.ratings[:, keep])
    fresh.max_candidates = K
    np.random.seed(seed)
    want_sims = fresh.compute_querySimilarities()
    np.random.seed(seed)
    want_scores = fresh.compute_scores()

    rec.max_candidates = K
    np.random.seed(seed)
    with pytest.raises(ValueError):
        rec.remove_queries(given)                        # no run yet
    rec.compute_querySimilarities()
    res = rec.last_result
    with pytest.raises(ValueError):
        rec.remove_queries([N], update_lists=True)
    assert rec.queriesIDs.size == N and rec._query_index.n == N
    got_pos = rec.remove_queries(given, update_lists=True)
    assert isinstance(got_pos, np.ndarray) and got_pos.dtype == np.int64 and np.array_equal(got_pos, pos)
    assert rec.last_result is res
    assert np.array_equal(rec.queriesIDs, fresh.queriesIDs) and np.array_equal(rec.ratings, fresh.ratings)
    assert np.array_equal(np.asarray(rec.queries, dtype=object), fresh.queries)
    _same_dict(rec.current_query_similarities(), want_sims)
    got = rec.compute_scores(reuse_lists=True)
    assert rec.last_result is res                        # no new run happened
    assert np.array_equal(got[0], want_scores[0]) and np.array_equal(got[2], want_scores[2])
    assert np.array_equal(got[1].to_numpy(), want_scores[1].to_numpy())
    assert list(got[1].columns) == list(want_scores[1].columns)
    # the new-query surface sees the shrunk set
    sims = rec.similar_queries(np.asarray(fresh.queries, dtype=object)[:3])
    assert all(int(v["indexes"].max()) < N - len(np.unique(given)) for v in sims.values())
    # without the flag the live lists are dropped, and a later update raises
    rec.remove_queries([1])
    assert rec._query_index.lists is None and rec.queriesIDs.size == N - len(np.unique(given)) - 1
    with pytest.raises(ValueError):
        rec.remove_queries([0], update_lists=True)
    with pytest.raises(ValueError):
        rec.current_query_similarities()


# ------------------------------------------------------------------------------------------------ 9. arguments
def test_argument_errors():
    from qrlsh import _lib, ops
    c = LC.CROWDED
    sig = LC.crowded(40)
    N, b, K = c["N"], c["b"], c["K"]
    stored = LC.full_lists(sig, b, K)
    # an id out of range: ValueError, the index unchanged
    qi = _index(sig, b, K, lists=stored)
    snap = _snapshot(qi)
    for bad in ([N], [-1], [3, 2**40], np.array([0, N + 5])):
        with pytest.raises(ValueError):
            qi.remove(bad, update_lists=True)
        with pytest.raises(ValueError):
            qi.remove(bad)
    with pytest.raises(ValueError):
        qi.remove([0.5])
    assert qi.n == N
    _assert_snapshot(qi, snap, "after refused removals")
    # no ids: nothing happens, the lists stay the same tensors
    held = qi.lists
    assert torch.equal(qi.remove([], update_lists=True), torch.arange(N, device="cuda")) and qi.lists is held
    assert torch.equal(qi.remove(np.empty(0, dtype=np.int64)), torch.arange(N, device="cuda")) and qi.lists is held
    # update_lists=True without lists
    with pytest.raises(ValueError):
        _index(sig, b, K).remove([1], update_lists=True)
    qi.remove([1])
    with pytest.raises(ValueError):
        qi.remove([2], update_lists=True)
    # the library itself
    lib = _lib.load()
    vp = ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())
    st = vp(torch.cuda.current_stream().cuda_stream)
    out2 = torch.zeros((2,), dtype=torch.int64, device="cuda")
    ids = torch.tensor([5, 9, 5, 339, 0], dtype=torch.int32, device="cuda")
    removed = ops.idmap_build(ids, N)
    assert removed.count == 4 and removed.members().tolist() == [0, 5, 9, 339]
    assert np.array_equal(removed.positions().cpu().numpy(), RC.new_positions(N, [0, 5, 9, 339]))
    with pytest.raises(ValueError):
        ops.idmap_build(torch.tensor([5, N], dtype=torch.int32, device="cuda"), N)
    rc = lib.qrlsh_idmap_build(p(ids), 5, N, p(removed.ws), lib.qrlsh_idmap_workspace_bytes(N) - 1, p(out2), st)
    assert rc == _lib.QRLSH_EWORKSPACE
    dl = _dev(stored)
    pick = torch.empty((lib.qrlsh_idmap_workspace_bytes(N),), dtype=torch.uint8, device="cuda")
    for badK in (0, 257):
        rc = lib.qrlsh_lists_remove_mark(p(dl[0]), p(dl[1]), len(stored[0]), N, badK, p(removed.ws), p(pick), p(out2), st)
        assert rc == _lib.QRLSH_EINVAL and b"K=%d" % badK in lib.qrlsh_last_error()
        rc = lib.qrlsh_lists_remove_count(p(dl[0]), p(dl[1]), p(dl[2]), len(stored[0]), N, badK, p(removed.ws), vp(), vp(), 0,
                                          p(pick), pick.numel(), p(out2), st)
        assert rc == _lib.QRLSH_EINVAL and b"K=%d" % badK in lib.qrlsh_last_error()
    rc = lib.qrlsh_lists_remove_mark(vp(), vp(), 0, 2**31, 4, p(removed.ws), p(pick), p(out2), st)
    assert rc == _lib.QRLSH_EINVAL and b"2^31" in lib.qrlsh_last_error()
    ws = torch.empty((lib.qrlsh_lists_remove_workspace_bytes(N, len(stored[0])),), dtype=torch.uint8, device="cuda")
    rc = lib.qrlsh_lists_remove_count(p(dl[0]), p(dl[1]), p(dl[2]), len(stored[0]), N, K, p(removed.ws), vp(), vp(), 0, p(ws),
                                      ws.numel() - 1, p(out2), st)
    assert rc == _lib.QRLSH_EWORKSPACE
    full = _index(sig, b, K)
    ko, io = torch.empty((b, N - 4), dtype=torch.int64, device="cuda"), torch.empty((b, N - 4), dtype=torch.int32, device="cuda")
    do = torch.empty((lib.qrlsh_index_dir_words(N - 4, b),), dtype=torch.int32, device="cuda")
    ws = torch.empty((lib.qrlsh_index_remove_workspace_bytes(N, b),), dtype=torch.uint8, device="cuda")
    args = lambda nbytes: (p(full.keys), p(full.ids), N, b, p(removed.ws), 4, vp(), 0, p(ko), p(io), p(do), vp(), p(ws), nbytes, st)
    assert lib.qrlsh_index_remove(*args(ws.numel() - 1)) == _lib.QRLSH_EWORKSPACE
    assert lib.qrlsh_index_remove(*args(ws.numel())) == _lib.QRLSH_OK
    torch.cuda.synchronize()
    stay = RC.new_positions(N, [0, 5, 9, 339]) >= 0
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), AC.restate_layout(AC.np_band_keys(sig[stay], b))[0])
    # nothing removed / everything removed: nothing is written
    ko.fill_(-7)
    assert lib.qrlsh_index_remove(p(full.keys), p(full.ids), N, b, p(removed.ws), 0, vp(), 0, p(ko), p(io), p(do), vp(), p(ws),
                                  ws.numel(), st) == _lib.QRLSH_OK
    assert lib.qrlsh_index_remove(p(full.keys), p(full.ids), N, b, p(removed.ws), N, vp(), 0, vp(), vp(), vp(), vp(), vp(), 0,
                                  st) == _lib.QRLSH_OK
    torch.cuda.synchronize()
    assert bool((ko == -7).all())
    rc = lib.qrlsh_rows_remove(p(full.sig), 25, vp(), N, p(removed.ws), p(ko), vp(), st)
    assert rc == _lib.QRLSH_EINVAL and b"multiple of 2" in lib.qrlsh_last_error()
    # stored lists that break the contract: refused through the word that is read back
    s, d, v = stored
    for bad in ((s[::-1].copy(), d, v), (s, np.where(d == d[0], N, d), v)):
        with pytest.raises(ValueError):
            ops.lists_remove_mark(*_dev(bad)[:2], N, K, removed)
