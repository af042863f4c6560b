"""Replacing queries of a built index in place (qrlsh_rows_replace, qrlsh_index_replace, qrlsh_lists_replace_*,
QueryIndex.replace / set, Recommender.replace_queries): every check is exact.  The device is held to the numpy
restatements (tests/index_replace_cases.py, tests/index_append_cases.py), to the oracle's lists over the new rows, and to
a fresh build / full run over them -- never to the replacement itself."""
import numpy as np
import pytest
import torch

import index_append_cases as AC
import index_replace_cases as PC
import lists_update_cases as LC
from test_gpu_index_remove import (FORMATS, _assert_index, _assert_layout, _assert_lists, _assert_snapshot, _dev,
                                   _device_full, _host, _index, _rows, _same_dict, _snapshot)

pytestmark = pytest.mark.gpu


def _replace(qi, ids, rows_new, compact, **kw):
    return qi.replace(ids, _rows(rows_new, compact), **kw)


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
    from qrlsh.index import QueryIndex
    sig, stored = crowded_refs[hi]
    layout = AC.restate_layout(AC.np_band_keys(sig, b))
    for name, case in PC.replacement_sets(N).items():
        what = (hi, name, compact)
        ids, rows_new = case[0], PC.new_rows(sig, case)
        rows = PC.overwritten(sig, ids, rows_new)
        given_rows, given_lists = _rows(sig, compact), _dev(stored)
        held = given_rows.clone()
        qi = QueryIndex(given_rows, None, b, K=K, lists=given_lists)
        _replace(qi, ids if name != "even" else torch.from_numpy(ids).cuda(), rows_new, compact, update_lists=True)
        # the tensors given to the constructor are never written
        assert torch.equal(given_rows, held) and qi.sig.data_ptr() != given_rows.data_ptr(), what
        _assert_lists(given_lists, stored, (what, "constructor lists"))
        _assert_layout(qi, PC.restate_replace_layout(layout, ids, AC.np_band_keys(rows_new, b)), (what, "restatement"))
        _assert_index(qi, rows, compact, what)
        want, picked = PC.restate_replace_lists(stored, sig, ids, rows_new, b, K)
        _assert_lists(qi.lists, want, (what, "restatement"))
        _assert_lists(qi.lists, LC.full_lists(rows, b, K), (what, "oracle over the new rows"))
        _assert_lists(qi.lists, _device_full(rows, b, K, compact), (what, "full path"))
        assert qi.last_picked == len(picked) == PC.PICKED[(hi, name)] and qi.lists_K == K, (what, qi.last_picked)
        if case[1] == "self":
            _assert_lists(qi.lists, stored, (what, "unchanged"))
    # without the flag the lists are dropped, as append and remove drop them
    qi = _index(sig, b, K, compact, lists=stored)
    case = PC.replacement_sets(N)["random40"]
    _replace(qi, case[0], PC.new_rows(sig, case), compact)
    assert qi.lists is None and qi.n == N and qi.last_picked is None
    _assert_index(qi, PC.overwritten(sig, case[0], PC.new_rows(sig, case)), compact, (hi, compact, "no lists"))
    # no ids: nothing happens
    qi = _index(sig, b, K, compact, lists=stored)
    held, snap = qi.lists, _snapshot(qi)
    assert _replace(qi, [], np.empty((0, c["P"]), dtype=np.int32), compact, update_lists=True) is None and qi.lists is held
    _assert_snapshot(qi, snap, "no ids")


@pytest.mark.parametrize("compact", FORMATS)
def test_stored_lists_that_end_on_a_tile_boundary(crowded_refs, compact):
    """the merge's fill works the stored entries in steps of 1024 (4 per lane, 256 lanes), with dropped ids as without:
    lists trimmed to 255, 256, 257 entries (the sparse shape) and to 1023, 1024, 1025 (the crowded one); a trimmed list
    is still a list, its last row shorter and the rows behind it empty.  Rows are picked at every size"""
    c = LC.CROWDED
    N, b, K = c["N"], c["b"], c["K"]
    case = PC.replacement_sets(N)["random40"]
    for hi, sizes in ((40, (255, 256, 257)), (3, (1023, 1024, 1025))):
        sig, stored = crowded_refs[hi]
        assert len(stored[0]) > max(sizes)
        ids, rows_new = case[0], PC.new_rows(sig, case)
        for E in sizes:
            cutl = tuple(a[:E] for a in stored)
            want, picked = PC.restate_replace_lists(cutl, sig, ids, rows_new, b, K)
            qi = _index(sig, b, K, compact, lists=cutl)
            _replace(qi, ids, rows_new, compact, update_lists=True)
            _assert_lists(qi.lists, want, (hi, E, compact))
            assert qi.last_picked == len(picked) > 0, (hi, E, compact)


# ------------------------------------------------------------------------------------------------ 2. band tiles
def test_band_records_on_tile_boundaries():
    """the band kernels work tiles of REMOVE_TILE records; few distinct values, so runs of equal mix bits straddle the
    tile edges.  Tiles with records that leave and none that arrives, with arrivals only, and with neither."""
    from qrlsh import _lib
    T = _lib.REMOVE_TILE
    n, P, b = 3 * T + 17, 8, 4
    rng = np.random.default_rng(44)
    sig = rng.integers(0, 3, size=(n, P)).astype(np.int32)
    keys = AC.np_band_keys(sig, b)
    layout = AC.restate_layout(keys)
    band0 = layout[1][0].astype(np.int64)
    top0 = AC.np_mix64(layout[0][0]) >> np.uint64(32)
    assert any(top0[e - 1] == top0[e] for e in (T, 2 * T, 3 * T))          # an equal-bit run across a tile edge
    edge = np.array([band0[0], band0[T - 1], band0[T], band0[2 * T - 1], band0[3 * T], band0[n - 1]])
    first_key_row = sig[band0[0]]                                          # its band-0 record sorts into tile 0
    last_key_row = sig[band0[n - 1]]
    cases = {
        "tile edges, random rows": (edge, rng.integers(0, 3, size=(len(edge), P)).astype(np.int32)),
        "tile edges, their own rows": (edge, sig[edge]),
        # ids of band 0's tile 1 leave and take the keys of the band's first and last record: in band 0 tile 1 only
        # loses and the new records land in the first and the last key's runs; the kinds of all tiles are checked below
        "leave one tile for another": (band0[T + 5:T + 45], np.where(np.arange(40)[:, None] % 2 == 0, first_key_row, last_key_row)),
        "a whole tile": (band0[T:2 * T], rng.integers(0, 3, size=(T, P)).astype(np.int32)),
    }
    for what, (ids, rows_new) in cases.items():
        qi = _index(sig, b, 4)
        qi.replace(ids, _rows(rows_new))
        _assert_layout(qi, PC.restate_replace_layout(layout, ids, AC.np_band_keys(rows_new, b)), (what, "restatement"))
        _assert_index(qi, PC.overwritten(sig, ids, rows_new), False, what)
    # the fill kernel's own view of every (band, tile) of that case: does a record leave it, does a batch record land
    # among its survivors (jlo < jhi)
    ids, rows_new = cases["leave one tile for another"]
    rid = np.sort(ids)
    bkeys = AC.np_band_keys(rows_new, b)[:, np.argsort(ids, kind="stable")]
    kinds = set()
    for t in range(b):
        gone = np.isin(layout[1][t].astype(np.int64), ids)
        surv = PC._composite(layout[0][t][~gone], layout[1][t][~gone])
        s_j = np.searchsorted(surv, np.sort(PC._composite(bkeys[t], rid)), side="left")
        before = np.concatenate(([0], np.cumsum(~gone)))
        for tile in range(4):
            base, end = before[tile * T], before[min((tile + 1) * T, n)]
            jlo, jhi = np.searchsorted(s_j, base, side="right"), np.searchsorted(s_j, end - 1, side="right")
            kinds.add((bool(gone[tile * T:(tile + 1) * T].any()), bool(end > base and jhi > jlo)))
    assert (True, False) in kinds and (False, True) in kinds and (False, False) in kinds, kinds
    gone0 = np.isin(band0, ids)
    assert gone0[T:2 * T].sum() == 40 and gone0.sum() == 40          # band 0: only tile 1 loses


# ------------------------------------------------------------------------------------------------ 3. a popular key
def test_reverse_runs_beyond_4096_and_rows_that_stream_through_the_select():
    """LC.POPULAR's recipe: a planted band tuple shared by 3 unreplaced ids and 4200 replaced ones.  The three hold that
    band alone (one more value each, so that they differ), so their stored rows are short, lose nothing and are NOT
    picked: each merges its 2 stored entries with a reverse run of 4200 records, most of them at tied values"""
    import query_index_cases as QC
    p = LC.POPULAR
    N, b, K = p["n"] + p["m"], p["b"], p["K"]
    rng = np.random.default_rng(12)
    sig = rng.integers(0, 6, size=(N, p["P"])).astype(np.int32)
    sig[:3] = -1
    sig[:3, 0] = (100, 101, 102)
    sig[:3, 2:4] = (7, 9)
    ids = np.sort(rng.choice(np.arange(3, N), p["planted"], replace=False))
    rows_new = rng.integers(0, 6, size=(len(ids), p["P"])).astype(np.int32)
    rows_new[:, 2:4] = (7, 9)
    rows_new[:4] = sig[0]                                    # copies of row 0: records at 1000, tied with stored entries
    stored = LC.full_lists(sig, b, K)
    rows = PC.overwritten(sig, ids, rows_new)
    in_r, length, lost = PC._row_facts(stored, N, ids, K)
    picked = (length == K) & (lost > 0) & ~in_r
    assert not picked[:3].any() and (length[:3] == 2).all() and picked.sum() > 0
    for i in range(3):                                       # the reverse run of row i: the replaced queries that name it
        cand = QC.restate_candidates(rows, b, rows[i])
        assert in_r[cand].sum() == len(ids) > 4096
    qi = _index(sig, b, K, lists=stored)
    qi.replace(ids, _rows(rows_new), update_lists=True)
    assert qi.last_picked == picked.sum()
    _assert_index(qi, rows, False, "popular")
    want = LC.full_lists(rows, b, K)
    _assert_lists(qi.lists, want, "oracle over the new rows")
    _assert_lists(qi.lists, _device_full(rows, b, K), "full path")
    s, d, v = want
    assert d[s == 0].tolist() == [1, 2] + ids[:3].tolist() and (v[s == 0] == 1000).all()      # ties by id, both ways


# ------------------------------------------------------------------------------------------------ 4. caller keys
@pytest.mark.parametrize("compact", FORMATS)
def test_wide_bands_and_colliding_caller_keys(compact):
    """picked rows take their keys from the index: with caller keys that all collide a recomputed key finds nothing"""
    c = LC.WIDE
    sig = LC.wide()
    N, b, K = c["N"], c["b"], c["K"]
    rng = np.random.default_rng(6)
    ids = rng.choice(N, 60, replace=False)
    rows_new = np.concatenate((rng.integers(0, 2, size=(40, c["P"])).astype(np.int32), sig[rng.choice(N, 20)]))
    rows = PC.overwritten(sig, ids, rows_new)
    stored = LC.full_lists(sig, b, K)
    want = LC.full_lists(rows, b, K)
    for collide in (False, True):
        keys = torch.zeros((b, N), dtype=torch.int64, device="cuda") if collide else None
        new_keys = torch.zeros((b, len(ids)), dtype=torch.int64, device="cuda") if collide else None
        qi = _index(sig, b, K, compact, lists=stored, keys=keys)
        qi.replace(ids, _rows(rows_new, compact), keys=new_keys, update_lists=True)
        assert qi.last_picked > 0
        _assert_index(qi, rows, compact, (compact, collide), keys=np.zeros((b, N), dtype=np.uint64) if collide else None)
        _assert_lists(qi.lists, want, (compact, collide, "oracle"))
        _assert_lists(qi.lists, _device_full(rows, b, K, compact), (compact, collide, "full path"))


# ------------------------------------------------------------------------------------------------ 5. row widths
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("P", [180, 6, 3, 8])
def test_rows_of_every_width(P, compact):
    """rows move as the widest vector that divides their width: 16 bytes (P = 8 int32), 8 (P = 180 compact = 360 bytes),
    4 (P = 6 compact, P = 3 int32), 2 (P = 3 compact); more than one block"""
    from qrlsh import ops
    n = 3000
    rng = np.random.default_rng(P)
    sig = rng.integers(-1, 60000, size=(n, P)).astype(np.int32)
    ids = np.sort(rng.choice(n, 700, replace=False))
    rows_new = rng.integers(-1, 60000, size=(700, P)).astype(np.int32)
    rows, norm2 = _rows(sig, compact), torch.arange(n, dtype=torch.int64, device="cuda") * 7
    new_norm2 = -torch.arange(700, dtype=torch.int64, device="cuda")
    ops.rows_replace(rows, norm2, torch.from_numpy(ids.astype(np.int32)).cuda(), _rows(rows_new, compact), new_norm2)
    want_norm = np.arange(n, dtype=np.int64) * 7
    want_norm[ids] = -np.arange(700)
    assert torch.equal(rows, _rows(PC.overwritten(sig, ids, rows_new), compact))
    assert np.array_equal(norm2.cpu().numpy(), want_norm)
    qi = _index(sig, 1, 4, compact)          # and through the index
    qi.replace(ids, _rows(rows_new, compact))
    _assert_index(qi, PC.overwritten(sig, ids, rows_new), compact, (P, compact))


# ------------------------------------------------------------------------------------------------ 6. round trips
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("hi", [3, 40])
def test_round_trips(crowded_refs, hi, compact):
    import index_remove_cases as RC
    c = LC.CROWDED
    N, b, K = c["N"], c["b"], c["K"]
    sig, _ = crowded_refs[hi]
    n = 300
    rows = sig[:n].copy()
    qi = _index(rows, b, K, compact, lists=LC.full_lists(rows, b, K))

    def check(what):
        _assert_index(qi, rows, compact, (hi, compact, what))
        _assert_lists(qi.lists, LC.full_lists(rows, b, K), (hi, compact, what))

    sets = PC.replacement_sets(n)
    for step, name in enumerate(("random40", "copy")):
        case = sets[name]
        rows_new = PC.new_rows(rows, case, seed=step)
        _replace(qi, case[0], rows_new, compact, update_lists=True)
        rows = PC.overwritten(rows, case[0], rows_new)
        check("replace " + name)
    qi.append(_rows(sig[n:], compact), update_lists=True)
    rows = np.concatenate((rows, sig[n:]))
    check("append")
    given = RC.removal_sets(N)["random40"]
    qi.remove(given, update_lists=True)
    rows = rows[RC.new_positions(N, given) >= 0]
    check("remove")
    case = PC.replacement_sets(len(rows))["even"]
    rows_new = PC.new_rows(rows, case)
    _replace(qi, case[0], rows_new, compact, update_lists=True)
    rows = PC.overwritten(rows, case[0], rows_new)
    check("replace after remove")
    # one call equals three successive calls
    case = sets["random40"]
    rows_new = PC.new_rows(sig[:n], case)
    one = _index(sig[:n], b, K, compact, lists=LC.full_lists(sig[:n], b, K))
    _replace(one, case[0], rows_new, compact, update_lists=True)
    three = _index(sig[:n], b, K, compact, lists=LC.full_lists(sig[:n], b, K))
    for lo, up in ((0, 13), (13, 26), (26, 40)):
        _replace(three, case[0][lo:up], rows_new[lo:up], compact, update_lists=True)
    _assert_snapshot(three, _snapshot(one), (hi, compact, "three calls"))


def test_set_takes_answer_sets_through_the_held_table():
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    nq, m, D, P, b, K = 700, 50, 2000, 32, 8, 5
    offsets, rows = synth.synth_csr(nq, D, seed=3)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=9))
    res = pipeline.query_similarities(offsets, rows, table, b, K)
    boff, brows = synth.synth_csr(m, D, seed=4)
    ids = np.random.default_rng(8).choice(nq, m, replace=False)
    by_set, by_replace = QueryIndex.from_result(res, table, lists=True), QueryIndex.from_result(res, table, lists=True)
    assert by_set.set(ids, boff, brows, update_lists=True) is None
    bsig, bnorm2, bkeys = by_replace.signatures(boff, brows)
    by_replace.replace(ids, bsig, bnorm2, bkeys, update_lists=True)
    _assert_snapshot(by_set, _snapshot(by_replace), "set")
    assert by_set.last_picked == by_replace.last_picked and torch.equal(by_set.sig[torch.from_numpy(ids).cuda()], bsig)
    # and both are the full run over the edited answer sets
    sizes = (offsets[1:] - offsets[:-1]).cpu().numpy()
    bsz = (boff[1:] - boff[:-1]).cpu().numpy()
    sets = np.split(rows.cpu().numpy(), np.cumsum(sizes)[:-1])
    for x, i in enumerate(ids.tolist()):
        sets[i] = brows.cpu().numpy()[int(boff[x]):int(boff[x]) + int(bsz[x])]
    off2 = torch.from_numpy(np.concatenate(([0], np.cumsum([len(a) for a in sets]))).astype(np.int64)).to(offsets.dtype).cuda()
    full = pipeline.query_similarities(off2, torch.from_numpy(np.concatenate(sets)).to(rows.dtype).cuda(), table, b, K)
    _assert_lists(by_set.lists, _host((full.src, full.dst, full.val)), "full run over the edited sets")
    assert torch.equal(by_set.sig, full.sig)


# ------------------------------------------------------------------------------------------------ 7. Recommender
@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_serves_the_edited_set(sub):
    from test_gpu_recommend import _recommender_on
    from test_gpu_recommend_users import _same_answers
    from qrlsh import pipeline
    rec, g = _recommender_on(sub)
    N, nu = rec.queriesIDs.size, rec.usersIDs.size
    K = pipeline.max_candidates(N)
    seed = int(g["seed"])
    positions = np.array([N - 1, 0, N // 2, 3, N // 3])
    queries = np.asarray(rec.queries, dtype=object)
    edited = queries[[1, 2, N // 2 + 1, N - 2, 5]].copy()          # texts other served queries hold: ties by id appear
    fresh, _ = _recommender_on(sub)
    fresh.queries = np.array(queries, copy=True)
    fresh.queries[positions] = edited
    fresh.max_candidates = K
    np.random.seed(seed)
    want_sims = fresh.compute_querySimilarities()

    rec.max_candidates = K
    np.random.seed(seed)
    with pytest.raises(ValueError):
        rec.replace_queries(positions, edited)                  # no run yet
    rec.compute_querySimilarities()
    res = rec.last_result
    held_sig = res.sig.clone()
    ids_before, ratings_before = rec.queriesIDs.copy(), np.array(rec.ratings, copy=True)
    for bad in ([N, 0, 1, 2, 3], [0, 0, 1, 2, 3], [0, 1, 2]):
        with pytest.raises(ValueError):
            rec.replace_queries(bad, edited, update_lists=True)
    assert np.array_equal(np.asarray(rec.queries, dtype=object), queries) and rec._query_index.n == N
    assert rec.replace_queries(positions, edited, update_lists=True) is None
    assert rec.last_result is res and torch.equal(res.sig, held_sig)
    assert np.array_equal(rec.queriesIDs, ids_before) and np.array_equal(rec.ratings, ratings_before)      # ratings=None keeps them
    assert np.array_equal(np.asarray(rec.queries, dtype=object), fresh.queries)
    _same_dict(rec.current_query_similarities(), want_sims)
    usim = type(rec).compute_userSimilarities(rec)
    rec.compute_userSimilarities = lambda: usim
    final = rec.compute_scores(reuse_lists=True)[1]
    assert rec.last_result is res
    users = [0, nu - 1, 7, 7, 3]
    _same_answers(rec.recommend_users(users, 7, user_sim=usim), rec.recommend(final, 7, users))
    # a ratings block overwrites the columns
    block = (np.arange(nu * 2).reshape(nu, 2) % 5).astype(np.int64)
    rec.replace_queries([4, 2], edited[:2], ratings=block, update_lists=True)
    want = ratings_before.copy()
    want[:, [4, 2]] = block
    assert np.array_equal(rec.ratings, want)
    fresh.queries[[4, 2]] = edited[:2]
    np.random.seed(seed)
    _same_dict(rec.current_query_similarities(), fresh.compute_querySimilarities())
    # without the flag the live lists are dropped, and a later update raises
    rec.replace_queries([1], edited[:1])
    assert rec._query_index.lists is None
    with pytest.raises(ValueError):
        rec.replace_queries([0], edited[:1], update_lists=True)
    with pytest.raises(ValueError):
        rec.current_query_similarities()


# ------------------------------------------------------------------------------------------------ 8. arguments
def test_argument_errors():
    from qrlsh import _lib
    c = LC.CROWDED
    sig = LC.crowded(40)
    N, b, K = c["N"], c["b"], c["K"]
    stored = LC.full_lists(sig, b, K)
    two = _rows(sig[:2])
    qi = _index(sig, b, K, lists=stored)
    snap = _snapshot(qi)
    for bad in ([5, 5], [0, N], [-1, 3], [3, 2**40]):          # duplicates, an id equal to n, ids outside
        with pytest.raises(ValueError):
            qi.replace(bad, two, update_lists=True)
        with pytest.raises(ValueError):
            qi.replace(bad, two)
    with pytest.raises(ValueError):
        qi.replace([0.5, 1.5], two)
    with pytest.raises(ValueError):
        qi.replace([1, 2, 3], two)                              # one id per row
    _assert_snapshot(qi, snap, "after refused replacements")
    # update_lists=True without lists
    bare = _index(sig, b, K)
    with pytest.raises(ValueError):
        bare.replace([1, 2], two, update_lists=True)
    # K above QRLSH_INDEX_MAX_K
    qi.lists_K = _lib.INDEX_MAX_K + 1
    with pytest.raises(ValueError):
        qi.replace([1, 2], two, update_lists=True)
    qi.lists_K = K
    _assert_snapshot(qi, snap, "after K = 257")
    # stored lists that break the contract: src not ascending, an id outside [0, n)
    s, d, v = stored
    for bad in ((s[::-1].copy(), d, v), (s, np.where(d == d[0], N, d), v)):
        qi.lists = _dev(bad)
        with pytest.raises(ValueError):
            qi.replace([1, 2], two, update_lists=True)
        for k, w in snap[0].items():
            assert torch.equal(getattr(qi, k), w), k
        _assert_lists(qi.lists, bad, "the broken lists stay as given")
    # the library itself: sizes and workspace
    import ctypes
    from qrlsh import ops
    lib = _lib.load()
    vp = ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())
    st = vp(torch.cuda.current_stream().cuda_stream)
    rids = torch.tensor([4, 9], dtype=torch.int32, device="cuda")
    rmap = ops.idmap_build(rids, N)
    nk = ops.band_keys(two, b)
    ko, io, do = torch.full_like(bare.keys, -7), torch.empty_like(bare.ids), torch.empty_like(bare.dir)
    ws = torch.empty((lib.qrlsh_index_replace_workspace_bytes(N, 2, b),), dtype=torch.uint8, device="cuda")
    args = lambda m, nbytes: (p(bare.keys), p(bare.ids), p(bare.dir), N, b, p(rmap.ws), p(rids), p(nk), m, vp(), 0, p(ko),
                              p(io), p(do), vp(), p(ws), nbytes, st)
    assert lib.qrlsh_index_replace(*args(2, ws.numel() - 1)) == _lib.QRLSH_EWORKSPACE
    assert lib.qrlsh_index_replace(*args(N + 1, ws.numel())) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_index_replace(*args(0, 0)) == _lib.QRLSH_OK           # m = 0: at once, nothing written
    torch.cuda.synchronize()
    assert bool((ko == -7).all())
    assert lib.qrlsh_index_replace(*args(2, ws.numel())) == _lib.QRLSH_OK
    torch.cuda.synchronize()
    want = AC.restate_layout(AC.np_band_keys(PC.overwritten(sig, [4, 9], sig[:2]), b))
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(io.cpu().numpy().view(np.uint32), want[1])
    rc = lib.qrlsh_rows_replace(p(bare.sig), 25, vp(), N, p(rids), p(two), vp(), 2, st)
    assert rc == _lib.QRLSH_EINVAL and b"multiple of 2" in lib.qrlsh_last_error()
