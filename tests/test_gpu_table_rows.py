"""Dataset rows come and go under a live index (qrlsh_table_rows_mark / _fill, qrlsh_bitmaps_set_rows, qrlsh.LiveTable,
Recommender.add_rows / remove_rows): every check is exact.  The kernels are held to the numpy restatements
(tests/table_rows_cases.py), the table and the index to a fresh recompute over the edited table in slot numbering -- answer
sets, MinHash, a fresh QueryIndex, the oracle's lists and the device's full run -- never to the row operation itself."""
import ctypes

import numpy as np
import pytest
import torch

import lists_update_cases as LC
import table_rows_cases as TC

pytestmark = pytest.mark.gpu

FORMATS = [False, True]      # int32 rows, compact uint16 rows


def _sig_dev(sig, compact):
    t = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.int32)).cuda()
    return t.bitwise_and(0xFFFF).to(torch.int16) if compact else t


def _sig_host(t):
    from qrlsh import ops
    return ops.sig_to_int32(t).cpu().numpy()


def _mark_and_fill(c, compact, force_i32=False):
    """the addition of case c through the two kernels -> (ids, rows int32, norm2, matched, changed count)"""
    from qrlsh import ops
    table = ops.perm_table(c.perms, force_i32=force_i32)
    cells, slots, _ = c.batch()
    batch = ops.RowBatch(cells, slots, "cuda")
    qrows = torch.from_numpy(c.qrows).cuda()
    sig = _sig_dev(c.sig, compact)
    held = sig.clone()
    changed, matched = ops.table_rows_mark(qrows, batch, table, sig)
    ids = changed.members()
    rows, norm2 = ops.table_rows_fill(qrows, batch, table, sig, ids)
    assert torch.equal(sig, held), "the sig passed in is never written"
    assert rows.dtype == sig.dtype and rows.is_contiguous()
    return ids.cpu().numpy().astype(np.int64), _sig_host(rows), norm2.cpu().numpy(), matched, changed.count


def _check_addition(c, compact, what, force_i32=False):
    ids, rows, norm2, matched, changed = _mark_and_fill(c, compact, force_i32)
    cells, _, tab_rows = c.batch()
    want_ids, want_rows = TC.restate_add(c.sig, c.qrows, cells, tab_rows)
    assert np.array_equal(ids, want_ids), (what, ids[:8], want_ids[:8])
    assert np.array_equal(rows, want_rows), what
    w = want_rows.astype(np.int64)
    assert norm2.dtype == np.int64 and np.array_equal(norm2, (w * w).sum(axis=1)), what
    assert (matched, changed) == (TC.matched_count(c.qrows, cells), len(want_ids)), what
    assert np.array_equal(want_rows, c.sig_after[want_ids]), what      # and that is MinHash over all D + m rows
    assert c.EMPTY in ids and (not c.quiet or c.QUIET not in ids), what
    assert matched >= changed and (not c.quiet or matched > changed), what     # matching alone does not list a query


# ------------------------------------------------------------------------------------------------ 1. mark and fill
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("P", [16, 180, 200])
def test_mark_and_fill_against_the_restatement(P, compact):
    """n = 1003 queries (not a multiple of 64, four workgroups), nfeat = 3 with 4 values each: most rows match many queries;
    m on every side of the 64-row tile; P = 200: four rounds of positions, the last one partial"""
    for m in TC.TILE_EDGES:
        c = TC.Case(n=1003, nfeat=3, nvals=4, P=P, D=50, m=m, seed=1000 + P + m)
        _check_addition(c, compact, (P, compact, m))


@pytest.mark.parametrize("nfeat", [1, 63])
def test_mark_and_fill_with_one_and_63_features(nfeat):
    for compact in FORMATS:
        c = TC.Case(n=300, nfeat=nfeat, nvals=2 if nfeat == 63 else 4, P=24, D=40, m=70, seed=nfeat)
        if nfeat == 63:        # random 63-feature queries match nothing: half of them take a few constraints of a batch row
            rng = np.random.default_rng(5)
            for q in range(3, c.n, 2):
                c.qrows[q] = -1
                f = rng.choice(nfeat, 2, replace=False)
                c.qrows[q, f] = c.cells[c.D + q % c.m, f]
            live = np.zeros(c.D + c.m, dtype=bool)
            live[:c.D] = True
            c.sig = TC.minhash(*TC.brute_answer_sets(c.cells, c.qrows, live), c.tab)
            c.sig_after = TC.minhash(*TC.brute_answer_sets(c.cells, c.qrows), c.tab)
        _check_addition(c, compact, (nfeat, compact))


def test_mark_and_fill_under_an_int32_table():
    c = TC.Case(n=500, nfeat=3, nvals=4, P=40, D=50, m=65, seed=77)
    _check_addition(c, False, "int32 table", force_i32=True)


# ------------------------------------------------------------------------------------------------ 2. the removal's mark
@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("keep_slot0", [True, False])
def test_remove_mark_is_exactly_the_queries_whose_minimum_sat_there(keep_slot0, compact):
    from qrlsh import ops
    for P, m in ((16, 65), (200, 5)):
        c = TC.Case(n=1003, nfeat=3, nvals=4, P=P, D=50, m=m, seed=P + m)
        gone = c.removal(keep_slot0, count=9 if m == 5 else 70, seed=m)
        table = ops.perm_table(c.perms)
        sig = _sig_dev(c.sig_after, compact)
        held = sig.clone()
        changed, matched = ops.table_rows_mark(torch.from_numpy(c.qrows).cuda(), ops.RowBatch(c.cells[gone], gone, "cuda"),
                                               table, sig, remove=True)
        ids = changed.members().cpu().numpy().astype(np.int64)
        assert torch.equal(sig, held)
        assert np.array_equal(ids, TC.restate_remove(c.sig_after, c.qrows, c.cells[gone], c.tab[gone])), (P, m)
        live = np.ones(c.D + c.m, dtype=bool)
        live[gone] = False
        after = TC.minhash(*TC.brute_answer_sets(c.cells, c.qrows, live), c.tab)
        assert np.array_equal(ids, np.nonzero((after != c.sig_after).any(axis=1))[0]), (P, m)
        assert (matched, changed.count) == (TC.matched_count(c.qrows, c.cells[gone]), len(ids))
        # matches a removed row whose values are nowhere its minimum: not marked
        assert TC.matches(c.qrows, c.cells[gone])[c.QUIET].any() and (c.QUIET in ids) == (not keep_slot0)
        assert matched >= changed.count and (not keep_slot0 or matched > changed.count)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _fresh(lt, table, b, compact):
    """(sig, norm2) of MinHash over the table's answer sets now, and the sets on the host"""
    from qrlsh import ops
    off, rows = lt.answer_sets()
    sig, norm2, _ = ops.minhash(off, rows, table, b=None, want_norm=True, compact=compact)
    return sig, norm2, off.cpu().numpy(), rows.cpu().numpy()


def _assert_fresh(qi, lt, table, compact, columns, live, what, lists=True):
    """the index and its lists are those of a fresh recompute over the edited table in slot numbering; the table's answer
    sets are the oracle's over the string table without the dead slots"""
    from oracle import oracle as O
    from test_gpu_index_remove import _assert_index, _assert_lists, _device_full
    sig, norm2, off, rows = _fresh(lt, table, qi.b, compact)
    D = len(live)
    qs = np.asarray(what[1], dtype=object).astype(str)
    woff, wrows = O.answer_sets([np.asarray(c[:D]).astype(str) for c in columns], qs)
    keep = live[wrows]
    owner = np.repeat(np.arange(len(woff) - 1), np.diff(woff))
    assert np.array_equal(rows, wrows[keep]), (what[0], "answer sets")
    assert np.array_equal(np.diff(off), np.bincount(owner[keep], minlength=len(woff) - 1)), (what[0], "answer set sizes")
    s = _sig_host(sig)
    _assert_index(qi, s, compact, what[0])
    assert torch.equal(qi.norm2, norm2), what[0]
    if lists:
        _assert_lists(qi.lists, LC.full_lists(s, qi.b, qi.lists_K), (what[0], "oracle"))
        _assert_lists(qi.lists, _device_full(s, qi.b, qi.lists_K, compact), (what[0], "full path"))
    return s


def _live_setup(compact, D=60, extra=30, cap=100):
    from qrlsh import ops
    from qrlsh.index import QueryIndex
    from qrlsh.table import LiveTable
    from test_gpu_index_remove import _dev
    c = LC.CROWDED
    columns, queries = TC.string_table(c["N"], D, extra)
    lt = LiveTable.build([col[:D] for col in columns], queries, capacity=cap)
    table = ops.perm_table(ops.legacy_permutations(c["P"], cap, seed=3))
    sig, norm2, _, _ = _fresh(lt, table, c["b"], compact)
    stored = LC.full_lists(_sig_host(sig), c["b"], c["K"])
    qi = QueryIndex(sig, norm2, c["b"], table=table, K=c["K"], lists=_dev(stored))
    rows = np.stack(columns, axis=1)
    return lt, table, qi, columns, queries, rows


@pytest.mark.parametrize("compact", FORMATS)
def test_rows_come_and_go_under_a_live_index(compact):
    D, extra = 60, 30
    lt, table, qi, columns, queries, rows = _live_setup(compact, D, extra)
    live = np.ones(D, dtype=bool)
    _assert_fresh(qi, lt, table, compact, columns, live, ("built", queries))
    # rows come: the first carries a value new to the table
    slots = lt.add_rows(rows[D:D + 20], qi, update_lists=True)
    assert slots.dtype == np.int64 and slots.tolist() == list(range(D, D + 20)) and lt.D == D + 20
    assert 0 < lt.last_changed <= lt.last_matched <= qi.n
    live = np.ones(D + 20, dtype=bool)
    _assert_fresh(qi, lt, table, compact, columns, live, ("added", queries))
    # a query that names the new value joins: the row that carries it answers
    newq = np.array([["", "fresh", ""], ["only", "", ""]], dtype=object)
    nq = lt.encode(newq)
    off, rws = lt.answer_sets(nq)
    assert rws[off[0]:off[1]].tolist() == [D] and rws[off[1]:off[2]].tolist() == [D - 1]
    qi.add(off, rws, update_lists=True)
    lt.add_queries(nq)
    queries = np.concatenate((queries, newq))
    _assert_fresh(qi, lt, table, compact, columns, live, ("query added", queries))
    # rows go: D - 1 is the last row of query 1 and of the query just added
    gone = np.array([D - 1, 3, D + 4, 17, D])
    lt.remove_rows(gone, qi, update_lists=True)
    live[gone] = False
    assert 0 < lt.last_changed <= lt.last_matched
    s = _assert_fresh(qi, lt, table, compact, columns, live, ("removed", queries))
    assert (s[1] == -1).all() and (s[-1] == -1).all() and (s[-2] == -1).all()      # they lost their last rows
    # an all-unconstrained query sees the live slots only
    off, rws = lt.answer_sets(np.full((1, 3), -1, dtype=np.int32))
    assert np.array_equal(rws.cpu().numpy(), np.nonzero(live)[0]) and int(off[1]) == live.sum()
    # more rows after the removal: slots are not reused
    slots = lt.add_rows(rows[D + 20:], qi, update_lists=True)
    assert slots.tolist() == list(range(D + 20, D + extra))
    live = np.concatenate((live, np.ones(extra - 20, dtype=bool)))
    _assert_fresh(qi, lt, table, compact, columns, live, ("added again", queries))
    # without the flag a changed query drops the lists, as replace does
    lt.remove_rows([0, 1, 2], qi)
    live[[0, 1, 2]] = False
    assert lt.last_changed > 0 and qi.lists is None
    _assert_fresh(qi, lt, table, compact, columns, live, ("no lists", queries), lists=False)


@pytest.mark.parametrize("compact", FORMATS)
def test_split_batches_equal_one_batch(compact, monkeypatch):
    from qrlsh import _lib
    from test_gpu_index_remove import _snapshot, _assert_snapshot
    D, extra = 60, 30
    one = _live_setup(compact, D, extra)
    one[0].add_rows(one[5][D:], one[2], update_lists=True)
    one[0].remove_rows(np.arange(5, 40), one[2], update_lists=True)
    monkeypatch.setattr(_lib, "TABLE_ROWS_MAX_M", 7)
    many = _live_setup(compact, D, extra)
    many[0].add_rows(many[5][D:], many[2], update_lists=True)
    many[0].remove_rows(np.arange(5, 40), many[2], update_lists=True)
    _assert_snapshot(many[2], _snapshot(one[2]), (compact, "split"))
    assert torch.equal(many[0].bitmaps[:many[0].dictionary.nrows], one[0].bitmaps[:one[0].dictionary.nrows])
    assert torch.equal(many[0].cells, one[0].cells)


def test_no_changed_query_leaves_index_and_lists_alone():
    from test_gpu_index_remove import _snapshot, _assert_snapshot
    lt, table, qi, columns, queries, rows = _live_setup(False)
    # drop the all-unconstrained query's effect: a row of values nobody names matches query 0 only -- make it constrained
    q0 = lt.encode(np.array([["f0v0", "", ""]], dtype=object))
    off, rws = lt.answer_sets(q0)
    qi.set([0], off, rws, update_lists=True)
    lt.set_queries([0], q0)
    held, snap = qi.lists, _snapshot(qi)
    for flag in (True, False):
        lt.add_rows(np.array([["nobody", "names", "these"]], dtype=object), qi, update_lists=flag)
        assert (lt.last_matched, lt.last_changed) == (0, 0)
        assert qi.lists is held                     # not even update_lists=False drops them
        _assert_snapshot(qi, snap, flag)
    lt.remove_rows([lt.D - 1], qi)
    assert (lt.last_matched, lt.last_changed) == (0, 0) and qi.lists is held
    _assert_snapshot(qi, snap, "removed")


# ------------------------------------------------------------------------------------------------ 4. Recommender
def _assert_recommender_fresh(rec, what):
    """rec's index and lists against a fresh run over its live table's answer sets (slot numbering, the run's table)"""
    from qrlsh import pipeline
    from qrlsh.index import QueryIndex
    lt, qi = rec._live_table, rec._query_index
    assert lt.n == qi.n == rec.queriesIDs.size, what
    off, rows = lt.answer_sets()
    full = pipeline.query_similarities(off, rows, rec.last_table, qi.b, qi.lists_K)
    assert full.sig.dtype == qi.sig.dtype
    for a, f, name in zip(qi.lists, (full.src, full.dst, full.val), ("src", "dst", "val")):
        assert a.dtype == f.dtype and a.shape == f.shape and torch.equal(a, f), (what, name)
    fresh = QueryIndex.from_result(full, rec.last_table)
    for name in ("keys", "ids", "dir", "sig", "norm2"):
        a, f = getattr(qi, name), getattr(fresh, name)
        assert a.dtype == f.dtype and tuple(a.shape) == tuple(f.shape) and torch.equal(a, f), (what, name)


@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_rows_come_and_go(sub):
    from test_gpu_recommend import _recommender_on
    from test_gpu_index_remove import _same_dict
    from qrlsh import pipeline
    full, g = _recommender_on(sub)
    N, Dfull = full.queriesIDs.size, full.dataset.shape[0]
    K = pipeline.max_candidates(N)
    seed = int(g["seed"])
    full.max_candidates = K
    np.random.seed(seed)
    want = full.compute_querySimilarities()

    rec, _ = _recommender_on(sub)
    tail = rec.dataset.iloc[Dfull - 8:]
    rec.dataset = rec.dataset.iloc[:Dfull - 8].reset_index(drop=True)
    rec.max_candidates = K
    with pytest.raises(ValueError):
        rec.add_rows(tail)                               # no run yet
    rec.row_capacity = Dfull
    np.random.seed(seed)
    rec.compute_querySimilarities()
    res = rec.last_result
    assert rec.last_table.D == Dfull
    pos = rec.add_rows(tail, update_lists=True)
    assert pos.dtype == np.int64 and pos.tolist() == list(range(Dfull - 8, Dfull)) and rec.last_result is res
    assert rec.dataset.equals(full.dataset) and np.array_equal(rec.row_slots, np.arange(Dfull))
    _same_dict(rec.current_query_similarities(), want)   # the same table draw: the reference-pinned run over all rows
    _assert_recommender_fresh(rec, (sub, "added"))
    with pytest.raises(ValueError, match="row_capacity"):
        rec.add_rows(tail.iloc[:1], update_lists=True)   # no free slot is left
    assert rec.dataset.shape[0] == Dfull
    # rows go
    given = np.array([0, Dfull - 1, 5, 5, Dfull // 2, 17])
    new_pos = rec.remove_rows(given, update_lists=True)
    keep = np.ones(Dfull, dtype=bool)
    keep[given] = False
    assert new_pos.dtype == np.int64 and np.array_equal(new_pos, np.where(keep, np.cumsum(keep) - 1, -1))
    assert rec.dataset.equals(full.dataset[keep].reset_index(drop=True)) and np.array_equal(rec.row_slots, np.nonzero(keep)[0])
    assert np.array_equal(rec._live_table.live, keep)
    _assert_recommender_fresh(rec, (sub, "removed"))
    # the query surface stays in step with the table
    q = np.asarray(rec.queries, dtype=object)
    rec.add_queries(q[:3], update_lists=True)
    rec.replace_queries([1, N - 1], q[[N - 1, 2]], update_lists=True)
    rec.remove_queries([4], update_lists=True)
    _assert_recommender_fresh(rec, (sub, "queries"))
    assert rec.queriesIDs.size == N + 2
    # the next run starts afresh
    rec.compute_querySimilarities()
    assert rec._live_table is None and rec.row_slots is None


def test_a_refused_query_call_after_dropped_lists_leaves_the_table_alone():
    """Found by the random schedules of test_gpu_live_sequence.py, cut down to its shortest form: under a live table, one
    call without update_lists drops the lists; add_queries / replace_queries(update_lists=True) is then refused -- and
    must be refused before its texts reach the table's dictionary (a value new to it used to get a dictionary entry and a
    bitmap row from the refused call)."""
    from test_gpu_recommend import _recommender_on
    rec, _ = _recommender_on("cfg2")
    rec.row_capacity = rec.dataset.shape[0] + 2
    rec.compute_querySimilarities()
    rec.remove_rows([3], update_lists=True)              # the live table exists from here on
    rec.remove_queries([1])                              # the lists are dropped
    lt, qi = rec._live_table, rec._query_index
    assert qi.lists is None
    held = (lt.bitmaps, lt.bitmaps.clone(), lt.dictionary.nrows, [dict(m) for m in lt.dictionary.maps], lt.qrows, lt.qrows.clone())
    n = rec.queriesIDs.size
    q = np.asarray(rec.queries, dtype=object)[:1].copy()
    q[0, 0] = "a value no row and no query holds"
    for call in (lambda: rec.add_queries(q, update_lists=True), lambda: rec.replace_queries([0], q, update_lists=True)):
        with pytest.raises(ValueError, match="dropped"):
            call()
        assert lt.bitmaps is held[0] and torch.equal(lt.bitmaps, held[1])
        assert lt.dictionary.nrows == held[2] and [dict(m) for m in lt.dictionary.maps] == held[3]
        assert lt.qrows is held[4] and torch.equal(lt.qrows, held[5]) and (qi.n, rec.queriesIDs.size) == (n, n)
    rec.add_queries(q)                                   # without the flag the call goes through, new value and all
    assert lt.dictionary.nrows == held[2] + 1 and rec.queriesIDs.size == n + 1 == qi.n


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors_leave_everything_as_it_was():
    from qrlsh import _lib, ops
    from qrlsh.table import LiveTable
    from test_gpu_index_remove import _snapshot, _assert_snapshot
    D, extra = 60, 30
    lt, table, qi, columns, queries, rows = _live_setup(False, D, extra, cap=70)
    snap, bits, cells = _snapshot(qi), lt.bitmaps.clone(), lt.cells.clone()

    def unchanged(what):
        _assert_snapshot(qi, snap, what)
        n = bits.shape[0]
        assert lt.D == D and torch.equal(lt.bitmaps[:n], bits) and torch.equal(lt.cells, cells), what
        assert not bool(lt.bitmaps[n:].any()) and lt.live.sum() == D, what

    with pytest.raises(ValueError):
        lt.add_rows(rows[D:D + 11], qi, update_lists=True)              # 11 rows, 10 free slots
    with pytest.raises(ValueError):
        lt.add_rows(rows[D:D + 2, :2], qi, update_lists=True)           # wrong column count
    with pytest.raises(ValueError):
        lt.add_rows(rows[D], qi, update_lists=True)                     # not [m, nfeat]
    for bad in ([D], [-1], [3, 3], [0.5]):
        with pytest.raises(ValueError):
            lt.remove_rows(bad, qi, update_lists=True)                  # never used, outside, duplicate, not an integer
    unchanged("refused")
    lt.remove_rows([7], qi, update_lists=True)
    dead = _snapshot(qi)
    with pytest.raises(ValueError):
        lt.remove_rows([7], qi, update_lists=True)                      # a dead slot
    with pytest.raises(ValueError):
        lt.remove_rows([8, 7], qi, update_lists=True)
    _assert_snapshot(qi, dead, "dead slot")
    assert lt.live.sum() == D - 1
    # a permutation table drawn for fewer rows than the slots asked for
    small = LiveTable.build([c[:D] for c in columns], queries, capacity=D + 5)
    qs = type(qi)(qi.sig.clone(), None, qi.b, table=ops.perm_table(ops.legacy_permutations(qi.P, D, seed=3)), K=qi.K)
    with pytest.raises(ValueError):
        small.add_rows(rows[D:D + 1], qs)
    with pytest.raises(ValueError):
        lt.add_rows(rows[D:D + 1], qs, update_lists=True)               # an index without lists
    assert small.D == D
    # an index out of step with the served queries
    short = type(qi)(qi.sig[:10].clone(), None, qi.b, table=table, K=qi.K)
    with pytest.raises(ValueError):
        lt.add_rows(rows[D:D + 1], short)
    # 64 features
    with pytest.raises(ValueError):
        LiveTable.build([np.array(["a"], dtype=object)] * 64, np.full((1, 64), "", dtype=object))
    with pytest.raises(ValueError):
        LiveTable.build([c[:D] for c in columns], queries, capacity=D - 1)
    # the library itself
    lib = _lib.load()
    vp = ctypes.c_void_p
    p = lambda t: vp(t.data_ptr())
    st = vp(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty((lib.qrlsh_idmap_workspace_bytes(qi.n),), dtype=torch.uint8, device="cuda")
    out2 = torch.zeros((2,), dtype=torch.int64, device="cuda")
    b = ops.RowBatch(np.ones((2, 3), dtype=np.int32), [0, 1], "cuda")
    for nfeat, m in ((64, 2), (0, 2), (3, 65537)):
        rc = lib.qrlsh_table_rows_mark(p(lt.qrows), qi.n, nfeat, p(b.cells), p(b.slots), m, p(table.tab), table.code, table.P,
                                       table.P_stride, p(qi.sig), _lib.SIG_I32, _lib.ROWS_ADD, p(ws), p(out2), st)
        assert rc == _lib.QRLSH_EINVAL and b"nfeat" in lib.qrlsh_last_error()
    # an empty batch: an empty map
    rc = lib.qrlsh_table_rows_mark(p(lt.qrows), qi.n, 3, vp(), vp(), 0, p(table.tab), table.code, table.P, table.P_stride,
                                   p(qi.sig), _lib.SIG_I32, _lib.ROWS_ADD, p(ws), p(out2), st)
    assert rc == _lib.QRLSH_OK and out2.tolist() == [0, 0]
    with pytest.raises(ValueError):
        ops.table_rows_mark(lt.qrows, ops.RowBatch(np.ones((1, 3), dtype=np.int32), [table.D], "cuda"), table, qi.sig)
    with pytest.raises(ValueError):
        ops.bitmaps_set_rows(lt.bitmaps, ops.RowBatch(np.full((1, 3), lt.bitmaps.shape[0], dtype=np.int32), [0], "cuda"), 0, True)
    with pytest.raises(ValueError):
        ops.RowBatch(np.ones((2, 3), dtype=np.int32), [4, 4], "cuda")
