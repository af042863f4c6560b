"""The postings of the answer sets and the exact lists served from them on the device (qrlsh_answer_postings,
qrlsh_exact_neighbours_postings, qrlsh.answer_postings, exact_neighbours(postings=...), Recommender.answer_postings /
exact_query_lists(postings=...)).  The postings are compared byte for byte with the numpy transpose of
tests/postings_cases.py, every output word of the lists with the restatements there and in tests/exactlists_cases.py, and
the sweep route (postings=None) is run beside the new one as a second oracle.  No tolerances.  The cases beyond one pass
(several halved windows beside more than 512 lists, single-id passes, probe chains, lane counts, late windows, a mixed
launch) prove on the CPU, in their builders, that they reach their path."""
import numpy as np
import pytest
import torch

import exactlists_cases as XC
import fidelity_cases as FC
import postings_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
FILL = 0xA5


def _build(case):
    import qrlsh
    return qrlsh.answer_postings(case.offsets, case.rows, case.D, device=DEV)


def _same_postings(got, case):
    p_off, p_qry = PC.postings_ref(case.offsets, case.rows, case.D)
    assert got.p_off.dtype == torch.int64 and got.p_qry.dtype == torch.int32 and got.p_off.is_cuda, case.name
    assert (got.D, got.nq, got.nnz) == (case.D, case.nq, len(case.rows)), case.name
    assert np.array_equal(got.p_off.cpu().numpy(), p_off), case.name
    assert np.array_equal(got.p_qry.cpu().numpy(), p_qry), case.name


def _run(case, K, queries=None, postings=None):
    import qrlsh
    postings = _build(case) if postings is None else postings
    return qrlsh.exact_neighbours(case.offsets, case.rows, case.D, K, queries=queries, device=DEV, postings=postings)


def _sweep(case, K, queries=None):
    import qrlsh
    return qrlsh.exact_neighbours(case.offsets, case.rows, case.D, K, queries=queries, device=DEV)


def _check(case, K, queries=None, postings=None, sweep=True):
    """the postings route against the restatement and (sweep) against the sweep route, word for word"""
    got = _run(case, K, queries, postings)
    XC.same_lists(got, case.ref(K, queries), "%s K=%d" % (case.name, K))
    if sweep:
        other = _sweep(case, K, queries)
        for k in ("queries", "dst", "inter", "union", "listed", "positives"):
            assert torch.equal(getattr(got, k), getattr(other, k)), (case.name, k)
    return got


# ---- the postings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [XC.sizes_case, lambda: XC.planted_case(31), lambda: XC.planted_case(32),
                                  lambda: XC.planted_case(33), lambda: XC.Case([{0}, set(), {0}], 1, "D=1"),
                                  PC.empty_rows_case, lambda: XC.Case([set(), set(), set()], 7, "nnz=0"),
                                  lambda: XC.Case([], 7, "nq=0"), lambda: XC.Case([], 0, "nq=0 D=0"), PC.every_query_case,
                                  PC.narrow_case],
                         ids=["sizes", "D31", "D32", "D33", "D1", "empty-rows", "nnz0", "nq0", "nq0-D0", "every-query",
                              "four-tiles"])
def test_postings_bytes(make):
    case = make()
    _same_postings(_build(case), case)
    if case.nq:   # device inputs are used where they are
        import qrlsh
        dev = qrlsh.answer_postings(torch.from_numpy(case.offsets).to(DEV), torch.from_numpy(case.rows).to(DEV), case.D,
                                    device=DEV)
        _same_postings(dev, case)


def _broken(case, **kw):
    out = XC.Case.__new__(XC.Case)
    out.__dict__.update(case.__dict__, **kw)
    return out


def test_postings_flags():
    case = XC.planted_case(200)
    for bad in (case.D, -1):
        rows = case.rows.copy()
        rows[case.offsets[40]] = bad
        with pytest.raises(ValueError, match="row id"):
            _build(_broken(case, rows=rows))
    first, last, down = case.offsets.copy(), case.offsets.copy(), case.offsets.copy()
    first[0], last[-1] = 1, last[-1] - 1
    down[10], down[11] = down[11], down[10]
    assert down[10] > down[11]
    for off in (first, last, down):
        with pytest.raises(ValueError, match="not a CSR"):
            _build(_broken(case, offsets=off))
    with pytest.raises(ValueError, match="not a CSR"):
        _build(_broken(case, rows=case.rows[:-1]))
    _same_postings(_build(case), case)                       # and the same inputs unbroken pass


def test_postings_scratch_between_guards(monkeypatch):
    from qrlsh import _lib, ops, postings
    case = PC.every_query_case()
    made = []

    def guarded(nbytes, device):
        n = max(int(nbytes), 16)
        whole = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=device)
        made.append((whole, n))
        return whole[GUARD:GUARD + n]
    monkeypatch.setattr(ops, "_ws", guarded)
    assert postings.ops is ops
    _same_postings(_build(case), case)
    torch.cuda.synchronize()
    assert len(made) == 1 and made[0][1] == _lib.load().qrlsh_answer_postings_scratch_bytes(len(case.rows), case.D)
    w = made[0][0].cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + made[0][1]:] == FILL).all(), "bytes outside the scratch were written"


# ---- the lists: set sizes, list lengths, ties --------------------------------------------------------------------------
def test_every_set_size():
    case = XC.sizes_case()
    got = _check(case, 5)                                # a = 0 and a = D = 200 are among the requests
    assert got.K == 5 and got.dst.is_cuda and got.dst.dtype == torch.int32 and tuple(got.dst.shape) == (case.nq, 5)
    assert got.queries.tolist() == list(range(case.nq))
    _check(case, 64)


@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_list_lengths_and_positives_around_them(K):
    case = XC.positives_case(K)                          # positives = 0, K - 1, K, K + 1 for queries 0 .. 3
    got = _check(case, K, [0, 1, 2, 3])
    assert got.positives.tolist() == [0, K - 1, K, K + 1] and got.listed.tolist() == [0, K - 1, K, K]
    _check(case, K)


def test_duplicates_of_the_chosen_set_beyond_the_list_and_ties():
    case = XC.planted_case(200)
    for K in (1, 2, 4):
        got = _check(case, K, [0, 3, 5])
        assert got.dst[0].tolist() == [1, 2, 3, 4][:K] and got.dst[2].tolist() == [0, 1, 2, 3][:K]
    _check(XC.tie_case(), 10)


@pytest.mark.parametrize("nq", [1, 2])
def test_the_smallest_query_counts(nq):
    got = _check(XC.Case([{0, 3}, {3, 4}][:nq], 5, "nq=%d" % nq), 4)
    assert got.positives.tolist() == [nq - 1] * nq


def test_a_row_held_by_every_query_and_a_request_of_more_lists_than_stay_in_lds():
    case = PC.every_query_case()
    _check(case, 7)
    long = PC.long_request_case()
    assert long.offsets[1] == long.D > PC.LIST_CURSORS
    _check(long, 9, long.requests)
    _check(long, 3)


# ---- the passes: around C, the halving, the bound, the queue -----------------------------------------------------------
@pytest.fixture(scope="module")
def pass_entries():
    from qrlsh import _lib
    lib = _lib.load()
    C = int(lib.qrlsh_exact_postings_pass_entries())
    assert C == PC.PASS_ENTRIES
    # the cases are built around these two as well: a changed constant fails here instead of hollowing the cases out
    assert int(lib.qrlsh_exact_postings_queue()) == PC.QUEUE
    assert int(lib.qrlsh_exact_postings_list_cursors()) == PC.LIST_CURSORS
    assert int(lib.qrlsh_exact_postings_threads()) == PC.THREADS
    return C


@pytest.mark.parametrize("delta", [-2, -1, 0, 1])
def test_one_list_on_both_sides_of_a_pass(pass_entries, delta):
    """the request's one list holds C - 1, C, C + 1 and C + 2 entries (C - 2 .. C + 1 others and itself): one pass, then
    two; every candidate has multiplicity a = 1"""
    case = PC.single_row_case(pass_entries + delta, C=pass_entries)
    got = _check(case, 10, case.requests)
    assert got.positives[0].item() == pass_entries + delta and (got.inter[0] == 1).all()


def test_a_narrow_range_overflows_the_even_cut_and_is_halved(pass_entries):
    case = PC.narrow_case(pass_entries)
    got = _check(case, 12, case.requests)
    assert got.positives.tolist()[3] == 0 and got.positives[0].item() > pass_entries // 2


def test_nothing_pruned_and_more_survivors_than_the_queue(pass_entries):
    case = PC.unpruned_case()
    _check(case, 10, case.requests)
    many = PC.survivors_case(C=pass_entries)
    got = _check(many, 10, many.requests)
    assert got.dst[0].min().item() > PC.QUEUE            # the kept entries all came in a late round of the walk
    _check(many, 64, many.requests, sweep=False)


# ---- more than one window beside more than 512 lists, single-id passes, probe chains, lanes, late windows ---------------
def test_long_requests_over_several_halved_windows(pass_entries):
    """a = 511 / 512 / 513 / 600 side by side, 3 - 4 non-empty passes each, every one with lo > 0 and found by halving
    (PC.long_windows_case asserts it): the per-window bounds of the requests whose cursors do not stay in LDS"""
    case = PC.long_windows_case(C=pass_entries)
    got = _check(case, 64, case.requests)
    assert got.positives.tolist()[:4] == [63] * 4 and got.positives[5].item() == 0
    _check(case, 1, case.requests)
    _check(case, 9)                                       # every query, the 4032 empty ones among them


def test_passes_of_a_single_id_with_more_than_C_entries(pass_entries):
    """request 0 reads C + 8 lists; ids 0 (itself: the table stays empty), 17, 18 and 19 are passes of one id holding
    C + 8, C + 8, C + 8 and C + 1 entries (PC.hot_id_case asserts it): the hi - lo <= 1 arm of the pass rule"""
    case = PC.hot_id_case(C=pass_entries)
    got = _check(case, 64, case.requests)
    assert got.inter[0, :3].tolist() == [case.D, case.D, pass_entries + 1] and got.dst[0, :3].tolist() == [17, 18, 19]
    _check(case, 1, case.requests)
    _check(case, 3)


def test_probe_chains_that_wrap_with_different_multiplicities(pass_entries):
    """767 keys whose home slots are the last 32 and the first 64 of the table: chains run past slot 16383 into a crowded
    slot 0 .. 63; colliding keys count 1, 2 or 3 (PC.probe_chain_case asserts it)"""
    case = PC.probe_chain_case(C=pass_entries)
    got = _check(case, 64, case.requests)
    assert got.positives[0].item() == 767 and got.positives[3].item() == 0
    _check(case, 1, case.requests)
    _check(case, 7, case.requests)


def test_every_lane_count_of_the_fill():
    """a = 1 .. 512: L = 1024 .. 2 lanes per list, each request with lists both longer and shorter than its L
    (PC.lanes_case asserts it)"""
    case = PC.lanes_case()
    _check(case, 10, case.requests)
    _check(case, 64, case.requests[::-1])


def test_a_threshold_of_the_first_window_prunes_the_later_ones(pass_entries):
    """later windows hold candidates whose bound is below the K-th entry, whose bound EQUALS it and whose J equals it
    exactly (higher ids: they lose the tie); in request nq - 2 the equal class lies below the kept ids and wins
    (PC.late_windows_case asserts all of it with fractions)"""
    case = PC.late_windows_case(C=pass_entries)
    got = _check(case, 8, case.requests)
    assert got.dst[0].tolist() == list(range(1, 9)) and got.positives[0].item() > 2 * pass_entries
    _check(case, 9, case.requests)                        # one place more: the lowest id of the tied class takes it
    _check(case, 1, case.requests)


@pytest.fixture(scope="module")
def random_grid():
    return {(c.nq, c.D): c for c in PC.random_cases(0)}


@pytest.mark.parametrize("nq,D", PC.RANDOM_GRID)
def test_seeded_random_sets(random_grid, nq, D):
    case = random_grid[nq, D]
    for K in PC.RANDOM_KS:
        _check(case, K, case.requests)


def test_every_path_in_one_launch(pass_entries):
    """a = 0, a = 1, a = 513 over halved windows, the hot-id request with its single-id passes, short requests and
    repeats, unsorted, in one call (PC.mixed_case asserts the plans of the concatenated case)"""
    case = PC.mixed_case(C=pass_entries)
    for K in (5, 64):
        want = case.ref(K, case.requests)
        got = _check(case, K, case.requests)
        assert got.queries.tolist() == case.requests
        dev = _run(case, K, torch.tensor(case.requests, dtype=torch.int32, device=DEV))
        XC.same_lists(dev, want)


def test_flags_raised_from_a_long_request():
    import qrlsh
    case = PC.long_windows_case()
    postings = _build(case)
    s = case.requests[0]                                  # holds all 600 rows
    at = PC.LIST_CURSORS + 38
    assert case.offsets[s + 1] - case.offsets[s] > at >= PC.LIST_CURSORS
    # bit 3: a row id outside [0, D) at a position past the lists whose cursors stay in LDS, postings of the unbroken sets
    for bad in (case.D, -1):
        rows = case.rows.copy()
        rows[case.offsets[s] + at] = bad
        with pytest.raises(ValueError, match="row id"):
            _run(_broken(case, rows=rows), 5, [0, s], postings)
    # bit 4: an entry = nq at the end of a list that only the long request reads
    others = set(np.concatenate([case.rows[case.offsets[q]:case.offsets[q + 1]] for q in case.requests[1:]]).tolist())
    row = max(r for r in range(PC.LIST_CURSORS, case.D) if r not in others)
    p_off = postings.p_off.cpu().numpy()
    end = int(p_off[row + 1]) - 1
    assert end > int(p_off[row]) and int(postings.p_qry[end].item()) > s     # not the request's own entry
    planted = qrlsh.AnswerPostings(postings.p_off, postings.p_qry.clone(), postings.D, postings.nq, postings.nnz)
    planted.p_qry[end] = case.nq
    with pytest.raises(ValueError, match="do not belong"):
        _run(case, 5, [s], planted)
    XC.same_lists(_run(case, 5, case.requests[1:], planted), case.ref(5, case.requests[1:]))   # nobody else reads it
    XC.same_lists(_run(case, 5, [s], postings), case.ref(5, [s]))


# ---- requests ----------------------------------------------------------------------------------------------------------
def test_repeated_and_unsorted_requests_from_host_and_device():
    case = XC.planted_case(200)
    postings = _build(case)
    chosen = [case.nq - 1, 0, 0, 7, 30, 8, 0, 9]
    want = case.ref(6, chosen)
    host = _run(case, 6, chosen, postings)
    XC.same_lists(host, want)
    assert host.queries.tolist() == chosen
    for dtype in (torch.int64, torch.int32):
        dev = _run(case, 6, torch.tensor(chosen, dtype=dtype, device=DEV), postings)
        XC.same_lists(dev, want)
    got = _run(case, 3, [], postings)                    # m = 0
    assert tuple(got.dst.shape) == (0, 3) and tuple(got.positives.shape) == (0,)
    import qrlsh
    e = np.zeros(0, dtype=np.int32)
    none = qrlsh.answer_postings(np.zeros(1, dtype=np.int64), e, 10, device=DEV)
    got = qrlsh.exact_neighbours(np.zeros(1, dtype=np.int64), e, 10, 3, device=DEV, postings=none)
    assert tuple(got.dst.shape) == (0, 3)


def test_flags_of_the_request_kernel():
    case = XC.planted_case(200)
    postings = _build(case)
    K = 3
    # bit 2: a device id outside [0, nq)
    for bad in (-1, case.nq):
        with pytest.raises(ValueError, match="chosen query is outside"):
            _run(case, K, torch.tensor([0, bad], device=DEV), postings)
    # bit 3: a row id of a chosen query outside [0, D), with the postings of the unbroken sets
    for bad in (-1, case.D):
        rows = case.rows.copy()
        rows[case.offsets[0]] = bad
        with pytest.raises(ValueError, match="row id"):
            _run(_broken(case, rows=rows), K, [0], postings)
    # bit 4: the postings of another CSR of the same shape whose p_off[D] differs
    import qrlsh
    other = qrlsh.AnswerPostings(postings.p_off.clone(), postings.p_qry, postings.D, postings.nq, postings.nnz)
    other.p_off[-1] -= 1
    with pytest.raises(ValueError, match="do not belong"):
        _run(case, K, [0], other)
    # bit 4: an entry = nq at the end of a list the request reads
    row = int(case.rows[case.offsets[0]])
    planted = qrlsh.AnswerPostings(postings.p_off, postings.p_qry.clone(), postings.D, postings.nq, postings.nnz)
    planted.p_qry[int(postings.p_off[row + 1].item()) - 1] = case.nq
    with pytest.raises(ValueError, match="do not belong"):
        _run(case, K, [0], planted)
    XC.same_lists(_run(case, K, [0], postings), case.ref(K, [0]))       # the originals were not touched


def test_request_blocks_under_a_small_budget(monkeypatch):
    from qrlsh import postings as po
    case = XC.planted_case(200)
    K = 4
    monkeypatch.setattr(po, "WORKSPACE_BUDGET", 16 * (3 * K + 2) * 4)    # sixteen requests a call
    calls = []
    lib = po._lib.load()
    real = lib.qrlsh_exact_neighbours_postings
    monkeypatch.setattr(lib, "qrlsh_exact_neighbours_postings", lambda *a: calls.append(a[7]) or real(*a))
    XC.same_lists(_run(case, K), case.ref(K))
    assert calls == [15] * (case.nq // 15) and case.nq % 15 == 0       # 60 -> 30 -> 15 fits
    chosen = list(range(case.nq - 1, -1, -1)) + [0, 0]
    calls.clear()
    XC.same_lists(_run(case, K, chosen), case.ref(K, chosen))
    assert calls == [16, 16, 16, 14]                                     # 62 -> 31 -> 16 fits; a short last block


# ---- the library itself: every output word written, nothing outside ----------------------------------------------------
def test_every_output_word_is_written_between_guards():
    from qrlsh import _lib
    from qrlsh.ops import _ptr, _stream
    lib = _lib.load()
    case = XC.planted_case(200)
    postings = _build(case)
    chosen, K = [0, 7, 8, 30, case.nq], 5                               # the last one is outside: all padding
    off, rows = torch.from_numpy(case.offsets).to(DEV), torch.from_numpy(case.rows).to(DEV)
    q = torch.tensor(chosen, dtype=torch.int32, device=DEV)
    m = len(chosen)
    words = [m * K, m * K, m * K, m * 2]
    whole = [torch.full((w * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV) for w in words]
    outs = [t[GUARD:GUARD + w * 4].view(torch.int32) for t, w in zip(whole, words)]
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    status = lib.qrlsh_exact_neighbours_postings(_ptr(off), _ptr(rows), case.nq, case.D, _ptr(postings.p_off),
                                                 _ptr(postings.p_qry), _ptr(q), m, K, *(_ptr(t) for t in outs), _ptr(flag),
                                                 None, 0, _stream())
    torch.cuda.synchronize()
    assert status == _lib.QRLSH_OK and int(flag.item()) == 4
    for t, w in zip(whole, words):
        h = t.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + w * 4:] == FILL).all(), "bytes outside an output were written"
    dst, inter, union = (t.cpu().numpy().reshape(m, K) for t in outs[:3])
    counts = outs[3].cpu().numpy().reshape(m, 2)
    want = case.ref(K, chosen[:-1])
    XC.same_lists(dict(dst=dst[:-1], inter=inter[:-1], union=union[:-1], counts=counts[:-1]), want)
    assert (dst[-1] == -1).all() and not inter[-1].any() and not union[-1].any() and not counts[-1].any()


# ---- the existing kernel as a second oracle ----------------------------------------------------------------------------
def test_list_fidelity_finds_the_lists_exact():
    import qrlsh
    case = XC.no_tail_case()
    K = 8
    got = _check(case, K)
    src, dst, milli = got.coo()
    lf = qrlsh.list_fidelity(case.offsets, case.rows, case.D, src, dst, milli, case.nq, K, device=DEV)
    w = dict(zip(FC.WORDS, lf.per_request.T))
    assert np.array_equal(w["listed"], got.listed.cpu().numpy()) and np.array_equal(w["hits"], w["listed"])
    assert not w["inversions"].any() and int(w["listed"].sum()) > 0


# ---- Recommender -------------------------------------------------------------------------------------------------------
def _same_as_the_sweep(rec, K, what):
    a, b = rec.exact_query_lists(K=K), rec.exact_query_lists(K=K, postings=True)
    for k in ("queries", "dst", "inter", "union", "listed", "positives"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
    assert int(b.listed.sum().item()) > 0, what
    some = [rec.queriesIDs.size - 1, 0, 3]
    held = rec.answer_postings()
    c = rec.exact_query_lists(K=2, positions=some, postings=held)
    d = rec.exact_query_lists(K=2, positions=some)
    assert torch.equal(c.dst, d.dst) and torch.equal(c.union, d.union), what
    return held


def test_recommender_postings_follow_the_live_operations():
    from test_gpu_recommend import _recommender_on
    rec, g = _recommender_on("cfg1")
    rec.compute_querySimilarities()
    held = _same_as_the_sweep(rec, 3, "run")
    assert repr(held).startswith("AnswerPostings(") and held.nq == rec.queriesIDs.size
    own = rec.exact_query_lists(postings=True)
    assert own.K == rec.last_result.K
    q = np.asarray(rec.queries, dtype=object)
    rec.add_queries(q[:3], update_lists=True)
    with pytest.raises(ValueError, match="built from"):
        rec.exact_query_lists(K=3, postings=held)          # stale: three queries more
    _same_as_the_sweep(rec, 3, "queries added")
    rec.remove_rows([0, 5, 17, rec.dataset.shape[0] - 1], update_lists=True)
    held = _same_as_the_sweep(rec, 3, "rows removed")
    rec.remove_queries([1, rec.queriesIDs.size - 1], update_lists=True)
    with pytest.raises(ValueError, match="built from"):
        rec.exact_query_lists(K=3, postings=held)          # stale: two queries fewer
    held = _same_as_the_sweep(rec, 3, "queries removed")
    from qrlsh import ops
    off, _, _ = rec._answer_set_inputs()
    sizes = np.diff(ops.to_host(off))
    p, t = next((p, t) for p in range(sizes.size) for t in range(sizes.size) if sizes[p] != sizes[t] and sizes[t] > 0)
    rec.replace_queries([p], np.asarray(rec.queries, dtype=object)[t:t + 1], update_lists=True)
    assert int(ops.to_host(rec._answer_set_inputs()[0])[-1]) != held.nnz and held.nq == rec.queriesIDs.size
    with pytest.raises(ValueError, match="built from"):
        rec.exact_query_lists(K=3, postings=held)          # stale: as many queries, another entry count
    _same_as_the_sweep(rec, 3, "a query replaced by one of another size")
