"""The exact neighbour lists on the device (qrlsh_exact_neighbours, qrlsh.exact_neighbours, ExactLists.coo,
Recommender.exact_query_lists and the `lists` keyword): every output word is compared for equality with the restatement
of tests/exactlists_cases.py (Python sets and fractions), and the existing list_fidelity kernel is run over the result as
a second oracle.  No tolerances."""
import numpy as np
import pytest
import torch

import exactlists_cases as XC
import fidelity_cases as FC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
FILL = 0xA5


def _run(case, K, queries=None, slices=0):
    import qrlsh
    return qrlsh.exact_neighbours(case.offsets, case.rows, case.D, K, queries=queries, slices=slices, device=DEV)


def _group(D):
    from qrlsh import fidelity
    return fidelity.group_size(D)


def _check(case, K, queries=None, slices=0):
    got = _run(case, K, queries, slices)
    XC.same_lists(got, case.ref(K, queries), "%s K=%d slices=%d" % (case.name, K, slices))
    return got


# ---- set sizes, table edges, list lengths ------------------------------------------------------------------------------
def test_every_set_size_with_fewer_queries_than_lane_groups():
    case = XC.sizes_case()
    assert case.nq < XC.LANE_GROUPS
    got = _check(case, 5)
    assert got.K == 5 and got.dst.is_cuda and got.dst.dtype == torch.int32 and tuple(got.dst.shape) == (case.nq, 5)
    assert got.queries.tolist() == list(range(case.nq))
    _check(case, 64)
    # device inputs are used where they are
    import qrlsh
    dev = qrlsh.exact_neighbours(torch.from_numpy(case.offsets).to(DEV), torch.from_numpy(case.rows).to(DEV), case.D, 5,
                                 device=DEV)
    XC.same_lists(dev, case.ref(5))


@pytest.mark.parametrize("nq", [1, 2])
def test_the_smallest_query_counts(nq):
    case = XC.Case([{0, 3}, {3, 4}][:nq], 5, "nq=%d" % nq)
    got = _check(case, 4)
    assert got.positives.tolist() == [nq - 1] * nq


@pytest.mark.parametrize("D", [31, 32, 33])
def test_bitmap_word_edges(D):
    _check(XC.planted_case(D), 3)


@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_list_lengths_and_positives_around_them(K):
    case = XC.positives_case(K)                         # positives = 0, K - 1, K, K + 1 for queries 0 .. 3
    got = _check(case, K, [0, 1, 2, 3])
    assert got.positives.tolist() == [0, K - 1, K, K + 1] and got.listed.tolist() == [0, K - 1, K, K]
    _check(case, K)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_more_duplicates_of_the_chosen_set_than_the_list_holds(K):
    case = XC.planted_case(200)
    got = _check(case, K, [0, 3, 5])
    d = got.dst.cpu().numpy()
    assert d[0].tolist() == [1, 2, 3, 4][:K] and d[1].tolist() == [0, 1, 2, 4][:K] and d[2].tolist() == [0, 1, 2, 3][:K]
    assert (got.inter.cpu().numpy() == got.union.cpu().numpy()).all()              # J = 1 throughout


# ---- slices: a tie group across every boundary -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ties():
    case = XC.tie_case()
    return case, case.ref(10)


@pytest.mark.parametrize("slices", [1, 2, 7, 0])
def test_a_tie_group_that_straddles_every_slice_boundary(ties, slices):
    case, ref = ties
    assert case.nq % 2 and case.nq % 7                  # nq is no multiple of the slice
    XC.same_lists(_run(case, 10, slices=slices), ref, "slices=%d" % slices)


def test_more_slices_than_queries():
    case = XC.sizes_case()
    XC.same_lists(_run(case, 5, slices=256), case.ref(5))          # most slices hold no id at all


# ---- the group rule: the LDS layout on both sides of every step -------------------------------------------------------
def _edge_requests(case, G):
    """m = 1, G and G + 1 requests: the first and the last query among them, a repeat once they run out"""
    ids = [0, case.nq - 1, 7, 8] + list(range(1, case.nq - 1))
    ids = (ids * (1 + (G + 1) // len(ids)))[:G + 1]
    return [ids[:1], ids[:G], ids]


@pytest.mark.parametrize("step", range(5))
@pytest.mark.parametrize("side", [0, 1])
def test_both_sides_of_every_group_step(step, side):
    D = FC.group_steps(_group)[step] + side
    G = _group(D)
    case = XC.planted_case(D, nq=200, seed=20 + step)
    for chosen in _edge_requests(case, G):
        _check(case, 3, chosen)


def test_the_largest_table():
    D = 1 << 20
    assert _group(D) == 1
    case = XC.planted_case(D, nq=200, seed=40)
    for chosen in ([case.nq - 1], [0, 8]):               # m = 1 = G, m = G + 1; 8 holds all 2^20 rows
        _check(case, 3, chosen)


def test_group_sizes_at_the_smallest_table():
    case = XC.planted_case(33, nq=70)
    G = _group(33)
    assert G == 32 and case.nq > 2 * G
    for chosen in _edge_requests(case, G):
        _check(case, 3, chosen)


# ---- requests ----------------------------------------------------------------------------------------------------------
def test_repeated_and_unsorted_requests_from_host_and_device():
    case = XC.planted_case(200)
    chosen = [case.nq - 1, 0, 0, 7, 30, 8, 0, 9]
    want = case.ref(6, chosen)
    host = _run(case, 6, chosen)
    XC.same_lists(host, want)
    assert host.queries.tolist() == chosen
    for dtype in (torch.int64, torch.int32):
        dev = _run(case, 6, torch.tensor(chosen, dtype=dtype, device=DEV))
        XC.same_lists(dev, want)
        assert dev.queries.tolist() == chosen
    with pytest.raises(ValueError, match="more than once"):
        host.coo()


def test_no_queries_and_no_requests():
    import qrlsh
    e = np.zeros(0, dtype=np.int32)
    got = qrlsh.exact_neighbours(np.zeros(1, dtype=np.int64), e, 10, 3, device=DEV)
    assert tuple(got.dst.shape) == (0, 3) and got.listed.numel() == 0 and all(t.numel() == 0 for t in got.coo())
    case = XC.planted_case(33)
    got = _run(case, 3, [])
    assert tuple(got.dst.shape) == (0, 3) and tuple(got.positives.shape) == (0,)
    with pytest.raises(ValueError, match="outside"):
        qrlsh.exact_neighbours(np.zeros(1, dtype=np.int64), e, 10, 3, queries=torch.tensor([0], device=DEV), device=DEV)


def test_host_layer_runs_request_blocks(monkeypatch):
    from qrlsh import exactlists
    case = XC.planted_case(200)
    K, G = 4, _group(200)
    want = case.ref(K)
    monkeypatch.setattr(exactlists, "WORKSPACE_BUDGET", G * K * 3 * 4)      # one group per call at one slice
    assert G < case.nq < 2 * G
    calls = []
    lib = exactlists._lib.load()
    real = lib.qrlsh_exact_neighbours
    monkeypatch.setattr(lib, "qrlsh_exact_neighbours", lambda *a: calls.append(a[5]) or real(*a))
    XC.same_lists(_run(case, K), want)
    assert calls == [G, case.nq - G]                                        # the second a partial group
    chosen = list(range(case.nq - 1, -1, -1)) + [0, 0]
    XC.same_lists(_run(case, K, chosen, slices=3), case.ref(K, chosen))


# ---- the library itself ------------------------------------------------------------------------------------------------
def _library_call(case, queries, K, flag, slices=0, fill=-7, scratch_words=None):
    """qrlsh_exact_neighbours over device copies, the outputs and the scratch pre-filled -> (status, dst, inter, union,
    counts) host arrays"""
    from qrlsh import _lib
    from qrlsh.ops import _ptr, _stream
    lib = _lib.load()
    off = torch.from_numpy(case.offsets).to(DEV)
    rows = torch.from_numpy(case.rows).to(DEV)
    q = torch.tensor(queries, dtype=torch.int32, device=DEV)
    m = len(queries)
    out = [torch.full((m, K), fill, dtype=torch.int32, device=DEV) for _ in range(3)]
    counts = torch.full((m, 2), fill, dtype=torch.int32, device=DEV)
    S = lib.qrlsh_exact_neighbours_slices(case.nq, m, case.D, slices)
    words = m * S * K * 3 if scratch_words is None else scratch_words
    scratch = torch.full((max(words, 4),), fill, dtype=torch.int32, device=DEV)
    status = lib.qrlsh_exact_neighbours(_ptr(off), _ptr(rows), case.nq, case.D, _ptr(q), m, K, slices, *(_ptr(t) for t in out),
                                        _ptr(counts), _ptr(flag), _ptr(scratch), words * 4, _stream())
    return [status] + [t.cpu().numpy() for t in out] + [counts.cpu().numpy()]


def test_every_output_word_is_written_and_the_scratch_size_is_the_formula():
    from qrlsh import _lib
    case = XC.planted_case(200)
    chosen, K = [0, 7, 8, 30], 5
    want = case.ref(K, chosen)
    for slices in (0, 3):
        flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
        status, dst, inter, union, counts = _library_call(case, chosen, K, flag, slices)
        assert status == _lib.QRLSH_OK and int(flag.item()) == 0
        XC.same_lists(dict(dst=dst, inter=inter, union=union, counts=counts), want)       # nothing of the -7 is left
    S = _lib.load().qrlsh_exact_neighbours_slices(case.nq, len(chosen), case.D, 3)
    assert S == 3
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    out = _library_call(case, chosen, K, flag, 3, scratch_words=len(chosen) * S * K * 3 - 1)
    assert out[0] == _lib.QRLSH_EWORKSPACE and (out[1] == -7).all() and (out[4] == -7).all()   # refused before any work


def test_each_flag_bit():
    case = XC.planted_case(200)
    K = 3
    ref = case.ref(K, [0])
    # bit 2: a chosen query outside [0, nq) (device ids: host ids are refused before the upload)
    for bad in (-1, case.nq):
        with pytest.raises(ValueError, match="outside"):
            _run(case, K, [0, bad])
        with pytest.raises(ValueError, match="chosen query is outside"):
            _run(case, K, torch.tensor([0, bad], device=DEV))
        flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
        status, dst, inter, union, counts = _library_call(case, [bad, 0], K, flag)
        assert status == 0 and int(flag.item()) == 4
        assert (dst[0] == -1).all() and not inter[0].any() and not union[0].any() and not counts[0].any()
        XC.same_lists(dict(dst=dst[1:], inter=inter[1:], union=union[1:], counts=counts[1:]), ref)   # its neighbour is served
    # bit 3: an answer-set row id outside [0, D) -- in a chosen query's set, and in a swept one
    for q in (0, 40):
        for bad in (-1, case.D):
            rows = case.rows.copy()
            rows[case.offsets[q]] = bad
            broken = XC.Case.__new__(XC.Case)
            broken.__dict__.update(case.__dict__, rows=rows)
            with pytest.raises(ValueError, match="row id"):
                _run(broken, K, [0])
            flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
            assert _library_call(broken, [0], K, flag)[0] == 0 and int(flag.item()) == 8


# ---- the scratch: nothing outside it is written, nothing in it is read before it is written ----------------------------
def test_guards_around_the_scratch_stay_intact(monkeypatch):
    from qrlsh import exactlists, ops
    case = XC.planted_case(200)
    chosen = list(range(case.nq)) + [0, 5]
    plain = [_run(case, 7, chosen, slices=s) for s in (0, 5)]
    made = []

    def guarded(nbytes, device):
        n = max(int(nbytes), 16)
        whole = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=device)
        made.append((whole, n))
        return whole[GUARD:GUARD + n]
    monkeypatch.setattr(ops, "_ws", guarded)
    assert exactlists.ops is ops
    patched = [_run(case, 7, chosen, slices=s) for s in (0, 5)]
    torch.cuda.synchronize()
    assert len(made) == 2 and made[1][1] == len(chosen) * 5 * 7 * 3 * 4      # m S K 3 words
    for whole, n in made:
        w = whole.cpu().numpy()
        assert (w[:GUARD] == FILL).all() and (w[GUARD + n:] == FILL).all(), "bytes outside the scratch were written"
    for a, b in zip(plain, patched):
        for k in ("dst", "inter", "union", "listed", "positives"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    XC.same_lists(patched[1], case.ref(7, chosen))


# ---- the existing kernel as a second oracle ----------------------------------------------------------------------------
def test_list_fidelity_finds_the_exact_lists_exact():
    import qrlsh
    case = XC.no_tail_case()                            # no milli-0 tails: the COO form is the whole lists
    K = 8
    got = _run(case, K)
    src, dst, milli = got.coo()
    want = XC.coo_ref(case.ref(K), range(case.nq))
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((src, dst, milli), want))
    assert int(src.numel()) == int(got.listed.sum().item())
    lf = qrlsh.list_fidelity(case.offsets, case.rows, case.D, src, dst, milli, case.nq, K, device=DEV)
    w = dict(zip(FC.WORDS, lf.per_request.T))
    assert np.array_equal(w["listed"], got.listed.cpu().numpy()) and np.array_equal(w["positives"], got.positives.cpu().numpy())
    assert np.array_equal(w["hits"], w["listed"]) and np.array_equal(w["listed"], w["reachable"])
    assert not w["inversions"].any() and not w["disjoint"].any() and lf.recall == 1.0
    assert (w["listed"] < K).any() and (w["listed"] == K).any()
    e = np.arange(FC.MAX_K)[None, :]
    inside = e < w["listed"][:, None]
    better, equal = lf.entries["better"], lf.entries["equal"]
    assert ((better <= e) & (e <= better + equal))[inside].all()          # entry e has e entries before it, ties aside
    assert np.array_equal(lf.entries["inter"][:, :K], got.inter.cpu().numpy())
    assert np.array_equal(lf.entries["union"][:, :K], got.union.cpu().numpy())


def test_coo_truncation_on_the_device():
    case = XC.tail_case()
    got = _run(case, 8)
    want = XC.coo_ref(case.ref(8), range(case.nq))
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got.coo(), want))
    assert int(got.listed.sum().item()) > len(want[0])                     # something was cut off


# ---- Recommender -------------------------------------------------------------------------------------------------------
def _assert_exact_lists_current(rec, K, what):
    off, rows = rec.answer_sets()
    nq = rec.queriesIDs.size
    want = XC.exact_ref(np.asarray(off, dtype=np.int64), np.asarray(rows), K)
    got = rec.exact_query_lists(K=K)
    XC.same_lists(got, want, what)
    assert got.queries.tolist() == list(range(nq)) and int(got.listed.sum().item()) > 0, what
    some = [nq - 1, 0, 3]
    XC.same_lists(rec.exact_query_lists(K=2, positions=some),
                  XC.exact_ref(np.asarray(off, dtype=np.int64), np.asarray(rows), 2, some), what)
    return got


def test_recommender_exact_lists_follow_the_live_operations():
    import qrlsh
    from qrlsh import users
    from test_gpu_recommend import _recommender_on
    rec, g = _recommender_on("cfg1")
    with pytest.raises(ValueError, match="no live lists"):
        rec.exact_query_lists()                           # K = None is the live lists' own: there are none yet
    before_run = rec.exact_query_lists(K=3)               # a given K needs no lists: the answer sets are enough
    rec.compute_querySimilarities()
    own = rec.exact_query_lists()
    assert own.K == rec.last_result.K
    first = _assert_exact_lists_current(rec, 3, "run")
    assert torch.equal(first.dst, before_run.dst)
    N = rec.queriesIDs.size

    # evaluate with no `lists` is what it was: qrlsh.evaluate over the live lists; with `lists`, over those
    rec.live_user_similarities(labels=users.cluster_labels(rec.ratings))
    ui = rec.user_index
    weights = dict(query_weight=rec.query_weight, user_weight=rec.user_weight, default_mean=rec.default_mean, device=DEV)
    live = rec._live_lists()
    held = [t.clone() for t in live]
    x = own.coo()
    for lists, kw in ((live, {}), (x, dict(lists=x))):
        want = qrlsh.evaluate(ui.ratings, lists[0], lists[1], lists[2], ui.as_user_sims(), fraction=1.0, seed=0,
                              sum_order=rec.sum_order, **weights)
        got = rec.evaluate(**kw)
        assert np.array_equal(got.totals, want.totals), sorted(kw)
        assert np.array_equal(XC._host(got.per_user), XC._host(want.per_user)), sorted(kw)
    assert not np.array_equal(rec.evaluate().totals, rec.evaluate(lists=x).totals)       # the two lists do differ
    ho = rec.evaluate(holdout=True, fraction=0.2, seed=3, lists=x)
    assert ho.n > 300 and not np.array_equal(ho.totals, rec.evaluate(holdout=True, fraction=0.2, seed=3).totals)
    rk = rec.evaluate_ranking(5, 50, fraction=0.2, seed=3, candidates="heldout", lists=x)
    assert rk.totals is not None
    recs = rec.recommend_users([0, 1, 2], 4, lists=x)
    assert sorted(recs) == [0, 1, 2]
    # list_fidelity from both calls: every entry of the exact lists is a hit and none is out of order (coo() may have cut
    # milli-0 tails, so listed can stay below reachable); the live lists are judged as before the keyword existed
    lf = rec.list_fidelity(positions=np.arange(N), lists=x, K=own.K)
    assert np.array_equal(lf.per_request[:, 3], lf.per_request[:, 0]) and not lf.per_request[:, 7].any()
    assert lf.totals[0] == int(x[0].numel()) > 0
    with pytest.raises(ValueError, match="K is required"):
        rec.list_fidelity(lists=x)
    plain = rec.list_fidelity(positions=np.arange(N))
    want = qrlsh.list_fidelity(*rec._fidelity_inputs()[:3], *live, N, own.K, device=DEV)
    assert plain.K == own.K and np.array_equal(plain.per_request, want.per_request)
    assert all(torch.equal(a, b) for a, b in zip(held, rec._live_lists()))               # nothing was installed

    q = np.asarray(rec.queries, dtype=object)
    rec.add_queries(q[:3], update_lists=True)
    assert rec.queriesIDs.size == N + 3
    added = _assert_exact_lists_current(rec, 3, "queries added")
    assert added.dst[N, 0].item() == 0 and added.inter[N, 0].item() == added.union[N, 0].item()   # the copy of query 0
    rec.remove_rows([0, 5, 17, rec.dataset.shape[0] - 1], update_lists=True)
    assert rec._live_table is not None
    _assert_exact_lists_current(rec, 3, "rows removed")
