"""The exact answer-set overlap of the neighbour lists on the device (qrlsh_edge_overlaps, qrlsh_list_fidelity,
qrlsh.edge_overlaps / list_fidelity, Recommender.list_fidelity / edge_overlaps): every output word is compared for
equality with the restatement of tests/fidelity_cases.py (Python sets and fractions).  No tolerances."""
import numpy as np
import pytest
import torch

import fidelity_cases as FC

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(case, queries=None, K=None, slices=0):
    import qrlsh
    return qrlsh.list_fidelity(case.offsets, case.rows, case.D, case.src, case.dst, case.val, case.nq,
                               case.K if K is None else K, queries=queries, slices=slices, device=DEV)


def _group(D):
    from qrlsh import fidelity
    return fidelity.group_size(D)


# ---- edge_overlaps -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overlap():
    return FC.overlap_case()


def test_edge_overlaps_every_size_against_every_size(overlap):
    import qrlsh
    offsets, rows, src, dst, want = overlap
    got = qrlsh.edge_overlaps(offsets, rows, src, dst, device=DEV)
    assert got.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    # device inputs are used where they are
    dev = [torch.from_numpy(a).to(DEV) for a in (offsets, rows, src, dst)]
    assert np.array_equal(qrlsh.edge_overlaps(*dev, device=DEV).cpu().numpy(), want)


@pytest.mark.parametrize("n", [0, 1, FC.WORKGROUP_EDGES - 1, FC.WORKGROUP_EDGES, FC.WORKGROUP_EDGES + 1])
def test_edge_overlaps_edge_counts(overlap, n):
    import qrlsh
    offsets, rows, src, dst, want = overlap
    pick = np.arange(len(src))[::-7][:n]      # not the first n: large sets among them
    got = qrlsh.edge_overlaps(offsets, rows, src[pick], dst[pick], device=DEV)
    assert tuple(got.shape) == (n,) and np.array_equal(got.cpu().numpy(), want[pick])


@pytest.mark.parametrize("bad", [-1, None])
def test_edge_overlaps_flags_an_end_outside(overlap, bad):
    import qrlsh
    from qrlsh import _lib
    from qrlsh.ops import _ptr, _stream
    offsets, rows, src, dst, want = overlap
    nq = len(offsets) - 1
    bad = nq if bad is None else bad
    for which in (0, 1):
        ends = [src[:40].copy(), dst[:40].copy()]
        ends[which][17] = bad
        with pytest.raises(ValueError, match="outside"):
            qrlsh.edge_overlaps(offsets, rows, ends[0], ends[1], device=DEV)
        # the library: bit 0, that edge 0, every other edge served
        dev = [torch.from_numpy(a).to(DEV) for a in (offsets, rows, ends[0], ends[1])]
        out = torch.full((40,), -7, dtype=torch.int32, device=DEV)
        flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
        _lib.check(_lib.load().qrlsh_edge_overlaps(_ptr(dev[0]), _ptr(dev[1]), nq, _ptr(dev[2]), _ptr(dev[3]), 40, _ptr(out),
                                                   _ptr(flag), _stream()))
        w = want[:40].copy()
        w[17] = 0
        assert int(flag.item()) == 1 and np.array_equal(out.cpu().numpy(), w)


# ---- list_fidelity: real lists -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lsh():
    """(case, its restatement over all queries at its own K), computed once"""
    out = []
    for shape in FC.LSH_SHAPES:
        case = FC.lsh_case(**shape)
        ref = case.ref()
        FC.assert_lsh_case_is_telling(case, ref)
        out.append((case, ref))
    return out


@pytest.mark.parametrize("which", [0, 1])
def test_real_lists_all_queries(lsh, which):
    case, ref = lsh[which]
    got = _run(case)
    FC.same_result(got, ref)
    assert got.K == case.K and np.array_equal(got.queries, np.arange(case.nq))
    t = ref["totals"]
    assert got.recall == t[3] / t[5] and got.sure_recall == t[4] / t[5] and got.disjoint_share == t[6] / t[0]


@pytest.mark.parametrize("slices", [1, 2, 7, 0])
def test_slices_give_the_same_words(lsh, slices):
    case, ref = lsh[0]
    assert case.nq % 2 and case.nq % 7                   # nq is no multiple of the slice
    FC.same_result(_run(case, slices=slices), ref)


@pytest.mark.parametrize("K", [1, 3, 5, 64])
def test_judged_length_below_and_above_the_stored_one(lsh, K):
    case, _ = lsh[0]
    assert 1 < case.K < 5
    chosen = np.arange(0, case.nq, 3)
    FC.same_result(_run(case, chosen, K=K), case.ref(chosen, K))


# ---- list_fidelity: planted lists, bitmap and group edges --------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    case = FC.planted_case(200)
    ref = case.ref()
    FC.assert_planted_case_is_telling(case, ref)
    return case, ref


def test_planted_lists_all_queries(planted):
    case, ref = planted
    FC.same_result(_run(case), ref)
    FC.same_result(_run(case, K=64), case.ref(K=64))     # row 10 holds exactly 64 entries


@pytest.mark.parametrize("D", [31, 32, 33])
def test_bitmap_word_edges(D):
    case = FC.planted_case(D)
    FC.same_result(_run(case), case.ref())


def _edge_requests(case, G):
    """m = 1, G and G + 1 requests: the first and the last query among them, a repeat once they run out"""
    ids = [0, case.nq - 1, 7, 8] + list(range(1, case.nq - 1))
    ids = (ids * (1 + (G + 1) // len(ids)))[:G + 1]
    return [ids[:1], ids[:G], ids]


def test_group_steps_are_where_the_rule_says():
    steps = FC.group_steps(_group)
    assert [_group(d) for d in steps] == [32, 16, 8, 4, 2] and all(_group(d + 1) == _group(d) // 2 for d in steps)


@pytest.mark.parametrize("step", range(5))
@pytest.mark.parametrize("side", [0, 1])
def test_both_sides_of_every_group_step(step, side):
    D = FC.group_steps(_group)[step] + side
    G = _group(D)
    case = FC.planted_case(D, nq=200, seed=20 + step)
    for chosen in _edge_requests(case, G):
        FC.same_result(_run(case, chosen), case.ref(chosen))


def test_the_largest_table():
    D = 1 << 20
    assert _group(D) == 1
    case = FC.planted_case(D, nq=200, seed=40)
    for chosen in ([case.nq - 1], [0, 8]):               # m = 1 = G, m = G + 1; 8 holds all 2^20 rows
        FC.same_result(_run(case, chosen), case.ref(chosen))


def test_group_sizes_at_the_smallest_table():
    case = FC.planted_case(33, nq=70)
    G = _group(33)
    assert G == 32 and case.nq > 2 * G
    for chosen in _edge_requests(case, G):
        FC.same_result(_run(case, chosen), case.ref(chosen))
    dev = torch.tensor([case.nq - 1, 0, 0], dtype=torch.int64, device=DEV)      # device ids, a repeat
    got = _run(case, dev)
    FC.same_result(got, case.ref([case.nq - 1, 0, 0]))
    assert got.queries.tolist() == [case.nq - 1, 0, 0]


# ---- list_fidelity: call handling --------------------------------------------------------------------------------------
def _library_call(case, queries, K, totals, flag, fill=-7):
    """qrlsh_list_fidelity itself over device copies -> (inter, union, better, equal [m, 64], words [m, 8]) host arrays"""
    from qrlsh import _lib, predict
    from qrlsh.ops import _ptr, _stream
    off = torch.from_numpy(case.offsets).to(DEV)
    rows = torch.from_numpy(case.rows).to(DEV)
    q_off, q_idx, _ = predict.lists_csr([torch.from_numpy(a) for a in (case.src, case.dst, case.val)], case.nq, DEV)
    q = torch.tensor(queries, dtype=torch.int32, device=DEV)
    m = len(queries)
    ent = [torch.full((m, FC.MAX_K), fill, dtype=torch.int32, device=DEV) for _ in range(4)]
    words = torch.full((m, 8), fill, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().qrlsh_list_fidelity(_ptr(off), _ptr(rows), case.nq, case.D, _ptr(q_off), _ptr(q_idx), _ptr(q), m,
                                               K, 0, *(_ptr(t) for t in ent), _ptr(words), _ptr(totals), _ptr(flag),
                                               _stream()))
    return [t.cpu().numpy() for t in ent] + [words.cpu().numpy()]


def test_totals_add_up_across_calls(planted):
    case, _ = planted
    first, second = [0, 5, 9, 10], [7, 8, 0, 30, 31]
    totals = torch.zeros((8,), dtype=torch.int64, device=DEV)
    flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
    a = _library_call(case, first, case.K, totals, flag)
    ra = case.ref(first)
    assert np.array_equal(totals.cpu().numpy(), ra["totals"])
    b = _library_call(case, second, case.K, totals, flag)
    rb = case.ref(second)
    assert np.array_equal(totals.cpu().numpy(), ra["totals"] + rb["totals"]) and int(flag.item()) == 0
    for got, want in ((a, ra), (b, rb)):                 # the outputs are written whole over whatever they held
        FC.same_result(dict(zip(("inter", "union", "better", "equal", "words"), got), totals=want["totals"]), want)


def test_host_layer_runs_request_blocks(planted, monkeypatch):
    from qrlsh import fidelity
    case, ref = planted
    G = _group(case.D)
    monkeypatch.setattr(fidelity, "MAX_REQUESTS", G)     # two calls, the second a partial group
    assert G < case.nq < 2 * G
    FC.same_result(_run(case), ref)
    chosen = list(range(case.nq - 1, -1, -1)) + [0, 0]
    FC.same_result(_run(case, chosen), case.ref(chosen))


def test_host_layer_splits_under_its_budget_into_whole_groups(monkeypatch):
    from qrlsh import _lib, fidelity
    case = FC.planted_case(33, nq=70)
    G = _group(33)
    assert case.nq > 2 * G
    whole = _run(case)
    FC.same_result(whole, case.ref())
    lib = _lib.load()
    calls = []
    real = lib.qrlsh_list_fidelity

    def counted(*args):
        calls.append(args[7])
        return real(*args)
    monkeypatch.setattr(lib, "qrlsh_list_fidelity", counted)
    monkeypatch.setattr(fidelity, "WORKSPACE_BUDGET", G * fidelity._REQUEST_BYTES)     # one group per call
    split = _run(case)                                   # every query, unnamed: the blocks are served by made-up ids
    assert calls == [G, G, case.nq - 2 * G]
    FC.same_result(split, case.ref())
    assert np.array_equal(split.queries, whole.queries) and np.array_equal(split.per_request, whole.per_request)
    assert np.array_equal(split.totals, whole.totals)
    assert all(np.array_equal(split.entries[name], whole.entries[name]) for name in whole.entries)


def _with(case, **kw):
    a = dict(offsets=case.offsets, rows=case.rows, D=case.D, src=case.src, dst=case.dst, val=case.val, K=case.K, name="bad")
    a.update(kw)
    return FC.FidelityCase(**a)


def test_each_flag_bit(planted):
    case, ref = planted
    totals = torch.zeros((8,), dtype=torch.int64, device=DEV)

    def flagged(bad_case, queries, match):
        with pytest.raises(ValueError, match=match):
            _run(bad_case, queries)
        flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
        out = _library_call(bad_case, queries, bad_case.K, totals, flag)
        return int(flag.item()), out
    # bit 0: a chosen query's row is longer than 64 -- not walked, its words 0; the request beside it is served
    long_row = 11
    keep = case.src != long_row
    extra = np.arange(65, dtype=np.int32) % case.nq
    order = np.argsort(np.concatenate((case.src[keep], np.full(65, long_row))), kind="stable")
    src = np.concatenate((case.src[keep], np.full(65, long_row, dtype=np.int32)))[order]
    dst = np.concatenate((case.dst[keep], extra))[order]
    bit, out = flagged(_with(case, src=src, dst=dst, val=np.zeros(len(src), dtype=np.int32)), [long_row, 0], "longer than 64")
    assert bit == 1 and not out[4][0].any() and not any(o[0].any() for o in out[:4])
    assert np.array_equal(out[4][1], ref["words"][0])
    assert qrlsh_ok(_with(case, src=src, dst=dst, val=np.zeros(len(src), dtype=np.int32)), [0, 5], case)   # not chosen: no flag
    # bit 1: a neighbour index outside [0, nq) among the judged entries -- nothing is gathered for it
    for bad in (-1, case.nq):
        dst = case.dst.copy()
        at = int(np.nonzero(case.src == 0)[0][1])
        dst[at] = bad
        bit, out = flagged(_with(case, dst=dst), [0], "neighbour index")
        assert bit == 2 and out[0][0, 1] == 0 and out[1][0, 1] == 0
    # bit 2: a chosen query outside [0, nq) (device ids: host ids are refused before the upload)
    for bad in (-1, case.nq):
        with pytest.raises(ValueError, match="outside"):
            _run(case, [0, bad])
        with pytest.raises(ValueError, match="chosen query is outside"):
            _run(case, torch.tensor([0, bad], device=DEV))
        flag = torch.zeros((1,), dtype=torch.int32, device=DEV)
        out = _library_call(case, [bad, 0], case.K, totals, flag)
        assert int(flag.item()) == 4 and not out[4][0].any() and np.array_equal(out[4][1], ref["words"][0])
    # bit 3: an answer-set row id outside [0, D) -- in a chosen query's set, and in a swept one
    for q in (0, 40):
        for bad in (-1, case.D):
            rows = case.rows.copy()
            rows[case.offsets[q]] = bad
            bit, _ = flagged(_with(case, rows=rows), [0], "row id")
            assert bit == 8


def qrlsh_ok(bad_case, queries, case):
    FC.same_result(_run(bad_case, queries), case.ref(queries))
    return True


def test_no_queries_and_no_requests():
    import qrlsh
    e = np.zeros(0, dtype=np.int32)
    got = qrlsh.list_fidelity(np.zeros(1, dtype=np.int64), e, 10, e, e, e, 0, 3, device=DEV)
    assert got.per_request.shape == (0, 8) and not got.totals.any() and np.isnan(got.recall)
    case = FC.planted_case(33)
    got = _run(case, [])
    assert got.per_request.shape == (0, 8) and got.entries["inter"].shape == (0, 64) and not got.totals.any()


# ---- Recommender -------------------------------------------------------------------------------------------------------
def _assert_recommender_current(rec, what):
    off, rows = rec.answer_sets()
    sims = rec.current_query_similarities()
    nq = rec.queriesIDs.size
    src = np.array([q for q in sorted(sims) for _ in sims[q]["indexes"]], dtype=np.int32)
    dst = np.array([d for q in sorted(sims) for d in sims[q]["indexes"]], dtype=np.int32)
    qi = rec._query_index
    K = qi.lists_K if qi is not None else rec.last_result.K
    got = rec.list_fidelity(positions=np.arange(nq))
    assert got.K == K, what
    want = FC.fidelity_ref(off, rows, src, dst, nq, K)
    FC.same_result(got, want)
    assert want["totals"][3] > 0, what
    s, d, v, inter, sizes = rec.edge_overlaps()
    assert np.array_equal(s.cpu().numpy(), src) and np.array_equal(d.cpu().numpy(), dst)
    assert np.array_equal(inter.cpu().numpy(), FC.overlaps_ref(off, rows, src, dst)), what
    assert np.array_equal(sizes.cpu().numpy(), np.diff(off)), what
    return got


def test_recommender_fidelity_follows_the_live_operations():
    from test_gpu_recommend import _recommender_on
    rec, g = _recommender_on("cfg1")
    with pytest.raises(ValueError, match="no live lists"):
        rec.list_fidelity()
    rec.compute_querySimilarities()
    first = _assert_recommender_current(rec, "run")
    N = rec.queriesIDs.size
    # the seeded sample, a judged length below the lists' own, nothing modified
    held = [t.clone() for t in rec._live_lists()]
    from qrlsh import fidelity
    sub = rec.list_fidelity(sample=16, seed=3, K=2)
    assert sub.queries.tolist() == fidelity.sample_positions(N, 16, 3).tolist() and sub.K == 2
    assert (sub.per_request[:, 0] <= 2).all()
    assert rec.list_fidelity().per_request.shape[0] == min(N, 1024)
    assert all(torch.equal(a, b) for a, b in zip(held, rec._live_lists()))
    q = np.asarray(rec.queries, dtype=object)
    rec.add_queries(q[:3], update_lists=True)
    assert rec.queriesIDs.size == N + 3
    added = _assert_recommender_current(rec, "queries added")
    assert added.per_request.shape[0] == N + 3
    assert added.per_request[N, 1] == added.per_request[0, 1]      # the copy of query 0 has query 0's answer set
    rec.remove_rows([0, 5, 17, rec.dataset.shape[0] - 1], update_lists=True)
    assert rec._live_table is not None
    _assert_recommender_current(rec, "rows removed")
    rec.set_list_lengths(query_K=3)
    cut = _assert_recommender_current(rec, "lists cut")
    assert cut.K == 3 and first.K != 3
    rec.remove_queries([1])                               # the lists are dropped
    with pytest.raises(ValueError, match="no live lists"):
        rec.list_fidelity()
