"""Serving new queries on the device (csrc/index.hip, qrlsh_predict_columns): exact against the numpy restatement of
tests/query_index_cases.py on golden hold-outs, batch invariance, a 1 M-query self-probe against the hot path's own
lists, both row formats, popular keys and the LDS-image boundaries, colliding caller keys, column prediction on
knife-edge cells, top users, and the Recommender end to end."""
import numpy as np
import pytest
import torch

import query_index_cases as QC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAP = 4096   # IX_CAP in csrc/index.hip


def _index(sig, b, K=16, compact=False, keys=None):
    from qrlsh.index import QueryIndex
    t = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.int32)).cuda()
    if compact:
        t = t.bitwise_and(0xFFFF).to(torch.int16)
    return QueryIndex(t, None, b, keys=keys, K=K)


def _probe(qi, xs, K=None, keys=None):
    t = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(xs), dtype=np.int32)).cuda()
    off, idx, milli, avail = qi.neighbours(t, keys=keys, K=K)
    off, idx, milli, avail = (x.cpu().numpy() for x in (off, idx, milli, avail))
    return [(idx[off[q]:off[q + 1]].astype(np.int64), milli[off[q]:off[q + 1]].astype(np.int64), int(avail[q]))
            for q in range(len(avail))]


def _assert_exact(got, want, what=""):
    assert len(got) == len(want), what
    for q, ((gi, gm, ga), (wi, wm, wa)) in enumerate(zip(got, want)):
        assert ga == wa, (what, q, ga, wa)
        assert np.array_equal(gi, wi) and np.array_equal(gm, wm), (what, q, gi, wi, gm, wm)


@pytest.mark.parametrize("compact", [False, True])
def test_golden_holdouts_exact_and_against_the_reference(compact):
    seen = 0
    for name, g, sig, b, K in QC.golden_sets():
        if compact and (name == "lsh_edge" or sig.max() >= 65535):
            continue
        for h in QC.holdout_queries(sig, g["pairs"]):
            isig, x, remap = QC.holdout(sig, h)
            qi = _index(isig, b, K, compact=compact)
            got = _probe(qi, x, K)
            _assert_exact(got, QC.restate_probe(isig, b, x, K), (name, h))
            assert np.array_equal(np.sort(qi.candidates(torch.from_numpy(x[None].copy()).cuda())[1].cpu().numpy()),
                                  QC.golden_candidates(g["pairs"], h, remap))
            if "qs_q" in g:
                ref = QC.golden_list(g, h, remap)
                if ref is not None:
                    QC.check_list_tie_aware(got[0][0], got[0][1], *ref)
            seen += 1
    assert seen >= 40


def test_batch_invariance_and_empty_sets():
    g = QC.load("full_p180")
    sig = g["sig"].astype(np.int32)
    b, K = int(g["b"]), int(g["K"])
    isig, probes = sig[:1000], sig[1000:].copy()
    probes[5] = -1                                   # an empty answer set
    qi = _index(isig, b, K)
    batch = _probe(qi, probes, K)
    assert len(batch[5][0]) == 0 and batch[5][2] == 0
    _assert_exact(batch, QC.restate_probe(isig, b, probes, K), "batch")
    perm = np.random.default_rng(3).permutation(len(probes))
    rev = _probe(qi, probes[perm], K)
    _assert_exact([rev[int(np.nonzero(perm == q)[0][0])] for q in range(len(probes))], batch, "permuted")
    for q in (0, 5, 77, len(probes) - 1):
        _assert_exact(_probe(qi, probes[q], K), [batch[q]], "alone")
    # an indexed query probed with its own signature finds itself at 1000
    own = _probe(qi, isig[:50], K + 1)
    for q, (ids, mi, _) in enumerate(own):
        if (isig[q] >= 0).all():
            assert q in ids.tolist() and mi[ids.tolist().index(q)] == 1000


def test_self_probe_equals_the_hot_path_on_a_million_queries():
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    nq, D, P, b = 1 << 20, 20000, 128, 32
    offsets, rows = synth.synth_csr(nq, D, seed=5)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=9))
    K = pipeline.max_candidates(nq)
    res = pipeline.query_similarities(offsets, rows, table, b, K)
    qi = QueryIndex.from_result(res, table)
    assert qi.K == K
    pick = torch.from_numpy(np.sort(np.random.default_rng(1).choice(nq, 4096, replace=False))).cuda()
    off, idx, milli, _ = qi.neighbours(res.sig[pick], res.norm2[pick], K=K + 1)
    off, idx, milli = off.cpu().numpy(), idx.cpu().numpy(), milli.cpu().numpy()
    src, dst, val = res.src.cpu().numpy(), res.dst.cpu().numpy(), res.val.cpu().numpy()
    starts = np.searchsorted(src, np.arange(nq + 1))
    for n, q in enumerate(pick.cpu().numpy().tolist()):
        ids, mi = idx[off[n]:off[n + 1]], milli[off[n]:off[n + 1]]
        keep = ids != q
        assert keep.sum() == len(ids) - (starts[q + 1] > starts[q] or len(ids) > 0), q    # finds itself
        ids, mi = ids[keep][:K], mi[keep][:K]
        lo, hi = starts[q], starts[q + 1]
        assert np.array_equal(ids, dst[lo:hi]) and np.array_equal(mi, val[lo:hi]), q


def test_popular_key_and_lds_image_boundaries():
    """one band value shared by many indexed queries: raw lists at CAP - 1, CAP, CAP + 1 and ~30 000 copies; one
    indexed query sharing every band with the probe"""
    rng = np.random.default_rng(7)
    P, b = 64, 16
    n = 45000
    sig = rng.integers(0, 60000, size=(n, P)).astype(np.int32)
    probe = rng.integers(0, 60000, size=(4, P)).astype(np.int32)
    sizes = [CAP - 1, CAP, CAP + 1, 30000]
    base = 0
    for q, s in enumerate(sizes):           # band q of the probe is shared by s indexed queries
        sig[base:base + s, q * 4:(q + 1) * 4] = probe[q, q * 4:(q + 1) * 4]
        base += 0 if q == 3 else s
    sig[n - 1] = probe[3]                      # shares every band with probe 3
    qi = _index(sig, b, 40)
    got = _probe(qi, probe, 40)
    _assert_exact(got, QC.restate_probe(sig, b, probe, 40), "popular")
    assert got[3][2] >= 30000 and got[0][2] >= CAP - 1
    assert got[3][0][0] == n - 1 and got[3][1][0] == 1000
    _assert_exact(_probe(qi, probe, 256), QC.restate_probe(sig, b, probe, 256), "K = 256")


def test_colliding_caller_keys_wide_bands():
    """r = 5 with caller keys that put EVERY indexed query in the probe's bucket: only true candidates come back"""
    g = QC.load("full_p100_r5")
    sig = g["sig"].astype(np.int32)
    b = int(g["b"])
    isig, probes = sig[:600], sig[600:]
    keys = torch.zeros((b, 600), dtype=torch.int64, device="cuda")
    qi = _index(isig, b, 12, keys=keys)
    pk = torch.zeros((b, len(probes)), dtype=torch.int64, device="cuda")
    _assert_exact(_probe(qi, probes, 12, keys=pk), QC.restate_probe(isig, b, probes, 12), "collide")


# ---------------------------------------------------------------------------------------------- column prediction
def _cols(qi_n, ratings, lists, order, weights=(0.6, 0.4, 60.0)):
    from qrlsh.index import QueryIndex
    qi = QueryIndex.__new__(QueryIndex)
    qi.n, qi.sig = qi_n, torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    off = np.concatenate(([0], np.cumsum([len(l["indexes"]) for l in lists]))).astype(np.int64)
    idx = np.concatenate([np.asarray(l["indexes"]) for l in lists]).astype(np.int32)
    mil = np.concatenate([np.rint(np.asarray(l["values"]) * 1000) for l in lists]).astype(np.int32)
    t = [torch.from_numpy(a).cuda() for a in (off, idx, mil)]
    return qi.predict_columns(ratings, *t, sum_order=order, query_weight=weights[0], user_weight=weights[1],
                              default_mean=weights[2]).cpu().numpy()


@pytest.mark.parametrize("order", ["pairwise", "sequential"])
def test_predict_columns_knife_cells_both_orders(order):
    from test_query_index_host import column_case, restate_columns
    import predict_cases as PC
    c, lists, knife = column_case()
    summ = O.np_sum_order if order == "pairwise" else PC.sequential_sum
    got = _cols(c.nq, c.ratings, lists, order)
    want = restate_columns(c.ratings, lists, summ)
    assert np.array_equal(got, want)
    other = restate_columns(c.ratings, lists, PC.sequential_sum if order == "pairwise" else O.np_sum_order)
    assert (other != want).sum() >= 1


def test_predict_columns_shapes_limits_and_weights():
    from test_query_index_host import restate_columns
    rng = np.random.default_rng(4)
    nu, nq = 257, 3000
    ratings = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < 0.3)).astype(np.int32)
    lists = []
    for n in list(range(1, 65)) + [0]:
        ids = rng.choice(nq, size=n, replace=False)
        lists.append({"indexes": ids, "values": np.sort(rng.integers(0, 1001, size=n))[::-1] / 1000.0})
    for order, summ in (("pairwise", O.np_sum_order), ("sequential", None)):
        import predict_cases as PC
        summ = summ or PC.sequential_sum
        assert np.array_equal(_cols(nq, ratings, lists, order), restate_columns(ratings, lists, summ))
    w = (0.3, 0.7, 42.0)
    assert np.array_equal(_cols(nq, ratings, lists, "pairwise", w), restate_columns(ratings, lists, weights=w))
    with pytest.raises(ValueError):
        _cols(nq, ratings, lists + [{"indexes": np.arange(65), "values": np.full(65, 0.5)}], "pairwise")


def test_top_users_equal_the_restatement():
    from qrlsh.index import QueryIndex
    from test_recommend_host import restate
    rng = np.random.default_rng(8)
    cols = (rng.integers(-5, 90, size=(300, 2001)) * (rng.random((300, 2001)) < 0.4)).astype(np.int32)
    for k in (1, 7, 64):
        u, v, a = (x.cpu().numpy() for x in QueryIndex.top_users(torch.from_numpy(cols).cuda(), k))
        wi, wv, wa = restate(np.zeros_like(cols), cols, k)
        assert np.array_equal(u, wi) and np.array_equal(v, wv) and np.array_equal(a, wa)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_new_queries_end_to_end(sub):
    from test_gpu_recommend import _recommender_on
    from test_recommend_host import restate
    from test_query_index_host import restate_columns
    rec, _ = _recommender_on(sub)
    rec.compute_scores()
    res = rec.last_result
    sig = res.sig_int32().cpu().numpy()
    b, K = res.b, res.K
    q = np.asarray(rec.queries, dtype=object)
    ds = rec.dataset
    new = [list(q[0]), list(q[-1])]
    row = [str(ds[f].iloc[3]) for f in rec.datasetFeatures]
    new.append([row[0]] + [""] * (len(row) - 1))
    new.append([row[0], row[1] if len(row) > 1 else ""] + [""] * (len(row) - 2))
    new.append(["no-such-value"] + [""] * (len(row) - 1))
    new = np.array(new, dtype=object)
    sims = rec.similar_queries(new)
    # restatement on the host: the new rows' signatures, through the same table
    from qrlsh import answers
    off, rows = answers.answer_sets(rec._answer_index, answers.encode_queries(rec._answer_index, new))
    xs = O.minhash(off.cpu().numpy(), rows.cpu().numpy(), _perm(rec))
    want = QC.restate_probe(sig, b, xs, K)
    for x, (ids, mi, avail) in enumerate(want):
        if avail == 0:
            assert x not in sims
        else:
            assert np.array_equal(sims[x]["indexes"], ids) and np.array_equal(sims[x]["values"], mi / 1000.0)
    assert want[0][2] > 0 and want[-1][2] == 0
    lists = [{"indexes": ids, "values": mi / 1000.0} for ids, mi, _ in want]
    for order, summ in (("pairwise", O.np_sum_order), ("sequential", None)):
        import predict_cases as PC
        pred = rec.predict_new_queries(new, sum_order=order)
        assert pred.shape == (rec.usersIDs.size, len(new))
        assert np.array_equal(pred.to_numpy().T, restate_columns(rec.ratings, lists, summ or PC.sequential_sum))
    recs = rec.recommend_new_queries(new, 5, sum_order="pairwise")
    cols = restate_columns(rec.ratings, lists)
    wi, wv, wa = restate(np.zeros_like(cols), cols, 5)
    for x in range(len(new)):
        n = min(5, int(wa[x]))
        assert recs[x]["available"] == wa[x]
        assert np.array_equal(recs[x]["users"], wi[x, :n]) and np.array_equal(recs[x]["values"], wv[x, :n])


def _perm(rec):
    """the permutations of the last run, [P][D] (the table is their transpose)"""
    t = rec.last_table
    tab = t.tab.cpu().numpy()
    if tab.dtype == np.int16:
        tab = tab.view(np.uint16).astype(np.int32)
    return np.ascontiguousarray(tab[:, :t.P].T)


def test_lsh_query_matches_the_restatement():
    from lsh import LSH
    g = QC.load("full_p160")
    sig = g["sig"].astype(np.int32)
    b = int(g["b"])
    lsh = LSH(b)
    lsh.compute_buckets_batch(sig[:700])
    got = lsh.query(sig[700:])
    for x, s in enumerate(got):
        assert s == set(QC.restate_candidates(sig[:700], b, sig[700 + x]).tolist())
