"""Appending queries to a built index on the device (qrlsh_index_append, QueryIndex.append / add / reserve,
Recommender.add_queries, LSH.query): every check is exact.  The device is held to the numpy restatement
(tests/index_append_cases.py, tests/query_index_cases.py) and to a fresh build over all rows (QueryIndex over the
concatenation: the build the index had before appends existed), never to itself."""
import ctypes

import numpy as np
import pytest
import torch

import index_append_cases as AC
import query_index_cases as QC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAP = 4096   # IX_CAP in csrc/index.hip


def _rows(sig, compact=False):
    t = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.int32)).cuda()
    if compact:
        t = t.bitwise_and(0xFFFF).to(torch.int16)
    return t


def _index(sig, b, K=16, compact=False, keys=None):
    from qrlsh.index import QueryIndex
    return QueryIndex(_rows(sig, compact), None, b, keys=keys, K=K)


def _same_index(qi, fresh, what=""):
    """byte equality of everything the index holds with a fresh build over all rows"""
    assert qi.n == fresh.n, what
    for name in ("keys", "ids", "dir", "sig", "norm2"):
        a, f = getattr(qi, name), getattr(fresh, name)
        assert a.dtype == f.dtype and tuple(a.shape) == tuple(f.shape), (what, name, a.shape, f.shape)
        assert a.is_contiguous() and torch.equal(a, f), (what, name)


def _same_restated(qi, sig, what=""):
    """the band arrays equal the numpy restatement of the layout over the rows' band keys"""
    sk, ids, dirw = AC.restate_layout(AC.np_band_keys(sig, qi.b))
    assert np.array_equal(qi.keys.cpu().numpy().view(np.uint64), sk), (what, "keys")
    assert np.array_equal(qi.ids.cpu().numpy().view(np.uint32), ids), (what, "ids")
    assert np.array_equal(qi.dir.cpu().numpy().view(np.uint32), dirw), (what, "dir")


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


def _random_rows(rng, n, P, empty=()):
    sig = rng.integers(0, 60000, size=(n, P)).astype(np.int32)
    sig[rng.integers(0, n, size=n // 8)] = sig[rng.integers(0, n, size=n // 8)]     # whole-row duplicates
    cols = rng.integers(0, P // 4, size=n // 4) * 4
    rws = rng.integers(0, n, size=n // 4)
    for c, x in zip(cols, rws):                                                   # shared bands
        sig[x, c:c + 4] = sig[(x * 7 + 1) % n, c:c + 4]
    for e in empty:
        if e < n:
            sig[e] = -1                                                           # an empty answer set: every band empty
    return sig


# ------------------------------------------------------------------------------------------------ 1. byte equality
@pytest.mark.parametrize("compact", [False, True])
def test_appends_equal_the_fresh_build_byte_for_byte(compact):
    rng = np.random.default_rng(21)
    P, b = 32, 8
    batches = [1, 63, 64, 65, 4095, 4096, 4097]
    n0 = 1000                        # 1000 -> 1193 crosses 2^10, -> 13481 crosses 2^12 and 2^13: d changes on the way
    total = n0 + sum(batches)
    sig = _random_rows(rng, total, P, empty=(5, 999, 1000, 1001, 1100, 1200, 1201, 1202, 6000, total - 1))
    qi = _index(sig[:n0], b, compact=compact)
    n = n0
    widths = {qi.dir.numel()}
    for m in batches:
        first, cnt = qi.append(_rows(sig[n:n + m], compact))
        assert (first, cnt) == (n, m)
        n += m
        _same_index(qi, _index(sig[:n], b, compact=compact), (compact, n))
        _same_restated(qi, sig[:n], (compact, n))
        assert qi.dir.numel() == b * ((1 << AC.dir_bits(n)) + 1)
        widths.add(qi.dir.numel())
    assert len(widths) == 4                       # d = 7, 8, 10, 11: the directory width moved with n
    # the grown index serves probes like the fresh one
    probes = sig[rng.integers(0, total, size=64)].copy()
    probes[:, 8:] = rng.integers(0, 60000, size=(64, P - 8))
    _assert_exact(_probe(qi, probes, 16), QC.restate_probe(sig, b, probes, 16), "probes")


@pytest.mark.parametrize("compact", [False, True])
def test_append_from_nothing_nothing_appended_and_more_than_indexed(compact):
    rng = np.random.default_rng(22)
    P, b = 32, 8
    sig = _random_rows(rng, 5300, P, empty=(0, 3, 299, 300, 5299))
    # n = 0, then append
    qi = _index(sig[:0], b, compact=compact)
    assert qi.n == 0
    assert qi.append(_rows(sig[:300], compact)) == (0, 300)
    _same_index(qi, _index(sig[:300], b, compact=compact), "from nothing")
    _same_restated(qi, sig[:300], "from nothing")
    # m = 0: nothing moves
    held = (qi.keys, qi.ids, qi.dir, qi.sig.data_ptr())
    assert qi.append(_rows(sig[:0], compact)) == (300, 0)
    assert qi.keys is held[0] and qi.ids is held[1] and qi.dir is held[2] and qi.sig.data_ptr() == held[3]
    # m > n
    assert qi.append(_rows(sig[300:], compact)) == (300, 5000)
    _same_index(qi, _index(sig, b, compact=compact), "m > n")
    _same_restated(qi, sig, "m > n")
    # every row empty: one key per band, 2 -> 7002 copies
    e = np.full((7002, P), -1, dtype=np.int32)
    qe = _index(e[:2], b, compact=compact)
    qe.append(_rows(e[2:], compact))
    _same_index(qe, _index(e, b, compact=compact), "all empty")
    _same_restated(qe, e, "all empty")
    assert all(a == 0 and len(i) == 0 for i, _, a in _probe(qe, e[:2], 4))


def test_row_formats_capacity_and_the_K_rule():
    from qrlsh.index import QueryIndex
    from qrlsh import pipeline
    rng = np.random.default_rng(23)
    P, b = 32, 8
    sig = _random_rows(rng, 3000, P)
    # int32 rows into a compact index and compact rows into an int32 index: the index's format wins
    for compact in (False, True):
        qi = _index(sig[:1000], b, compact=compact)
        qi.append(_rows(sig[1000:2000], not compact))
        qi.append(_rows(sig[2000:], compact))
        _same_index(qi, _index(sig, b, compact=compact), ("mixed formats", compact))
    # reserve: appends inside the capacity copy m rows and leave the buffers where they are
    t = _rows(sig[:1000])
    keep = t.clone()
    qi = QueryIndex(t, None, b)
    assert qi.K == pipeline.max_candidates(1000)
    qi.reserve(3000)
    base = qi.sig.data_ptr()
    assert base != t.data_ptr()
    qi.append(_rows(sig[1000:1500]))
    qi.append(_rows(sig[1500:3000]))
    assert qi.sig.data_ptr() == base and qi.n == 3000 and qi.sig.is_contiguous() and qi.norm2.is_contiguous()
    assert torch.equal(t, keep)                               # the caller's tensor is never written
    assert qi.K == pipeline.max_candidates(3000)              # a defaulted K follows n
    _same_index(qi, _index(sig, b), "reserved")
    # without reserve the buffers grow geometrically: 1000 -> 2000 -> 4000 rows, not one reallocation per append
    qi = QueryIndex(_rows(sig[:1000]), None, b, K=7)
    ptrs = set()
    for lo in range(1000, 3000, 100):
        qi.append(_rows(sig[lo:lo + 100]))
        ptrs.add(qi.sig.data_ptr())
    assert len(ptrs) == 2 and qi.K == 7                       # a given K stays
    _same_index(qi, _index(sig, b), "geometric")


# ------------------------------------------------------------------------------------------------ 2. golden hold-outs
@pytest.mark.parametrize("compact", [False, True])
def test_golden_holdouts_after_two_appends(compact):
    seen = 0
    for name, g, sig, b, K in QC.golden_sets():
        if compact and (name == "lsh_edge" or sig.max() >= 65535):
            continue
        hs = QC.holdout_queries(sig, g["pairs"])
        keep = np.ones(sig.shape[0], dtype=bool)
        keep[hs] = False
        isig, xs = sig[keep], sig[hs]
        n = isig.shape[0]
        a, c = n // 2, n // 2 + (n - n // 2) // 2
        qi = _index(isig[:a], b, K, compact=compact)
        qi.append(_rows(isig[a:c], compact))
        qi.append(_rows(isig[c:], compact))
        assert qi.n == n
        _assert_exact(_probe(qi, xs, K), QC.restate_probe(isig, b, xs, K), name)
        _same_index(qi, _index(isig, b, K, compact=compact), name)
        seen += 1
    assert seen == (12 if compact else 16)


# ------------------------------------------------------------------------------------------------ 3. a popular key
def test_popular_key_appended_and_lds_image_boundaries():
    """7 000 indexed copies of one band value get 40 000 more in one batch; the same batch brings three other runs from
    100 copies to CAP - 1, CAP and CAP + 1"""
    rng = np.random.default_rng(7)
    P, b = 64, 16
    n, m = 8000, 52000
    sig = rng.integers(0, 60000, size=(n + m, P)).astype(np.int32)
    probe = rng.integers(0, 60000, size=(4, P)).astype(np.int32)
    sig[0:7000, 12:16] = probe[3, 12:16]
    sig[n:n + 40000, 12:16] = probe[3, 12:16]
    lo = n + 40000
    for q, size in enumerate((CAP - 1, CAP, CAP + 1)):
        sig[7000 + 100 * q:7100 + 100 * q, q * 4:q * 4 + 4] = probe[q, q * 4:q * 4 + 4]
        sig[lo:lo + size - 100, q * 4:q * 4 + 4] = probe[q, q * 4:q * 4 + 4]
        lo += size - 100
    assert lo <= n + m
    sig[n + m - 1] = probe[3]                   # an appended query sharing every band with probe 3
    qi = _index(sig[:n], b, 40)
    assert qi.append(_rows(sig[n:])) == (n, m)
    _same_index(qi, _index(sig, b, 40), "popular")
    _same_restated(qi, sig, "popular")
    got = _probe(qi, probe, 40)
    _assert_exact(got, QC.restate_probe(sig, b, probe, 40), "popular probes")
    assert [g[2] for g in got[:3]] == [CAP - 1, CAP, CAP + 1] and got[3][2] == 47001
    assert got[3][0][0] == n + m - 1 and got[3][1][0] == 1000
    _assert_exact(_probe(qi, probe, 256), QC.restate_probe(sig, b, probe, 256), "K = 256")


# ------------------------------------------------------------------------------------------------ 4. caller keys
def test_colliding_caller_keys_on_append():
    """r = 5 with caller keys that put EVERY query, indexed or appended, in one bucket: only true candidates come back"""
    g = QC.load("full_p100_r5")
    sig = g["sig"].astype(np.int32)
    b = int(g["b"])
    isig, probes = sig[:600], sig[600:]
    zeros = lambda k: torch.zeros((b, k), dtype=torch.int64, device="cuda")
    qi = _index(isig[:300], b, 12, keys=zeros(300))
    given = zeros(300)
    qi.append(_rows(isig[300:]), keys=given)
    assert torch.equal(given, zeros(300))                      # the caller's keys are not consumed
    _same_index(qi, _index(isig, b, 12, keys=zeros(600)), "collide")
    assert np.array_equal(qi.ids.cpu().numpy(), np.tile(np.arange(600, dtype=np.int32), (b, 1)))
    _assert_exact(_probe(qi, probes, 12, keys=zeros(len(probes))), QC.restate_probe(isig, b, probes, 12), "collide")


# ------------------------------------------------------------------------------------------------ 5. a million
def test_a_million_indexed_and_16384_appended_in_four_batches():
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    nq, extra, D, P, b = 1 << 20, 16384, 20000, 128, 32
    offsets, rows = synth.synth_csr(nq + extra, D, seed=5)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=9))
    K = pipeline.max_candidates(nq)
    sig, norm2, keys = ops.minhash(offsets, rows, table, b=b, want_norm=True, compact=ops.can_compact(table))
    qi = QueryIndex(sig[:nq].contiguous(), norm2[:nq].contiguous(), b, table=table, keys=keys[:, :nq].contiguous(), K=K)
    off_h = offsets.cpu().numpy()
    for lo in range(nq, nq + extra, extra // 4):
        hi = lo + extra // 4
        if lo == nq:        # the first batch from its answer sets, the others from their rows
            o = (offsets[lo:hi + 1] - offsets[lo]).contiguous()
            r = rows[int(off_h[lo]):int(off_h[hi])].contiguous()
            assert qi.add(o, r) == (lo, hi - lo)
        else:
            assert qi.append(sig[lo:hi], norm2[lo:hi].contiguous()) == (lo, hi - lo)
    _same_index(qi, QueryIndex(sig, norm2, b, table=table, keys=keys, K=K), "1 M + 16 384")
    pick = np.sort(np.random.default_rng(1).choice(extra, 4096, replace=False)) + nq
    pt = torch.from_numpy(pick).cuda()
    off, idx, milli, avail = (x.cpu().numpy() for x in qi.neighbours(sig[pt], norm2[pt], K=K + 1))
    s32 = ops.sig_to_int32(sig)
    nonempty = (s32[pt] >= 0).any(dim=1).cpu().numpy()
    assert nonempty.sum() >= 4000
    for x, qid in enumerate(pick.tolist()):
        ids, mi = idx[off[x]:off[x + 1]], milli[off[x]:off[x + 1]]
        if nonempty[x]:
            at = np.nonzero(ids == qid)[0]
            assert len(at) == 1 and mi[at[0]] == 1000, qid         # finds itself, an indexed query now
    for x in np.random.default_rng(2).choice(4096, 16, replace=False).tolist():
        wi, wm, wa = AC.device_restate_probe(s32, b, s32[int(pick[x])], K + 1)
        assert avail[x] == wa and np.array_equal(idx[off[x]:off[x + 1]], wi) and \
            np.array_equal(milli[off[x]:off[x + 1]], wm), pick[x]


# ------------------------------------------------------------------------------------------------ 6. Recommender
def _perm(rec):
    t = rec.last_table
    tab = t.tab.cpu().numpy()
    if tab.dtype == np.int16:
        tab = tab.view(np.uint16).astype(np.int32)
    return np.ascontiguousarray(tab[:, :t.P].T)


def _host_rows(rec, q):
    from qrlsh import answers
    off, rows = answers.answer_sets(rec._answer_index, answers.encode_queries(rec._answer_index, q))
    return O.minhash(off.cpu().numpy(), rows.cpu().numpy(), _perm(rec))


@pytest.mark.parametrize("sub", ["cfg1", "cfg1b", "cfg2"])
def test_recommender_add_queries_end_to_end(sub):
    import predict_cases as PC
    from test_gpu_recommend import _recommender_on
    from test_recommend_host import restate
    from test_query_index_host import restate_columns
    rec, _ = _recommender_on(sub)
    q = np.asarray(rec.queries, dtype=object)
    ds = rec.dataset
    row = [str(ds[f].iloc[3]) for f in rec.datasetFeatures]
    new = [list(q[0]), list(q[-1])]
    new.append([row[0]] + [""] * (len(row) - 1))
    new.append([row[0], row[1] if len(row) > 1 else ""] + [""] * (len(row) - 2))
    new.append(["no-such-value"] + [""] * (len(row) - 1))
    new = np.array(new, dtype=object)
    with pytest.raises(ValueError):
        rec.add_queries(new)                      # compute_querySimilarities has not run
    rec.compute_scores()
    res = rec.last_result
    n, nu = rec.queriesIDs.size, rec.usersIDs.size
    b, K = res.b, res.K
    sig = res.sig_int32().cpu().numpy()
    held = (res.sig.clone(), res.norm2.clone(), res.sig.data_ptr())
    shapes = (rec.queries.shape, rec.queriesIDs.shape, rec.ratings.shape)
    old_ratings = rec.ratings.copy()
    block = np.random.default_rng(5).integers(0, 101, size=(nu, 5)) * (np.random.default_rng(6).random((nu, 5)) < 0.5)
    with pytest.raises(ValueError):
        rec.add_queries(new, ratings=block[:, :4])
    with pytest.raises(ValueError):
        rec.add_queries(new, ids=["a", "b"])
    pos = rec.add_queries(new, ratings=block, ids=["N%d" % k for k in range(5)])
    assert np.array_equal(pos, np.arange(n, n + 5))
    # the recommender grew by 5; the closed-set run's output is untouched
    assert rec.queries.shape == (shapes[0][0] + 5, shapes[0][1]) and rec.queriesIDs.shape == (shapes[1][0] + 5,)
    assert rec.ratings.shape == (shapes[2][0], shapes[2][1] + 5)
    assert np.array_equal(rec.ratings[:, :n], old_ratings) and np.array_equal(rec.ratings[:, n:], block)
    assert list(rec.queriesIDs[n:]) == ["N%d" % k for k in range(5)]
    assert np.array_equal(np.asarray(rec.queries[n:], dtype=object), new)
    assert rec.last_result is res and res.sig.data_ptr() == held[2] and res.sig.shape[0] == n
    assert torch.equal(res.sig, held[0]) and torch.equal(res.norm2, held[1])
    assert rec._query_index.n == n + 5 and rec._query_index.K == K
    # restatement: the signatures of all n + 5 queries and the extended ratings
    all_sig = np.vstack([sig, _host_rows(rec, new)])
    more = np.array([list(new[2]), list(new[3]), list(q[1]), list(new[4]), list(q[0])], dtype=object)
    xs = _host_rows(rec, more)
    assert n + 2 in QC.restate_candidates(all_sig, b, xs[0]).tolist()      # an added query is a candidate now
    want = QC.restate_probe(all_sig, b, xs, K)
    sims = rec.similar_queries(more)
    for x, (ids, mi, avail) in enumerate(want):
        if avail == 0:
            assert x not in sims
        else:
            assert np.array_equal(sims[x]["indexes"], ids) and np.array_equal(sims[x]["values"], mi / 1000.0)
    lists = [{"indexes": ids, "values": mi / 1000.0} for ids, mi, _ in want]
    for order, summ in (("pairwise", O.np_sum_order), ("sequential", PC.sequential_sum)):
        pred = rec.predict_new_queries(more, sum_order=order)
        assert pred.shape == (nu, len(more))
        assert np.array_equal(pred.to_numpy().T, restate_columns(rec.ratings, lists, summ))
    recs = rec.recommend_new_queries(more, 5, sum_order="pairwise")
    cols = restate_columns(rec.ratings, lists)
    wi, wv, wa = restate(np.zeros_like(cols), cols, 5)
    for x in range(len(more)):
        k = min(5, int(wa[x]))
        assert recs[x]["available"] == wa[x]
        assert np.array_equal(recs[x]["users"], wi[x, :k]) and np.array_equal(recs[x]["values"], wv[x, :k])
    # default ratings and ids: zeros, and the positions
    pos = rec.add_queries(more[:2])
    assert np.array_equal(pos, [n + 5, n + 6]) and rec.ratings.shape[1] == n + 7
    assert not rec.ratings[:, n + 5:].any() and [str(v) for v in rec.queriesIDs[n + 5:]] == [str(n + 5), str(n + 6)]


# ------------------------------------------------------------------------------------------------ 7. LSH
def test_lsh_query_appends_instead_of_rebuilding():
    from lsh import LSH
    g = QC.load("full_p160")
    sig = g["sig"].astype(np.int32)
    b = int(g["b"])
    lsh = LSH(b)
    lsh.compute_buckets_batch(sig[:400])
    got = lsh.query(sig[700:])
    for x, s in enumerate(got):
        assert s == set(QC.restate_candidates(sig[:400], b, sig[700 + x]).tolist())
    index = lsh._index
    assert index.n == 400
    lsh.compute_buckets_batch(sig[400:700])
    got = lsh.query(sig[700:])
    for x, s in enumerate(got):
        assert s == set(QC.restate_candidates(sig[:700], b, sig[700 + x]).tolist())
    assert lsh._index is index and index.n == 700
    _same_index(index, _index(sig[:700], b, index.K), "lsh")


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_argument_errors():
    from qrlsh import _lib, ops
    rng = np.random.default_rng(9)
    P, b = 32, 8
    sig = _random_rows(rng, 200, P)
    qi = _index(sig[:100], b)
    with pytest.raises(ValueError):
        qi.append(_rows(np.zeros((3, P + 8), dtype=np.int32)))                         # P mismatch
    with pytest.raises(ValueError):
        qi.append(_rows(sig[100:110]), norm2=torch.zeros((9,), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        qi.append(_rows(sig[100:110]), keys=torch.zeros((b, 9), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        qi.append(_rows(sig[100:110]), keys=torch.zeros((b + 1, 10), dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        qi.append(sig[100:110])
    assert qi.n == 100
    _same_index(qi, _index(sig[:100], b), "after refused appends")
    lib = _lib.load()
    vp = ctypes.c_void_p
    # n + m at the id limit: refused on the sizes alone, before any pointer is looked at (nothing is allocated)
    lim = 2**32 - 1
    for n, m in ((lim - 5, 5), (0, lim), (lim - 1, 1), (5, lim - 5)):
        rc = lib.qrlsh_index_append(vp(), vp(), vp(), n, 4, vp(), m, vp(), vp(), vp(), vp(), 0, vp())
        assert rc == _lib.QRLSH_EINVAL, (n, m)
        assert b"2^32" in lib.qrlsh_last_error() or b"bad sizes" in lib.qrlsh_last_error()
    rc = lib.qrlsh_index_append(vp(), vp(), vp(), lim - 6, 4, vp(), 5, vp(), vp(), vp(), vp(), 0, vp())
    assert rc == _lib.QRLSH_EINVAL and b"null pointer" in lib.qrlsh_last_error()       # sizes fine: the pointers are not
    assert lib.qrlsh_index_append(vp(), vp(), vp(), lim - 6, 4, vp(), 0, vp(), vp(), vp(), vp(), 0, vp()) == _lib.QRLSH_OK
    assert lib.qrlsh_index_append(vp(), vp(), vp(), 10, 0, vp(), 5, vp(), vp(), vp(), vp(), 0, vp()) == _lib.QRLSH_EINVAL
    # a workspace that is too small
    need = lib.qrlsh_index_append_workspace_bytes(10, b)
    assert need > 0 and lib.qrlsh_index_append_workspace_bytes(0, b) == 0
    nk = ops.band_keys(_rows(sig[100:110]), b)
    ko = torch.empty((b, 110), dtype=torch.int64, device="cuda")
    io = torch.empty((b, 110), dtype=torch.int32, device="cuda")
    do = torch.empty((int(lib.qrlsh_index_dir_words(110, b)),), dtype=torch.int32, device="cuda")
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    p = lambda t: vp(t.data_ptr())
    st = vp(torch.cuda.current_stream().cuda_stream)
    rc = lib.qrlsh_index_append(p(qi.keys), p(qi.ids), p(qi.dir), 100, b, p(nk), 10, p(ko), p(io), p(do), p(ws), need - 1, st)
    assert rc == _lib.QRLSH_EWORKSPACE
    with pytest.raises(ValueError):
        ops.index_append(qi.keys, qi.ids, qi.dir, torch.zeros((b + 1, 4), dtype=torch.int64, device="cuda"))
    # and the same call with the workspace it asked for is the append
    rc = lib.qrlsh_index_append(p(qi.keys), p(qi.ids), p(qi.dir), 100, b, p(nk), 10, p(ko), p(io), p(do), p(ws), need, st)
    assert rc == _lib.QRLSH_OK
    fresh = _index(sig[:110], b)
    assert torch.equal(ko, fresh.keys) and torch.equal(io, fresh.ids) and torch.equal(do, fresh.dir)


# ------------------------------------------------------------------------- 9. the run's index is bound where it is made
@pytest.fixture(scope="module")
def cfg2_run():
    """a Recommender on golden cfg2 (700 dataset rows) after one compute_querySimilarities, and the dict the run returned"""
    from test_gpu_recommend import _recommender_on
    rec, _ = _recommender_on("cfg2")
    return rec, rec.compute_querySimilarities()


FIRST_LIVE_CALLS = {
    "similar_queries": lambda rec, K: rec.similar_queries(np.asarray(rec.queries, dtype=object)[:1]),
    "remove_queries": lambda rec, K: rec.remove_queries([]),
    "remove_rows": lambda rec, K: rec.remove_rows([]),
    "set_list_lengths": lambda rec, K: rec.set_list_lengths(query_K=K),
    "tune": lambda rec, K: rec.tune([(0.6, 0.4, 60.0)], q_cuts=[K], fraction=0.5, seed=3, apply_cuts=True),
}


@pytest.mark.parametrize("route", sorted(FIRST_LIVE_CALLS))
def test_first_live_call_binds_the_runs_index_and_keeps_its_lists(cfg2_run, route):
    """Each of the five routes to the index of the last run, as the first live call after the run (on a copy of the
    run's state: no route writes what the copies share), leaves the index bound, over the served queries, and
    current_query_similarities() what the run itself returned."""
    import copy
    ran, run = cfg2_run
    rec = copy.copy(ran)
    assert rec._query_index is None and rec.last_result is ran.last_result
    FIRST_LIVE_CALLS[route](rec, int(rec.last_result.K))
    assert rec._query_index is not None and rec._query_index.n == rec.queriesIDs.size
    now = rec.current_query_similarities()
    assert list(now) == list(run) and len(run) > 0
    for q, want in run.items():
        assert sorted(now[q]) == ["indexes", "values"]
        for key in ("indexes", "values"):
            assert now[q][key].dtype == want[key].dtype and np.array_equal(now[q][key], want[key]), (q, key)
    assert ran._query_index is None
