"""The device glue of the query-sharded step against the plain definitions of tests/shard_cases.py, bit for bit:
csrc/shard.hip (id set, row and answer-set gathers, re-based edge keys), the tail of csrc/score.hip (binary-search
remap, edge words, the exact band predicate, scoring over a two-piece table) and ops.topk_edges_local in both forms.
Sizes are the smallest that reach the path each test names (shard_cases: WHICH PATH A SIZE RUNS).  Every comparison is
S.same -- whole outputs, exact integers, no tolerance; outputs the tests allocate are pre-filled with a value no
result produces.  No id, row index or offset handed to a kernel leaves its range; the refusals tested are made by
ops or by the C entry points before any launch."""
import numpy as np
import pytest
import torch

import minhash_cases as M
import shard_cases as S
from oracle import oracle as O  # checker only

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402
from qrlsh.dist import HipBackend  # noqa: E402

DEV = "cuda"
H = HipBackend()
FILL64, FILL32 = -0x0101010101010102, -0x01010102        # int64 / int32 carriers of 0xFE.. words


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def d64(words):
    return dev(np.ascontiguousarray(words).view(np.int64))


def host(t):
    return None if t is None else t.cpu().numpy()


def total_of(rid):
    return int(rid.bounds[-1].item())


# ---------------------------------------------------------------------------- 1. id set
def check_id_set(case):
    pairs, q0, nql, nids, world = (case[k] for k in ("pairs", "q0", "nql", "nids", "world"))
    need = S.ref_need(pairs, q0, nql)
    p = d64(pairs)
    rid = H.remote_ids(p, q0, nql, nids, world)
    assert S.same(host(rid.bounds), S.ref_bounds(need, nql, world, nids))
    assert S.same(host(H.remote_id_list(rid, total_of(rid))), np.array(need, dtype=np.int64))
    assert S.same(host(H.remap_pairs(p, rid)), S.ref_slots(pairs, q0, nql, need))
    # the binary-search entry on the pairs whose first end is local
    mine = S.search_case(case)
    got = ops.remap_pairs(d64(mine), q0, nql, dev(np.array(need, dtype=np.int64)))
    assert S.same(host(got), S.ref_remap_search(mine, q0, nql, need))


SMALL = S.idset_cases(large=False)
LARGE = [c for c in S.idset_cases(large=True) if c[0] not in {l for l, _ in SMALL}]


@pytest.mark.parametrize("label,case", SMALL, ids=[l for l, _ in SMALL])
def test_id_set_at_word_shard_and_pair_count_edges(label, case):
    check_id_set(case)


@pytest.mark.parametrize("label,case", LARGE, ids=[l for l, _ in LARGE])
def test_id_set_multi_launch_scan_and_wide_ids(label, case):
    """nids = 1 048 544 is the last size whose rank structure is scanned by one workgroup; the next two take the
    chunked three-launch scan; 2^27 + 5 has ids past 2^26 (16 MB of bitmap, 32 MB of prefix)"""
    nw1 = S.ceil_div(case["nids"], 32) + 1
    assert (nw1 > S.SCAN_ONE_WORKGROUP) == (case["nids"] > S.IDSET_LAST_SINGLE_SCAN)
    check_id_set(case)


def test_remap_pairs_binary_search_entry_with_need_empty():
    """ops.remap_pairs (qrlsh_remap_pairs) with nothing to fetch: every second end is local"""
    case = S.all_local_case(5003, 5, 2, 300, seed=1)
    got = ops.remap_pairs(d64(case["pairs"]), case["q0"], case["nql"], dev(np.zeros(0, dtype=np.int64)))
    assert S.same(host(got), S.ref_remap_search(case["pairs"], case["q0"], case["nql"], []))
    assert ops.remap_pairs(d64(case["pairs"][:0]), case["q0"], case["nql"], dev(np.zeros(0, dtype=np.int64))).numel() == 0


def test_id_set_workspace_one_byte_short_is_refused_and_nothing_written():
    lib = _lib.load()
    case = S.idset_case(5003, 5, 2, 100, seed=2)
    nbytes = lib.qrlsh_idset_workspace_bytes(case["nids"])
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    bounds = torch.full((case["world"] + 1,), FILL64, dtype=torch.int64, device=DEV)
    p = d64(case["pairs"])
    rc = lib.qrlsh_idset_build(ops._ptr(p), p.numel(), case["q0"], case["nql"], case["nids"], case["nql"], case["world"],
                               ops._ptr(ws), nbytes - 1, ops._ptr(bounds), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.QRLSH_EWORKSPACE
    assert bool((ws == 0xAB).all()) and bool((bounds == FILL64).all())
    with pytest.raises(_lib.QrlshError):
        _lib.check(rc)


# ---------------------------------------------------------------------------- 2. gather_rows
@pytest.mark.parametrize("row_bytes,kind,P", S.ROW_FORMS, ids=["%dB" % f[0] for f in S.ROW_FORMS])
def test_gather_rows_every_row_width_offset_and_request_form(row_bytes, kind, P):
    nrows = 300
    sig, norm2 = S.row_table(nrows, kind, P, seed=row_bytes)
    assert sig.shape[1] * sig.itemsize == row_bytes
    d_sig, d_norm = dev(sig), dev(norm2)
    for q0 in (0, 12345):
        for form, n in (("mixed", 500), ("equal", 7), ("mixed", 1), ("mixed", 0)):
            ids = S.request_ids(nrows, q0, n, seed=n + q0, form=form)
            rows, norms = H.gather_rows(d_sig, d_norm, dev(ids), q0)
            want_rows, want_norms = S.ref_gather_rows(sig, norm2, ids, q0)
            assert S.same(host(rows), want_rows) and S.same(host(norms), want_norms), (q0, form, n)


def test_gather_rows_grid_stride_loop_with_q0():
    """140 000 rows of 256 bytes are 2 240 000 vectors: past the 2 097 152 the capped grid covers in one trip"""
    n, nrows, q0 = 140_000, 4096, 12345
    assert n * 16 > S.GATHER_ROWS_VECTORS_PER_TRIP
    sig, norm2 = S.row_table(nrows, "u16", 128, seed=3)
    ids = S.request_ids(nrows, q0, n, seed=4)
    rows, norms = H.gather_rows(dev(sig), dev(norm2), dev(ids), q0)
    want_rows, want_norms = S.ref_gather_rows(sig, norm2, ids, q0)
    assert S.same(host(rows), want_rows) and S.same(host(norms), want_norms)


def test_gather_rows_refuses_a_misaligned_table_and_writes_nothing():
    lib = _lib.load()
    P, nrows, n = 24, 64, 10
    flat = torch.zeros((nrows * P + 1,), dtype=torch.int16, device=DEV)
    sig = flat[1:].view(nrows, P)                                   # an odd element offset: 2 bytes off a 16-byte line
    assert sig.data_ptr() % 16 == 2
    norm2 = torch.zeros((nrows,), dtype=torch.int64, device=DEV)
    ids = dev(np.arange(n, dtype=np.int64))
    rows = torch.full((n, P), 0x7EFE, dtype=torch.int16, device=DEV)
    norms = torch.full((n,), FILL64, dtype=torch.int64, device=DEV)
    rc = lib.qrlsh_gather_rows(ops._ptr(sig), P * 2, ops._ptr(norm2), ops._ptr(ids), n, 0, ops._ptr(rows), ops._ptr(norms),
                               ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.QRLSH_EINVAL and b"alignment" in lib.qrlsh_last_error()
    assert bool((rows == 0x7EFE).all()) and bool((norms == FILL64).all())
    with pytest.raises(_lib.QrlshError, match="alignment"):
        ops.gather_rows(sig, norm2, ids, 0)


# ---------------------------------------------------------------------------- 3. gather_sets
SET_FORMS = [(np.int32, np.int16, 65536), (np.int64, np.int32, 70000), (np.int32, np.int32, 70000), (np.int64, np.int16, 65536)]


@pytest.mark.parametrize("off_dtype,row_dtype,D", SET_FORMS, ids=["o%d-r%d" % (np.dtype(o).itemsize * 8, np.dtype(r).itemsize * 8)
                                                                    for o, r, _ in SET_FORMS])
def test_gather_sets_every_width_count_and_both_scans(off_dtype, row_dtype, D):
    """n + 1 <= 32 768 lengths are scanned by one workgroup, 32 768 and 40 000 ids by the chunked scan; 16-bit row
    ids at and past 32 768 widen unsigned; a shard of empty sets, world = 1 and nql = 1"""
    for world, nql, empty, counts in ((5, 61, 3, S.SETS_N), (1, 200, None, (0, 1, 17, 600)), (7, 1, None, (0, 1, 16, 50)),
                                      (2, 30, 0, (33,))):
        offs, rows, sets = S.shard_sets(world, nql, D, seed=world, empty_shard=empty, off_dtype=off_dtype, row_dtype=row_dtype)
        d_offs, d_rows = dev(offs), dev(rows)
        for n in counts:
            ids = S.set_ids(world, nql, n, seed=n)
            assert n == 0 or (0 <= ids.min() and ids.max() < world * nql)
            off, got = H.gather_sets(dev(ids), d_offs, d_rows, nql)
            want_off, want_rows = S.ref_gather_sets(ids, sets, nql)
            assert S.same(host(off), want_off) and S.same(host(got), want_rows), (world, nql, n)
    # a request that meets empty sets only: no row id, and the fill is not launched
    offs, rows, sets = S.shard_sets(3, 20, D, seed=9, empty_shard=1, off_dtype=off_dtype, row_dtype=row_dtype)
    ids = np.arange(20, 40, dtype=np.int64)[::-1].copy()
    off, got = H.gather_sets(dev(ids), dev(offs), dev(rows), 20)
    assert S.same(host(off), np.zeros(21, dtype=np.int64)) and got.numel() == 0


# ---------------------------------------------------------------------------- 4. edge words
@pytest.mark.parametrize("id_bits", [1, 17, 26])
def test_pair_edges_packed_and_key_payload_separate_and_interleaved(id_bits):
    """forward / reverse arrays and the interleaved array, in both formats, fwd_dst and rev_dst included, over ids 0 ..
    2^id_bits - 1 and milli -1000 .. 1000 (inv up to 2000)"""
    for n in S.PAIR_COUNTS + (3000,):
        pairs, milli = S.edge_case(id_bits, n, seed=id_bits + n)
        p, m = d64(pairs), dev(milli)
        for wide in (False, True):
            want_keys, want_dst = S.ref_edges(pairs, milli, id_bits, wide)
            inter = ops.pair_edges_interleaved(p, m, id_bits, wide)
            fwd, rev = ops.pair_edges(p, m, id_bits, wide)
            if wide:
                assert S.same(host(inter[0]), want_keys) and S.same(host(inter[1]), want_dst), n
                assert S.same(host(fwd[0]), want_keys[0::2]) and S.same(host(fwd[1]), want_dst[0::2]), n
                assert S.same(host(rev[0]), want_keys[1::2]) and S.same(host(rev[1]), want_dst[1::2]), n
            else:
                assert S.same(host(inter), want_keys), n
                assert S.same(host(fwd), want_keys[0::2]) and S.same(host(rev), want_keys[1::2]), n
            keys, dst = H.edges(p, m, id_bits, wide)
            assert S.same(host(keys), want_keys) and (dst is None if not wide else S.same(host(dst), want_dst))


@pytest.mark.parametrize("id_bits", [1, 17, 26])
def test_pair_edges_equal_what_score_pairs_writes(id_bits):
    """the edge words of ops.score_pairs(..., edge_id_bits=) for pairs over a small table (rows of an empty answer set
    among them: negative scores) equal pair_edges of the same pairs and scores, and the definition"""
    nrows = min(1 << id_bits, 1 << 17)
    rng = np.random.default_rng(id_bits)
    sig = rng.integers(0, 40, size=(nrows, 8)).astype(np.int64)
    sig[::3] = -1
    if nrows > 2:
        sig[nrows - 1] = 7
    rows = S.sig_rows(sig, "u16")
    for n in (0, 1, 257):
        a, c = rng.integers(0, nrows, size=n), rng.integers(0, nrows, size=n)
        if n:
            a[0], c[0] = 0, nrows - 1
        pairs = S.pair_words(np.minimum(a, c), np.maximum(a, c))
        p = d64(pairs)
        want_milli = O.score_pairs(S.sig_rows(sig, "i32"), pairs, mode=1)
        assert n < 100 or ((want_milli < 0).any() and (want_milli > 0).any())
        for wide in (False, True):
            milli, _, edges = ops.score_pairs(dev(rows), dev(M.ref_norm2(sig)), p, edge_id_bits=id_bits, wide=wide)
            assert S.same(host(milli), want_milli)
            want_keys, want_dst = S.ref_edges(pairs, want_milli, id_bits, wide)
            inter = ops.pair_edges_interleaved(p, milli, id_bits, wide)
            if wide:
                assert S.same(host(edges[0]), want_keys) and S.same(host(edges[1]), want_dst)
                assert torch.equal(inter[0], edges[0]) and torch.equal(inter[1], edges[1])
            else:
                assert S.same(host(edges), want_keys) and torch.equal(inter, edges)


# ---------------------------------------------------------------------------- 5. re-based keys and the top-K cut
def check_local_topk(triples, id_bits, wide, K, q0, nql):
    keys, dst = S.pack_triples(triples, id_bits, wide)
    want = S.ref_topk(triples, K)
    # the re-based keys themselves
    loc = torch.full((len(triples),), FILL64, dtype=torch.int64, device=DEV)
    k, d = d64(keys), (None if dst is None else dev(dst))
    _lib.check(_lib.load().qrlsh_edges_localize(ops._ptr(k), ops._ptr(d), len(triples), id_bits, q0, nql, ops._ptr(loc),
                                                ops._stream()))
    assert S.same(host(loc), S.ref_localize(keys, dst, id_bits, q0))
    forms = (True, False) if K <= ops.SELECT_MAX_K else (True,)       # K = 300: the sort form through the switch
    for select in forms:
        got = ops.topk_edges_local(k.clone(), d, K, id_bits, q0, nql, select=select)
        for g, w in zip(got, want):
            assert S.same(host(g), w), (id_bits, wide, K, q0, nql, select)
    got = H.topk_local(k.clone(), d, K, id_bits, q0, nql)
    for g, w in zip(got, want):
        assert S.same(host(g), w)


@pytest.mark.parametrize("id_bits,wide", [(1, False), (17, False), (26, False), (27, True), (32, True)])
def test_local_topk_select_and_sort_form_equal_the_lexsort_cut(id_bits, wide):
    """lists shorter than, equal to and longer than K, ties at the cut that arrival order would cut otherwise,
    negative milli; q0 = 0 and far from 0; nql at 2^k and 2^k + 1"""
    for q0 in (0, 3_000_000):
        for nql in (1024, 1025):
            for K in (1, 40, 256, 300):
                triples = S.local_edges_case(id_bits, q0, nql, K, seed=id_bits + K + nql)
                check_local_topk(triples, id_bits, wide, K, q0, nql)
    # edges for the first and the last local query only; a rank that receives no edge
    q0, nql, K = 3_000_000, 1025, 40
    check_local_topk(S.local_edges_case(id_bits, q0, nql, K, seed=5, lengths={0: 3, nql - 1: K + 2}), id_bits, wide, K, q0, nql)
    none = torch.empty((0,), dtype=torch.int64, device=DEV)
    for t in ops.topk_edges_local(none, None if not wide else torch.empty((0,), dtype=torch.int32, device=DEV), K, id_bits, q0, nql):
        assert t.numel() == 0 and t.dtype == torch.int32


@pytest.mark.parametrize("K", [1, 40, 256, 300])
def test_local_topk_at_the_64_bit_key(K):
    """id_bits = 32 and nql = 2^21: 21 + 11 + 32 = 64 key bits, the select form's src < 2^(53 - id_bits) exactly; local
    src 0 and nql - 1 carry edges, so keys with bit 63 set (negative as int64) are sorted and cut"""
    id_bits, nql, lengths = S.boundary_case(K, seed=K)
    triples = S.local_edges_case(id_bits, 0, nql, K, seed=K + 1, lengths=lengths)
    keys, dst = S.pack_triples(triples, id_bits, True)
    assert (S.ref_localize(keys, dst, id_bits, 0) >> np.uint64(63)).any()
    assert max(d for _, _, d in triples) < (1 << 31)
    check_local_topk(triples, id_bits, True, K, 0, nql)


def test_one_bit_past_the_64_bit_key_is_refused():
    id_bits, nql, lengths = S.boundary_case(40, seed=1)
    triples = S.local_edges_case(id_bits, 0, nql, 40, seed=2, lengths=lengths)
    keys, dst = S.pack_triples(triples, id_bits, True)
    k, d = d64(keys), dev(dst)
    with pytest.raises(NotImplementedError):
        ops.topk_edges_local(k, d, 40, id_bits, 0, nql + 1)
    lib = _lib.load()
    out = torch.full((len(triples),), FILL64, dtype=torch.int64, device=DEV)
    rc = lib.qrlsh_edges_localize(ops._ptr(k), ops._ptr(d), len(triples), id_bits, 0, nql + 1, ops._ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.QRLSH_EINVAL and bool((out == FILL64).all())
    # packed input past 26 id bits is refused as well
    rc = lib.qrlsh_edges_localize(ops._ptr(k), None, len(triples), 27, 0, 1024, ops._ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.QRLSH_EINVAL and bool((out == FILL64).all())


# ---------------------------------------------------------------------------- 6. the exact band predicate
@pytest.mark.parametrize("kind", ["i32", "u16"])
@pytest.mark.parametrize("P,b", S.VERIFY_SHAPES)
def test_verify_pairs_low_16_rule_agrees_with_the_band_keys(P, b, kind):
    """flags against the definition, and against equality of the hashed band keys of the same rows (ops.band_keys on
    their int32 form -- the standalone kernel, which tests/test_gpu_minhash.py pins to the keys ops.minhash fuses --
    held here to minhash_cases.ref_band_keys too): both are functions of the low 16 bits of every value, so int32
    values 65536 apart meet in a band and 65535 is the -1 of an empty set"""
    r = P // b
    for n in (0, 1, 257):
        sig, pairs, labels = S.verify_case(P, b, kind == "i32", seed=P + n, n=n)
        rows = dev(S.sig_rows(sig, kind))
        p = d64(pairs)
        flags = host(ops.verify_pairs(rows, b, p))
        want = S.ref_verify(sig, b, pairs)
        assert flags.dtype == np.uint8 and S.same(flags, want), (n, [l for l, f, w in zip(labels, flags, want) if f != w])
        kept = ops.drop_unverified(rows, b, p)
        assert S.same(host(kept), pairs[want == 1])
        if n == 0:
            continue
        keys = host(ops.band_keys(dev(sig.astype(np.int32)), b)).view(np.uint64).T          # [rows][b]
        assert S.same(keys, M.ref_band_keys(sig, b))
        low = (sig & 0xFFFF).reshape(len(sig), b, r)
        sentinel = np.all(low == 0xFFFF, axis=2)
        for t, (i, j) in enumerate(S.endpoints(pairs)):
            equal = keys[i] == keys[j]
            if not equal.any():
                assert flags[t] == 0
            match = equal & ~sentinel[i] & np.all(low[i] == low[j], axis=1)
            if match.any():
                assert flags[t] == 1
        if kind == "i32" and n > len(labels):
            assert sig.max() > 65535 and (sig == 65535).any()


# ---------------------------------------------------------------------------- 7. the two-piece row table
@pytest.mark.parametrize("kind,P", [("u16", 128), ("u16", 256), ("u16", 24), ("i32", 24)])
def test_score_pairs_split_every_form_split_and_pair_location(kind, P):
    """compact rows of 128 / 256 values take the run form when the norms are given, everything else the generic form;
    pairs with both halves own, both fetched and one of each; no fetched rows at all; norms summed from the rows"""
    for split in (1, 50):
        for n in (0, 1, 15, 16, 17, 200):
            sig, pairs = S.split_case(P, split, 30, n, seed=P + split + n)
            want = O.score_pairs(S.sig_rows(sig, "i32"), pairs, mode=1)
            rows, norm2, p = dev(S.sig_rows(sig, kind)), dev(M.ref_norm2(sig)), d64(pairs)
            assert S.same(host(ops.score_pairs(rows, norm2, p)[0]), want)
            a, na, bb, nb = rows[:split].contiguous(), norm2[:split].contiguous(), rows[split:].contiguous(), norm2[split:].contiguous()
            assert S.same(host(H.score(a, na, bb, nb, p)), want), (split, n)
            assert S.same(host(ops.score_pairs_split(a, None, bb, None, p)), want), (split, n, "own norms")
        # a rank whose pairs are all local: HipBackend.score hands the kernel sig[:0] for the fetched piece
        for n in (0, 1, 15, 16, 17, 200):
            nrows = max(split, 2)
            sig, pairs = S.split_case(P, nrows, 0, n, seed=P + n)
            want = O.score_pairs(S.sig_rows(sig, "i32"), pairs, mode=1)
            rows, norm2 = dev(S.sig_rows(sig, kind)), dev(M.ref_norm2(sig))
            assert S.same(host(H.score(rows, norm2, None, None, d64(pairs))), want), (nrows, n)


# ---------------------------------------------------------------------------- 8. the chain on one simulated rank
@pytest.mark.parametrize("world,nq", S.CHAIN_SHAPES)
def test_chain_of_one_simulated_rank_equals_the_one_gpu_result(world, nq):
    """the driver's slicing restated in one process, no collectives: every rank takes the pairs it hosts, finds and
    lists its remote ids, gathers their rows, re-indexes and scores its pairs, writes their edges; every rank then cuts
    the edges whose src it owns (gathered from all ranks, shuffled).  The ranks' lists joined are O.topk over all
    pairs; the scores are O.score_pairs.  Packed edges over compact rows, key + payload edges over int32 rows"""
    case = S.chain_case(world, nq, 24, seed=world, shards=(0, 3, 12) if world == 13 else None)
    pairs, nql, hosts = case["pairs"], case["nql"], case["host"]
    nids = world * nql
    K, ib = 7, ops.id_bits_for(nids)
    all_milli = O.score_pairs(S.sig_rows(case["sig"], "i32"), pairs, mode=1)
    want = O.topk(pairs, all_milli, K)
    rng = np.random.default_rng(world)
    for wide, kind in ((False, "u16"), (True, "i32")):
        sig, norm2 = dev(S.sig_rows(case["sig"], kind)), dev(M.ref_norm2(case["sig"]))
        keys_all, dst_all, idle = [], [], 0
        for rank in range(world):
            q0 = rank * nql
            mine = pairs[hosts == rank]
            idle += len(mine) == 0
            p = d64(mine)
            rid = H.remote_ids(p, q0, nql, nids, world)
            need = H.remote_id_list(rid, total_of(rid))
            assert S.same(host(need), np.array(S.ref_need(mine, q0, nql), dtype=np.int64))
            rows_b, norms_b = H.gather_rows(sig, norm2, need, 0)
            local = H.remap_pairs(p, rid)
            milli = H.score(sig[q0:q0 + nql].contiguous(), norm2[q0:q0 + nql].contiguous(), rows_b, norms_b, local)
            assert S.same(host(milli), all_milli[hosts == rank])
            k, d = H.edges(p, milli, ib, wide)
            keys_all.append(host(k).view(np.uint64))
            dst_all.append(host(d) if wide else None)
        assert (idle > 0) == (world == 13)
        keys = np.concatenate(keys_all)
        dst = np.concatenate(dst_all) if wide else None
        src = np.array([int(x) >> (11 if wide else ib + 11) for x in keys])
        got = [[], [], []]
        for rank in range(world):
            q0 = rank * nql
            sel = rng.permutation(np.flatnonzero((src >= q0) & (src < q0 + nql)))
            out = H.topk_local(d64(keys[sel]), dev(dst[sel]) if wide else None, K, ib, q0, nql)
            for lst, t in zip(got, out):
                lst.append(host(t))
        for lst, w in zip(got, want):
            assert S.same(np.concatenate(lst), w)
