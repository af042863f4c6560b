"""The plain definitions of tests/shard_cases.py against the test backend the gloo driver tests rest on
(tests/dist_worker.py:OracleBackend) and against the oracle, on every case; the comparison the GPU tests use against
planted defects; and the argument rules of the Python layer.  No GPU."""
import numpy as np
import pytest
import torch

import shard_cases as S
from dist_worker import OracleBackend, pair_host
from oracle import oracle as O  # checker only
from qrlsh import ops

B = OracleBackend()


def t64(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy())


def host(t):
    return None if t is None else t.numpy()


IDSET = S.idset_cases(large=False) + [("scan", S.idset_case(S.IDSET_SCAN[1], 5, 2, 2000, 9))]


# ---------------------------------------------------------------------------- the twin against the definitions
@pytest.mark.parametrize("label,case", IDSET, ids=[l for l, _ in IDSET])
def test_twin_id_set_equals_the_definition(label, case):
    pairs, q0, nql, nids, world = (case[k] for k in ("pairs", "q0", "nql", "nids", "world"))
    need = S.ref_need(pairs, q0, nql)
    rid = B.remote_ids(t64(pairs), q0, nql, nids, world)
    assert S.same(host(rid.bounds), S.ref_bounds(need, nql, world, nids))
    assert S.same(host(B.remote_id_list(rid, len(need))), np.array(need, dtype=np.int64))
    assert S.same(host(B.remap_pairs(t64(pairs), rid)), S.ref_slots(pairs, q0, nql, need))
    # the binary-search statement of the slot agrees with the position statement wherever both are defined
    mine = S.search_case(case)
    want = S.ref_slots(mine, q0, nql, need)
    assert S.same(S.ref_remap_search(mine, q0, nql, need), want)


def test_twin_gather_rows_equals_the_definition():
    for row_bytes, kind, P in S.ROW_FORMS:
        sig, norm2 = S.row_table(300, kind, P, seed=row_bytes)
        assert sig.shape[1] * sig.itemsize == row_bytes
        for q0 in (0, 12345):
            for form, n in (("mixed", 500), ("equal", 7), ("mixed", 0), ("mixed", 1)):
                ids = S.request_ids(300, q0, n, seed=n + q0, form=form)
                rows, norms = B.gather_rows(torch.from_numpy(sig), torch.from_numpy(norm2), torch.from_numpy(ids), q0)
                want_rows, want_norms = S.ref_gather_rows(sig, norm2, ids, q0)
                assert S.same(host(rows), want_rows) and S.same(host(norms), want_norms), (row_bytes, q0, form, n)


@pytest.mark.parametrize("off_dtype,row_dtype,D", [(np.int32, np.int16, 65536), (np.int64, np.int32, 70000), (np.int32, np.int32, 70000)])
def test_twin_gather_sets_equals_the_definition(off_dtype, row_dtype, D):
    for world, nql, empty in ((5, 61, 3), (1, 200, None), (7, 1, None)):
        offs, rows, sets = S.shard_sets(world, nql, D, seed=world, empty_shard=empty, off_dtype=off_dtype, row_dtype=row_dtype)
        for n in (0, 1, 15, 16, 17, 600):
            ids = S.set_ids(world, nql, n, seed=n)
            off, got = B.gather_sets(torch.from_numpy(ids), torch.from_numpy(offs), torch.from_numpy(rows), nql)
            want_off, want_rows = S.ref_gather_sets(ids, sets, nql)
            assert S.same(host(off), want_off) and S.same(host(got), want_rows), (world, n)


@pytest.mark.parametrize("id_bits", [1, 17, 26])
def test_twin_edge_words_and_owner_groups_equal_the_definition(id_bits):
    for n in S.PAIR_COUNTS:
        pairs, milli = S.edge_case(id_bits, n, seed=id_bits + n)
        for wide in (False, True):
            keys, dst = B.edges(t64(pairs), torch.from_numpy(milli), id_bits, wide)
            want_keys, want_dst = S.ref_edges(pairs, milli, id_bits, wide)
            assert S.same(host(keys), want_keys) and (dst is None) == (want_dst is None)
            assert dst is None or S.same(host(dst), want_dst)
            world = 5
            nql = S.ceil_div(1 << id_bits, world)
            lo = 11 if wide else id_bits + 11
            gk, gd, gb = B.group_edges_by_owner(keys, dst, lo, nql, world)
            wk, wd, wb = S.ref_group_by_owner(want_keys, want_dst, lo, nql, world)
            assert S.same(host(gk), wk) and S.same(host(gb), wb) and (gd is None or S.same(host(gd), wd))


LOCAL = [(1, 0, 1024, 1), (17, 3_000_000, 1025, 40), (26, 0, 1024, 256), (27, 3_000_000, 1025, 300), (32, 0, 1024, 40)]


@pytest.mark.parametrize("id_bits,q0,nql,K", LOCAL)
def test_twin_local_topk_equals_the_definition(id_bits, q0, nql, K):
    triples = S.local_edges_case(id_bits, q0, nql, K, seed=id_bits)
    for wide in ([True] if id_bits > 26 else [False, True]):
        keys, dst = S.pack_triples(triples, id_bits, wide)
        got = B.topk_local(t64(keys), None if dst is None else torch.from_numpy(dst), K, id_bits, q0, nql)
        for g, w in zip(got, S.ref_topk(triples, K)):
            assert S.same(host(g), w)
        # the re-based key orders like the triple: its sort is the definition's sort
        loc = S.ref_localize(keys, dst, id_bits, q0)
        by_key = [triples[t] for t in np.argsort(loc, kind="stable")]
        assert by_key == sorted(triples)


def test_boundary_key_has_64_bits_and_its_top_bit_set():
    id_bits, nql, lengths = S.boundary_case(40, seed=1)
    triples = S.local_edges_case(id_bits, 0, nql, 40, seed=2, lengths=lengths)
    keys, dst = S.pack_triples(triples, id_bits, wide=True)
    loc = S.ref_localize(keys, dst, id_bits, 0)
    assert (loc >> np.uint64(63)).any() and (loc.view(np.int64) < 0).any() and not (loc >> np.uint64(63)).all()
    got = B.topk_local(t64(keys), torch.from_numpy(dst), 40, id_bits, 0, nql)
    for g, w in zip(got, S.ref_topk(triples, 40)):
        assert S.same(host(g), w)


@pytest.mark.parametrize("world,nq", S.CHAIN_SHAPES)
def test_local_topk_of_shuffled_edges_is_the_global_topk_restricted(world, nq):
    """what the chain test of the GPU module expects: per rank, the cut over the edges whose src it owns (any order)
    is O.topk over all sorted pairs, restricted to its queries"""
    case = S.chain_case(world, nq, 24, seed=world, shards=(0, 3, 12) if world == 13 else None)
    pairs, nql = case["pairs"], case["nql"]
    assert S.same(case["host"], pair_host(pairs, nql))
    milli = O.score_pairs(S.sig_rows(case["sig"], "i32"), pairs, mode=1)
    K, ib = 7, ops.id_bits_for(world * nql)
    s0, d0, v0 = O.topk(pairs, milli, K)
    rng = np.random.default_rng(world)
    for wide in (False, True):
        keys, dst = S.ref_edges(pairs, milli, ib, wide)
        src = np.array([int(k) >> (11 if wide else ib + 11) for k in keys])
        parts = []
        for rank in range(world):
            q0 = rank * nql
            mine = rng.permutation(np.flatnonzero((src >= q0) & (src < q0 + nql)))
            got = B.topk_local(t64(keys[mine]), None if dst is None else torch.from_numpy(dst[mine]), K, ib, q0, nql)
            sel = (s0 >= q0) & (s0 < q0 + nql)
            assert S.same(host(got[0]), s0[sel]) and S.same(host(got[1]), d0[sel]) and S.same(host(got[2]), v0[sel])
            parts.append(len(mine))
        assert sum(parts) == 2 * len(pairs) and (world != 13 or parts.count(0) == 10)


def test_pair_host_definition_equals_the_oracle_filter():
    case = S.chain_case(5, 603, 8, seed=3)
    for rank in range(5):
        assert S.same(O.filter_pair_host(case["pairs"], case["nql"], rank), case["pairs"][case["host"] == rank])


@pytest.mark.parametrize("P,b", S.VERIFY_SHAPES)
def test_twin_verify_flags_equal_the_definition_on_compact_values(P, b):
    """OracleBackend.verify_flags goes through O.candidates_from_sig, whose buckets compare int16 tuples: it is held
    to the definition on values a compact row can carry (the low-16 rule on wider int32 values is the device's own
    documented rule, pinned in the GPU module against the band keys)"""
    sig, pairs, _ = S.verify_case(P, b, False, seed=P)
    i, j = np.array(S.endpoints(pairs)).T
    distinct = i != j                                           # the candidate set holds pairs of two queries only
    got = B.verify_flags(torch.from_numpy(S.sig_rows(sig, "i32")), b, t64(pairs[distinct]))
    assert S.same(host(got), S.ref_verify(sig, b, pairs)[distinct])


@pytest.mark.parametrize("P", [24, 128])
def test_twin_split_scores_equal_the_oracle_over_the_whole_table(P):
    sig, pairs = S.split_case(P, 50, 30, 17, seed=P)
    rows = torch.from_numpy(S.sig_rows(sig, "i32"))
    got = B.score(rows[:50], None, rows[50:], None, t64(pairs))
    assert S.same(host(got), O.score_pairs(S.sig_rows(sig, "i32"), pairs, mode=1))


# ---------------------------------------------------------------------------- planted defects
def test_the_comparison_rejects_each_planted_defect():
    """each defect is planted in a copy of a correct output (or restated as the wrong rule over the same inputs) and
    must fail S.same, the comparison of tests/test_gpu_shard.py"""
    rejected = []
    # 1. a rank that is off by one at a word boundary of the bitmap: ids at bit 0 of a word rank one too high
    case = S.idset_case(5003, 5, 2, 500, seed=11)
    pairs, q0, nql = case["pairs"], case["q0"], case["nql"]
    need = S.ref_need(pairs, q0, nql)
    good = S.ref_slots(pairs, q0, nql, need)
    assert any(x % 32 == 0 for x in need)
    bad = S.words(((si + (si >= nql and need[si - nql] % 32 == 0)) << 32) | (sj + (sj >= nql and need[sj - nql] % 32 == 0))
                  for si, sj in S.endpoints(good))
    assert not S.same(bad, good) and S.same(good.copy(), good)
    rejected.append("rank off by one at a word boundary")
    # 2. a slot taken from `need` without the nql base
    bad = S.words(((si - nql if si >= nql else si) << 32) | (sj - nql if sj >= nql else sj) for si, sj in S.endpoints(good))
    assert not S.same(bad, good)
    rejected.append("slot without the nql base")
    # 3. a row gathered at id instead of id - q0
    sig, norm2 = S.row_table(300, "u16", 24, seed=12)
    ids = S.request_ids(300, 7, 500, seed=13)
    good_rows, good_norms = S.ref_gather_rows(sig, norm2, ids, 7)
    bad_rows, bad_norms = S.ref_gather_rows(sig, norm2, np.minimum(ids + 7, 7 + 299), 7)
    assert not S.same(bad_rows, good_rows) and not S.same(bad_norms, good_norms)
    rejected.append("row at id instead of id - q0")
    # 4. an edge key built with the inv and dst fields swapped
    ep, milli = S.edge_case(17, 257, seed=14)
    good_keys, _ = S.ref_edges(ep, milli, 17, False)
    bad = S.words(((int(k) >> 28) << 28) | ((int(k) & 0x1FFFF) << 11) | ((int(k) >> 17) & 0x7FF) for k in good_keys)
    assert not S.same(bad, good_keys)
    rejected.append("inv and dst swapped")
    # 5. a localised key that loses bit 63
    id_bits, bnql, lengths = S.boundary_case(40, seed=1)
    triples = S.local_edges_case(id_bits, 0, bnql, 40, seed=2, lengths=lengths)
    keys, dst = S.pack_triples(triples, id_bits, wide=True)
    good_loc = S.ref_localize(keys, dst, id_bits, 0)
    assert not S.same(good_loc & np.uint64((1 << 63) - 1), good_loc)
    rejected.append("bit 63 lost")
    # 6. a verify flag that counts a band that is all -1 in both rows
    vsig, vpairs, labels = S.verify_case(40, 8, False, seed=15)
    good_flags = S.ref_verify(vsig, 8, vpairs)
    r = 5
    bad_flags = np.array([int(any(list(vsig[i, k * r:(k + 1) * r]) == list(vsig[j, k * r:(k + 1) * r]) for k in range(8)))
                          for i, j in S.endpoints(vpairs)], dtype=np.uint8)
    assert bad_flags[labels.index("a band all -1 in both")] == 1 and not S.same(bad_flags, good_flags)
    rejected.append("all -1 band counted")
    assert len(rejected) == 6
    # and what the comparison does not forgive: a carrier of another width, a missing element
    assert not S.same(good_flags.astype(np.int32), good_flags) and not S.same(good_keys[:-1], good_keys)
    assert S.same(good_keys.view(np.int64), good_keys)


# ---------------------------------------------------------------------------- the argument rules of the Python layer
def test_python_layer_argument_rules():
    assert not ops.wide_ids(26) and ops.wide_ids(27)
    assert ops.local_bits_for(1) == 1 and ops.local_bits_for(2) == 1
    for k in range(1, 33):
        assert ops.local_bits_for(1 << k) == k and ops.local_bits_for((1 << k) + 1) == k + 1
        assert S.local_bits(1 << k) == k and S.local_bits((1 << k) + 1) == k + 1
    assert S.local_bits(1) == 1 and S.local_bits(2) == 1
    one = torch.zeros(1, dtype=torch.int64)
    d = torch.zeros(1, dtype=torch.int32)
    id_bits, nql, _ = S.boundary_case(40, seed=1)
    assert ops.local_bits_for(nql) + 11 + id_bits == 64 and ops.local_bits_for(nql + 1) + 11 + id_bits == 65
    with pytest.raises(NotImplementedError):
        ops.topk_edges_local(one, d, 40, id_bits, 0, nql + 1)
    with pytest.raises(NotImplementedError):
        ops.topk_edges_local(one, None, 40, 26, 0, (1 << 27) + 1)
