"""Run bounds of the select form of the top-K (csrc/topk.hip: edge_bounds_kernel takes a run of consecutive words per
thread, edge_bounds_fix_kernel fills the long stretches without edges, topk_len_kernel leaves its workgroups' own
scans and totals for the offsets) through ops.topk_select, against the oracle's top-K: list lengths on every side of
the per-thread run, a change of source on every word and none at all, stretches without edges of exactly the walked
length, one more and a million, edges at the first and at the last query only, the reverse-only and wide-id forms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from qrlsh import ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
SEL_GAP = 32     # csrc/topk.hip: stretches of queries without edges up to here are walked, longer ones searched
RUN = 4          # words a thread of edge_bounds_kernel takes (EB_RUN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pack(i, j):
    return np.unique((np.asarray(i).astype(np.uint64) << np.uint64(32)) | np.asarray(j).astype(np.uint64))


def rev_words(pairs, milli, ib, wide):
    pi, pj = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
    inv = (1000 - milli.astype(np.int64)).astype(np.uint64)
    if wide:
        return dev(((pj << np.uint64(11)) | inv).view(np.int64)), dev(pi.astype(np.int32))
    return dev(((pj << np.uint64(ib + 11)) | (inv << np.uint64(ib)) | pi).view(np.int64))


def check(pairs, nq, K, seed=0, forms=(False, True)):
    """ops.topk_select on the sorted unique pairs (values with many ties) == the oracle's top-K, packed and wide words"""
    rng = np.random.default_rng(seed)
    milli = rng.integers(995, 1001, size=len(pairs)).astype(np.int32)
    milli[::7] = rng.integers(-1000, 1001, size=len(milli[::7]))
    ws, wd, wv = O.topk(pairs, milli, K)
    ib = ops.id_bits_for(nq)
    for wide in forms:
        got = ops.topk_select(dev(pairs.view(np.int64)), dev(milli), rev_words(pairs, milli, ib, wide), K, ib, nq)
        s, d, v = (t.cpu().numpy() for t in got)
        assert np.array_equal(s, ws) and np.array_equal(d, wd) and np.array_equal(v, wv), (len(pairs), nq, K, wide)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 255, 256 * RUN - 1, 256 * RUN, 256 * RUN + 1, 64 * RUN + 2, 100_003])
def test_list_lengths_around_the_per_thread_run(n):
    """n pairs (so n + 1 positions, the end included): the last thread's run is cut anywhere, a wave's first lane
    fetches the word before its run, a workgroup ends on the list's end"""
    rng = np.random.default_rng(n)
    nq = 5000
    pairs = np.zeros(0, dtype=np.uint64)
    while len(pairs) < n:                    # (unique pairs: draw until there are n, keep the n smallest)
        i, j = rng.integers(0, nq, size=2 * n + 16), rng.integers(0, nq, size=2 * n + 16)
        keep = i != j
        pairs = np.union1d(pairs, pack(np.minimum(i, j)[keep], np.maximum(i, j)[keep]))
    pairs = pairs[np.sort(rng.choice(len(pairs), size=n, replace=False))]
    assert len(pairs) == n
    check(pairs, nq, 3, seed=n)


def test_a_change_of_source_on_every_word_and_none_at_all():
    nq = 40_000
    i = np.arange(0, 19_999)
    check(pack(i, i + 20_000), nq, 5)                        # forward and reverse: every word another source
    j = np.arange(6, 9_003)
    check(pack(np.full(len(j), 5), j), nq, 4)               # forward: one source (a long list); reverse: every word
    i = np.arange(0, 9_001)
    check(pack(i, np.full(len(i), 39_000)), nq, 256)        # reverse: one source; K = 256, the form's largest


def test_stretches_without_edges_of_the_walked_length_one_more_and_a_million():
    nq = 2_000_000
    a = 10
    src = np.array([a, a + SEL_GAP, a + 2 * SEL_GAP + 1, a + 2 * SEL_GAP + 1 + 1_000_000])
    assert list(np.diff(src)) == [SEL_GAP, SEL_GAP + 1, 1_000_000]
    i = np.repeat(src, 3)
    j = i + np.tile([1_000, 1_001 + SEL_GAP, 1_002 + 2 * SEL_GAP + 1], len(src))     # (the same gaps on the j side)
    j[-3:] = [nq - 1 - SEL_GAP - 1, nq - 1 - SEL_GAP, nq - 1]
    check(pack(i, j), nq, 2)
    check(pack(i, j), nq + 7, 2)        # a tail of queries without edges behind the last j


def test_edges_only_at_the_first_and_only_at_the_last_query():
    nq = 300_000
    j = np.arange(1, 2_000)
    check(pack(np.zeros(len(j), dtype=np.int64), j), nq, 6)                 # forward list: query 0 alone
    i = np.arange(nq - 2_500, nq - 1)
    check(pack(i, np.full(len(i), nq - 1)), nq, 6)                          # reverse list: query nq - 1 alone
    check(pack([0], [nq - 1]), nq, 1)                                       # one pair: both at once


@pytest.mark.parametrize("case", ["mixed", "first", "last", "gaps"])
def test_reverse_only_form(case):
    """pairs = None (the sharded driver's lists: reverse words alone, src = a local query).  The oracle ranks the
    same directed edges: every neighbour id lies above the local range, so the pairs (src, neighbour) have i = src and
    the oracle's lists of the sources below nql are exactly the directed lists."""
    rng = np.random.default_rng(len(case))
    nql, ib, K = 70_000, 22, 7
    if case == "mixed":
        deg = rng.integers(0, 9, size=nql)
        deg[rng.choice(nql, 30, replace=False)] = rng.integers(70, 900, size=30)
        src = np.repeat(np.arange(nql), deg)
    elif case == "first":
        src = np.zeros(1_001, dtype=np.int64)
    elif case == "last":
        src = np.full(1_003, nql - 1)
    else:
        src = np.repeat(np.array([3, 3 + SEL_GAP, 4 + 2 * SEL_GAP, 60_000]), 5)
    dst = nql + rng.choice((1 << ib) - nql, size=len(src), replace=False)
    pairs = pack(src, dst)
    assert len(pairs) == len(src)
    milli = rng.integers(990, 1001, size=len(pairs)).astype(np.int32)
    ws, wd, wv = O.topk(pairs, milli, K)
    keep = ws < nql
    pi, pj = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
    inv = (1000 - milli.astype(np.int64)).astype(np.uint64)
    words = (pi << np.uint64(ib + 11)) | (inv << np.uint64(ib)) | pj
    words = words[rng.permutation(len(words))]
    s, d, v = (t.cpu().numpy() for t in ops.topk_select(None, None, dev(words.view(np.int64)), K, ib, nql))
    assert np.array_equal(s, ws[keep]) and np.array_equal(d, wd[keep]) and np.array_equal(v, wv[keep])


def test_offsets_over_many_workgroups_of_the_length_kernel():
    """three million queries: 733 workgroups of topk_len_kernel leave their scans and totals, the totals are scanned
    and added -- K below, at and above the typical list length"""
    rng = np.random.default_rng(5)
    nq = 3_000_001
    i, j = rng.integers(0, nq, size=4_000_000), rng.integers(0, nq, size=4_000_000)
    keep = i != j
    pairs = pack(np.minimum(i, j)[keep], np.maximum(i, j)[keep])
    for K in (1, 3, 40):
        check(pairs, nq, K, seed=K, forms=(False,))
