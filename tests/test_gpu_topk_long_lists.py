"""Long lists of the select form of the top-K (csrc/topk.hip: topk_select_long_kernel holds a register batch of SEL_LK
keys per lane, reads a list of up to 64 * SEL_LK entries from memory once and works a longer one in batches; the medium
and long kernels run on the auxiliary stream beside the short one) through ops.topk_select, against the oracle's top-K,
exactly: list lengths on every side of a wave's row and of the register batch, lists made of the forward run, the
reverse run and both (the reverse run ending inside a row, on a row edge and on a batch edge), K below, at and above
the list length, ties that cross the cut and the batch edge, more long lists than the grid has waves beside medium
and short ones, the reverse-only and wide-id forms, overlap on and off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from qrlsh import ops, _lib  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
WAVE = 64
LK = 16                 # keys a lane holds (SEL_LK)
BATCH = WAVE * LK       # entries a wave holds (SEL_BATCH): a list up to here is read once
LENGTHS = [64, 65, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 3]
FORK_NQ = 1 << 22       # queries from which the medium and long kernels run on the auxiliary stream (SEL_FORK_NQ)


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


def narrow(rng, n):
    """scores from a narrow range: ties cross every cut"""
    return rng.integers(996, 1001, size=n).astype(np.int32)


def select(pairs, milli, nq, K, wide=False):
    ib = ops.id_bits_for(nq)
    got = ops.topk_select(dev(pairs.view(np.int64)), dev(milli), rev_words(pairs, milli, ib, wide), K, ib, nq)
    return tuple(t.cpu().numpy() for t in got)


def check(pairs, milli, nq, K, forms=(False,)):
    """ops.topk_select on the sorted unique pairs == the oracle's top-K (src, dst and val, exactly)"""
    ws, wd, wv = O.topk(pairs, milli, K)
    for wide in forms:
        s, d, v = select(pairs, milli, nq, K, wide)
        assert np.array_equal(s, ws) and np.array_equal(d, wd) and np.array_equal(v, wv), (len(pairs), nq, K, wide)


NQ = 6000
HUB = 3000              # the query with the long list; the short lists live among the other queries


def hub_pairs(rng, nr, nf, nq=NQ, hub=HUB, short=3000):
    """one list of nr reverse + nf forward entries at `hub`, among `short` random pairs of the other queries"""
    lo = rng.choice(hub, size=nr, replace=False)
    hi = hub + 1 + rng.choice(nq - hub - 1, size=nf, replace=False)
    i, j = rng.integers(0, nq, size=short), rng.integers(0, nq, size=short)
    keep = (i != j) & (i != hub) & (j != hub)
    return np.concatenate([pack(lo, np.full(nr, hub)), pack(np.full(nf, hub), hi),
                           pack(np.minimum(i, j)[keep], np.maximum(i, j)[keep])])


def list_order(pairs, q):
    """positions (in the pairs) of q's list entries in list order: the reverse run, then the forward run"""
    pi, pj = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
    return np.concatenate([np.flatnonzero(pj == q), np.flatnonzero(pi == q)])


def compositions(n):
    """(nr, nf) of a list of n entries: forward only, reverse only, and both -- the reverse run ending inside a row
    (nr = 64 k + 17), on a row edge and on a batch edge, wherever the length has room for it"""
    nrs = [0, n, 17, WAVE, WAVE * (LK // 2) + 17, BATCH, BATCH + WAVE + 17]
    return [(nr, n - nr) for nr in dict.fromkeys(nrs) if nr <= n]


@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths_and_compositions(n):
    rng = np.random.default_rng(n)
    for nr, nf in compositions(n):
        pairs = np.unique(hub_pairs(rng, nr, nf))
        assert len(list_order(pairs, HUB)) == n
        check(pairs, narrow(rng, len(pairs)), NQ, 40)


@pytest.mark.parametrize("K", [1, 40, 256])
def test_k_below_at_and_above_the_list_length(K):
    """K = 256 is the form's largest and exceeds the lists of 65 and 200; 40 and 1 cut every list"""
    rng = np.random.default_rng(K)
    for n, nr in ((65, 17), (200, 64), (BATCH, BATCH // 2 + 17), (BATCH + 1, 17), (2 * BATCH + 3, BATCH)):
        pairs = np.unique(hub_pairs(rng, nr, n - nr))
        check(pairs, narrow(rng, len(pairs)), NQ, K)


@pytest.mark.parametrize("n", [65, BATCH, BATCH + 1, 2 * BATCH + 3])
def test_every_score_equal(n):
    """the cut falls purely by neighbour id: the first K of the list order"""
    rng = np.random.default_rng(n + 1)
    pairs = np.unique(hub_pairs(rng, n // 3, n - n // 3))
    for K in (1, 40, 256):
        check(pairs, np.full(len(pairs), 997, dtype=np.int32), NQ, K)


@pytest.mark.parametrize("edge", [WAVE, BATCH, 2 * BATCH])
def test_ties_at_the_cut_on_both_sides_of_an_edge(edge):
    """the K-th value is shared by more entries than fit, and the entries that share it lie on both sides of a row
    edge, of the batch edge and of the second batch's edge: a few better entries far from the edge, then 60 entries
    at the cut value of which the first 40 - (better ones) in list order are kept -- some before the edge, some behind"""
    rng = np.random.default_rng(edge)
    n = 2 * BATCH + 100
    for nr in (0, n, edge - 9, edge + 9):
        pairs = np.unique(hub_pairs(rng, nr, n - nr))
        milli = rng.integers(900, 990, size=len(pairs)).astype(np.int32)
        order = list_order(pairs, HUB)
        assert len(order) == n
        milli[order[edge - 30:edge + 30]] = 995                       # the ties, across the edge
        better = np.setdiff1d(np.arange(n), np.arange(edge - 30, edge + 30))
        milli[order[rng.choice(better, size=15, replace=False)]] = rng.integers(996, 1001, size=15)
        check(pairs, milli, NQ, 40)          # 15 better + the first 25 ties (positions edge - 30 .. edge - 6)
        check(pairs, milli, NQ, 50)          # ... + the first 35 ties: up to position edge + 4, behind the edge
        check(pairs, milli, NQ, 256)         # the cut far below the ties


@pytest.fixture(scope="module")
def many_lists():
    """5 200 long lists of 65 .. 80 entries (more than the long kernel's 4 096 waves: every wave takes a second list),
    2 000 medium ones and short ones, in one call: the three kernels share the output arrays"""
    rng = np.random.default_rng(9)
    nq = 400_000
    hubs = rng.choice(nq, size=7200, replace=False)
    deg = np.concatenate([rng.integers(65, 81, size=5200), rng.integers(17, 65, size=2000)])
    a = np.repeat(hubs, deg)
    b = rng.integers(0, nq, size=len(a))
    i, j = rng.integers(0, nq, size=300_000), rng.integers(0, nq, size=300_000)
    a, b = np.concatenate([a, i]), np.concatenate([b, j])
    keep = a != b
    pairs = pack(np.minimum(a, b)[keep], np.maximum(a, b)[keep])
    milli = narrow(rng, len(pairs))
    ln = np.bincount((pairs >> np.uint64(32)).astype(np.int64), minlength=nq) + \
        np.bincount((pairs & np.uint64(0xFFFFFFFF)).astype(np.int64), minlength=nq)
    assert (ln > 64).sum() >= 5000 and ((ln > 16) & (ln <= 64)).sum() >= 1000 and (ln <= 16).sum() > 100_000
    return pairs, milli, nq, O.topk(pairs, milli, 40)


def test_a_wave_that_takes_several_lists(many_lists):
    pairs, milli, nq, (ws, wd, wv) = many_lists
    s, d, v = select(pairs, milli, nq, 40)
    assert np.array_equal(s, ws) and np.array_equal(d, wd) and np.array_equal(v, wv)


def test_overlap_on_and_off(many_lists):
    """the medium and long kernels beside the short one (auxiliary stream) and behind it: the same rows.  The same
    pairs among FORK_NQ queries (the added ones have no edges): below that the library does not fork."""
    pairs, milli, nq, (ws, wd, wv) = many_lists
    assert nq < FORK_NQ
    lib = _lib.load()
    got = {}
    try:
        for ov in (1, 0):
            lib.qrlsh_set_overlap(ov)
            got[ov] = select(pairs, milli, FORK_NQ, 40)
            torch.cuda.synchronize()
    finally:
        lib.qrlsh_set_overlap(1)
    for ov in (0, 1):
        assert all(np.array_equal(x, y) for x, y in zip(got[ov], (ws, wd, wv))), ov
    assert all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))


@pytest.mark.parametrize("K", [7, 40])
def test_reverse_only_form_with_long_lists(K):
    """pairs = None: shuffled reverse words alone, so the ties to keep at the cut are the smallest ids (the by_id radix
    select, on the registers where the list fits) -- two score values only: the ties at the cut exceed the room.
    Lengths on every side of the batch, and a few hundred short lists."""
    rng = np.random.default_rng(K)
    nql, ib = 50_000, 22
    deg = rng.integers(0, 4, size=nql)
    longs = rng.choice(nql, size=10, replace=False)
    deg[longs] = [65, 70, 900, BATCH - 1, BATCH, BATCH + 1, BATCH + WAVE, 2 * BATCH - 1, 2 * BATCH + 3, 3 * BATCH + 17]
    src = np.repeat(np.arange(nql), deg)
    dst = nql + rng.choice((1 << ib) - nql, size=len(src), replace=False)
    pairs = pack(src, dst)
    assert len(pairs) == len(src)
    milli = rng.integers(999, 1001, size=len(pairs)).astype(np.int32)
    ws, wd, wv = O.topk(pairs, milli, K)
    keep = ws < nql
    pi, pj = pairs >> np.uint64(32), pairs & np.uint64(0xFFFFFFFF)
    inv = (1000 - milli.astype(np.int64)).astype(np.uint64)
    words = (pi << np.uint64(ib + 11)) | (inv << np.uint64(ib)) | pj
    words = words[rng.permutation(len(words))]
    s, d, v = (t.cpu().numpy() for t in ops.topk_select(None, None, dev(words.view(np.int64)), K, ib, nql))
    assert np.array_equal(s, ws[keep]) and np.array_equal(d, wd[keep]) and np.array_equal(v, wv[keep])


def test_wide_ids():
    """reverse words as key + payload (rdst): one long list of each kind of length, packed and wide"""
    rng = np.random.default_rng(77)
    for n, nr in ((65, 17), (BATCH + 1, WAVE * 3 + 17), (2 * BATCH + 3, BATCH)):
        pairs = np.unique(hub_pairs(rng, nr, n - nr))
        check(pairs, narrow(rng, len(pairs)), NQ, 40, forms=(False, True))
