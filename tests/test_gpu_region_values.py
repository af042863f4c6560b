"""The fixed-region de-duplication (regions of 32-bit values: qrlsh_pair_regions_scatter32 +
qrlsh_region_unique_count_regions32, with ONE three-word read-back): its unique pairs against the oracle's sorted unique
words -- at the empty-marker boundary (2^24 - 1 and 2^24 ids at g = 8), with ids too wide for the value, with one
grouping level, and with a region filled to its capacity and one word beyond."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def pack(i, j):
    i, j = np.asarray(i).astype(np.uint64), np.asarray(j).astype(np.uint64)
    return (np.minimum(i, j) << np.uint64(32)) | np.maximum(i, j)


def random_words(rng, n, nids, dup=3):
    """n emitted words i << 32 | j, i < j < nids, every distinct pair about `dup` times, any order"""
    m = max(1, n // dup)
    i, j = rng.integers(0, nids, size=m), rng.integers(0, nids, size=m)
    w = pack(i, j)[i != j]
    return w[rng.integers(0, len(w), size=n)]


def scattered(words, g, ib, nids, wpq=0.0):
    """-> the unique pairs of the fixed-region form, after checking them against the oracle"""
    want = O.sort_unique(words)
    got, why = ops.region_unique_scattered(dev(words.view(np.int64)), g, ib, nids, wpq)
    assert why == "", why
    assert np.array_equal(u64(got), want)
    return got


def test_largest_value_beside_the_empty_marker():
    """2^24 - 1 ids at g = 8: group_bits + id_bits = 32 and the largest value, (255, 2^24 - 2) of the pair
    (2^24 - 257, 2^24 - 2), is 0xFFFFFFFE -- one below the marker of an empty slot.  The last region, that pair and the
    largest pair of all are in the input."""
    rng = np.random.default_rng(1)
    nids, g, ib = (1 << 24) - 1, 8, 24
    assert ops.id_bits_for(nids) == ib and ops.region_values_fit(g, ib, nids)
    top = nids - 1
    edge = pack([top - 1, top - 1, top - 255, 0, 255, 256, top - 256], [top, top, top, top, top, top, top - 1])
    words = np.concatenate([random_words(rng, 2_000_000, nids), edge, edge[:3]])
    words = words[rng.permutation(len(words))]
    got = scattered(words, g, ib, nids)
    assert int(u64(got)[-1]) == ((top - 1) << 32 | top)
    st = {}
    out = ops.unique_pairs(dev(words.view(np.int64)), nids, st)
    assert st["dedup_path"] == "regions-in-lds (scattered)" and st["group_bits"] == 8, st
    assert np.array_equal(u64(out), O.sort_unique(words))


def test_two_to_the_24_ids_leave_no_spare_value_at_g_8():
    """2^24 ids: (255, 2^24 - 1) would BE the marker, so g = 8 is refused -- by ops and by both library calls, before
    any device work -- and the step groups by 7 bits"""
    lib = _lib.load()
    rng = np.random.default_rng(2)
    nids, ib = 1 << 24, 24
    assert ops.id_bits_for(nids) == ib
    assert not ops.region_values_fit(8, ib, nids) and ops.region_values_fit(7, ib, nids)
    top = nids - 1
    words = np.concatenate([random_words(rng, 1_000_000, nids), pack([top - 1, 0, top - 255], [top, top, top])])
    with pytest.raises(ValueError):
        ops.region_unique_scattered(dev(words.view(np.int64)), 8, ib, nids)
    # the library's own refusal: both calls check before any device work, so dummy non-null pointers do
    p, n = 64, len(words)
    assert lib.qrlsh_pair_regions_scatter32(p, n, 8, ib, nids, 0.0, p, p, p, p, None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_region_unique_count_regions32(p, p, 4096, n, 8, ib, nids, p, p, 1 << 30, p, p, None) == _lib.QRLSH_EINVAL
    assert ops.region_group_bits(ib, nids, len(words) / nids) == 7
    st = {}
    out = ops.unique_pairs(dev(words.view(np.int64)), nids, st)
    assert st["group_bits"] == 7, st
    assert np.array_equal(u64(out), O.sort_unique(words))


def test_ids_of_25_bits_do_not_take_the_value_form_at_g_8():
    rng = np.random.default_rng(3)
    nids, ib = (1 << 25) - 1, 25
    assert ops.id_bits_for(nids) == ib and not ops.region_values_fit(8, ib, nids)
    words = random_words(rng, 500_000, nids)
    with pytest.raises(ValueError):
        ops.region_unique_scattered(dev(words.view(np.int64)), 8, ib, nids)
    # what the step does with such ids: 7 group bits are 2^18 regions, more than two levels of 256 digits reach --
    # the grouping is not served and the words are grouped by sorting, with the same result
    g = ops.region_group_bits(ib, nids, len(words) / nids)
    assert g == 7
    assert ops.region_unique_scattered(dev(words.view(np.int64)), g, ib, nids) == (None, "cap")
    out = ops.unique_pairs(dev(words.view(np.int64)), nids, {})
    assert np.array_equal(u64(out), O.sort_unique(words))


@pytest.mark.parametrize("nids,g", [(50_000, 8), (65_536, 8), (9_000, 6), (300, 3)])
def test_one_grouping_level(nids, g):
    """at most 256 regions: the only level writes the values"""
    lib = _lib.load()
    rng = np.random.default_rng(nids)
    ib = ops.id_bits_for(nids)
    words = random_words(rng, 300_000, nids, dup=5)
    assert lib.qrlsh_pair_regions_tmp_words(len(words), nids, g, 0.0) == 0
    assert lib.qrlsh_pair_regions_count(len(words), nids, g, 0.0) <= 256
    scattered(words, g, ib, nids)


def test_two_grouping_levels_and_popular_queries():
    """3 M ids at g = 8 (11 719 regions: two levels), regions sized to 6 400 words.  One query with ~5 400 distinct partners
    (with its region's ordinary words more than the main finish holds: the big-image kernel), two with ~1 500 emitted
    twice (popular rows of the main finish) -- each region still within its capacity"""
    lib = _lib.load()
    rng = np.random.default_rng(4)
    nids, g = 3_000_000, 8
    ib = ops.id_bits_for(nids)
    big = pack(np.full(5_400, 5), rng.choice(np.arange(6, nids), size=5_400, replace=False))
    hot = np.concatenate([pack(np.full(1_500, q), rng.integers(q + 1, nids, size=1_500)) for q in (70_000, 2_990_000)])
    words = np.concatenate([random_words(rng, 3_000_000, nids), big, hot, hot])
    words = words[rng.permutation(len(words))]
    wpq = 3.0         # (a hint above the true ~1 word per query: regions of 3 * 256 * 3 + 4096 = 6 400 words)
    assert lib.qrlsh_pair_regions_tmp_words(len(words), nids, g, wpq) > 0
    per_region = np.bincount((words >> np.uint64(32 + g)).astype(np.int64))
    assert per_region.max() <= lib.qrlsh_pair_regions_cap(len(words), nids, g, wpq)
    assert len(np.unique(words[(words >> np.uint64(32 + g)) == np.uint64(0)])) > 5_400
    scattered(words, g, ib, nids, wpq=wpq)


def test_a_region_at_its_capacity_and_one_word_beyond():
    """region 3 of a one-level grouping receives exactly its capacity in words (it is served), then one word
    more ("cap" through the one read-back, never a wrong list)"""
    lib = _lib.load()
    rng = np.random.default_rng(6)
    nids, g, n = 50_000, 8, 200_000
    ib = ops.id_bits_for(nids)
    cap = lib.qrlsh_pair_regions_cap(n, nids, g, 0.0)
    assert 4096 < cap < n // 2
    for extra in (0, 1):
        m = cap + extra
        i = rng.integers(3 << g, 4 << g, size=m)
        j = rng.integers(4 << g, 4 << g | 15, size=m)               # few distinct pairs: the finish's set is not the limit
        rest = random_words(rng, n, nids)
        rest = rest[(rest >> np.uint64(32 + g)) != np.uint64(3)][:n - m]
        words = np.concatenate([pack(i, j), rest])
        assert len(words) == n and int(np.count_nonzero((words >> np.uint64(32 + g)) == np.uint64(3))) == m
        words = words[rng.permutation(n)]
        if extra == 0:
            scattered(words, g, ib, nids)
        else:
            assert ops.region_unique_scattered(dev(words.view(np.int64)), g, ib, nids) == (None, "cap")


def test_more_distinct_pairs_than_the_finish_holds_is_reported_in_the_same_read_back():
    rng = np.random.default_rng(7)
    nids, g = 1 << 20, 8
    ib = ops.id_bits_for(nids - 1)
    one = pack(np.full(60_000, 1500), rng.integers(1501, nids, size=60_000))      # ~58 000 distinct partners of one query
    words = np.concatenate([random_words(rng, 400_000, nids - 1), one])
    words = words[rng.permutation(len(words))]
    got = ops.region_unique_scattered(dev(words.view(np.int64)), g, ib, nids - 1, len(words) / 3000)
    assert got == (None, "distinct") or got == (None, "cap")
    out = ops.unique_pairs(dev(words.view(np.int64)), nids - 1, {})
    assert np.array_equal(u64(out), O.sort_unique(words))
