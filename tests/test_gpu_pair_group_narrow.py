"""The narrow form of the two-level pair grouping (qrlsh_pair_regions_scatter32 with two levels: 32-bit values and a
digit byte between the levels, four entries per load in the second) called through the C ABI with buffers the test owns:
the tmp buffer pre-filled with 0xFF bytes, guard words behind `regions` and `counts`.  Region r must hold, in any order,
exactly the values (i & gmask) << id_bits | j of the words with i >> g == r, and counts[r] their number -- with digits
narrower than a byte in both levels, with all 32 value bits and full-byte tails, with a tmp region that ends at every
place of a four-entry load, and with a tmp region beyond its capacity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
GUARD = 64
GUARD32 = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def pack(i, j):
    i, j = np.asarray(i).astype(np.uint64), np.asarray(j).astype(np.uint64)
    return (np.minimum(i, j) << np.uint64(32)) | np.maximum(i, j)


def random_words(rng, n, nids, lo=0, hi=None):
    """n words i << 32 | j with lo <= i < hi (default: anywhere), i < j < nids"""
    hi = nids - 1 if hi is None else min(hi, nids - 1)
    i = rng.integers(lo, hi, size=n)
    j = rng.integers(i + 1, nids)
    return pack(i, j)


class Shape:
    """the split of the region id and the capacities the library uses for n words"""

    def __init__(self, n, nids, g):
        lib = _lib.load()
        self.n, self.nids, self.g, self.ib = n, nids, g, ops.id_bits_for(nids)
        nr = (nids + (1 << g) - 1) >> g
        rbits = max(1, (nr - 1).bit_length())
        self.rb = rbits if rbits <= 8 else (rbits + 1) // 2
        self.ra = rbits - self.rb
        self.nreg = lib.qrlsh_pair_regions_count(n, nids, g, 0.0)
        self.cap = lib.qrlsh_pair_regions_cap(n, nids, g, 0.0)
        self.words = lib.qrlsh_pair_regions_words(n, nids, g, 0.0)
        self.twords = lib.qrlsh_pair_regions_tmp_words(n, nids, g, 0.0)
        self.na = self.nreg >> self.rb
        assert self.ra > 0 and self.twords > 0 and self.twords % self.na == 0, "two levels expected"
        assert self.words == self.nreg * self.cap
        self.cap_a = self.twords // self.na

    def fits(self, words):
        r = (words >> np.uint64(32 + self.g)).astype(np.int64)
        return (np.bincount(r).max() <= self.cap and np.bincount(r >> self.rb).max() <= self.cap_a)


def scatter(words, sh):
    """the direct call -> (region id << 32 | value of every entry, sorted; counts; overflow word); the guards behind
    regions and counts are checked here"""
    lib = _lib.load()
    n = len(words)
    wd = dev(words.view(np.int64))
    tmp = torch.full((sh.twords,), -1, dtype=torch.int64, device=DEV)                       # 0xFF bytes
    regions = torch.full((sh.words + GUARD,), GUARD32, dtype=torch.int32, device=DEV)
    counts = torch.full((sh.nreg + 256 + GUARD,), GUARD32, dtype=torch.int32, device=DEV)
    ovf = torch.full((1 + GUARD,), GUARD32, dtype=torch.int32, device=DEV)
    P, st = ops._ptr, ops._stream()
    _lib.check(lib.qrlsh_pair_regions_scatter32(P(wd), n, sh.g, sh.ib, sh.nids, 0.0, P(tmp), P(regions), P(counts), P(ovf), st))
    torch.cuda.synchronize()
    assert bool((regions[sh.words:] == GUARD32).all()), "guard behind regions"
    assert bool((counts[sh.nreg + 256:] == GUARD32).all()), "guard behind counts"
    assert bool((ovf[1:] == GUARD32).all()), "guard behind the overflow word"
    overflow = int(ovf[0].item())
    cnt = counts[:sh.nreg].to(torch.int64)
    if overflow:
        return None, cnt.cpu().numpy(), overflow
    assert int(cnt.max().item()) <= sh.cap
    held = torch.arange(sh.cap, device=DEV)[None, :] < cnt[:, None]
    vals = regions[:sh.words].view(sh.nreg, sh.cap)[held]                                   # region after region
    rid = torch.repeat_interleave(torch.arange(sh.nreg, device=DEV), cnt)
    v = vals.to(torch.int64) & 0xFFFFFFFF
    got = np.sort(((rid << 32) | v).cpu().numpy().view(np.uint64))
    return got, cnt.cpu().numpy(), overflow


def expected(words, sh):
    i, j = words >> np.uint64(32), words & np.uint64(0xFFFFFFFF)
    r = i >> np.uint64(sh.g)
    v = ((i & np.uint64((1 << sh.g) - 1)) << np.uint64(sh.ib)) | j
    assert int(v.max()) < 0xFFFFFFFF
    return np.sort((r << np.uint64(32)) | v), np.bincount(r.astype(np.int64), minlength=sh.nreg)


def check(words, sh):
    want, want_counts = expected(words, sh)
    got, counts, overflow = scatter(words, sh)
    assert overflow == 0
    assert int(counts.sum()) == len(words)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [1, 8191, 8192, 8193, 200_003])
def test_digits_narrower_than_a_byte_in_both_levels(n):
    """5 000 ids at g = 3: 625 regions, five bits of region id per level"""
    rng = np.random.default_rng(n)
    sh = Shape(n, 5_000, 3)
    assert (sh.ib, sh.ra, sh.rb, sh.na) == (13, 5, 5, 20)
    big = Shape(300_000, 5_000, 3)
    assert (big.cap_a, big.cap) == (103_936, 5_568)        # (3 * 480 + 4096 = 5 536, rounded up to a multiple of 64)
    words = random_words(rng, n, sh.nids)
    assert sh.fits(words)
    check(words, sh)


def test_all_32_value_bits_and_full_byte_tails():
    """2^24 - 1 ids at g = 8: 65 536 regions, eight bits per level, group_bits + id_bits = 32.  Region 0, the last region
    (coarse digit 255, fine digit 255) and the pair whose value is 0xFFFFFFFE are in the input"""
    rng = np.random.default_rng(2)
    nids, g = (1 << 24) - 1, 8
    top = nids - 1
    edge = pack([0, 3, 255, top - 1, top - 2, top - 255, top - 255, top - 256],
                [1, top, 256, top, top - 1, top, top - 1, top])
    words = np.concatenate([random_words(rng, 200_000, nids), random_words(rng, 500, nids, 0, 256),
                            random_words(rng, 300, nids, top - 254, top), edge, edge[:4]])
    words = words[rng.permutation(len(words))]
    sh = Shape(len(words), nids, g)
    assert (sh.ib, sh.ra, sh.rb, sh.na, sh.nreg) == (24, 8, 8, 256, 65_536)
    assert sh.fits(words)
    want, want_counts = expected(words, sh)
    assert want_counts[0] > 500 and want_counts[65_535] > 300
    assert int(want[-1]) >> 32 == 65_535
    assert np.any(want == np.uint64((65_534 << 32) | 0xFFFFFFFE))
    check(words, sh)


# (8192 +- : the tile of the first level; 10 240 +- : the tile the second level reads a tmp region in)
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 8191, 8192, 8193, 8195, 10_239, 10_240, 10_241, 10_243])
def test_the_quad_read_at_a_tmp_regions_end(c):
    """coarse region 7 (ids 1792 - 2047) receives exactly c words, the others a few hundred: with the tmp buffer full
    of 0xFF bytes an entry read beyond the count would come out as a value nobody put in"""
    rng = np.random.default_rng(100 + c)
    nids, g = 5_000, 3
    parts = [random_words(rng, c, nids, 7 * 256, 8 * 256)]
    for a in range(20):
        if a != 7:
            parts.append(random_words(rng, int(rng.integers(200, 400)), nids, a * 256, (a + 1) * 256))
    words = np.concatenate(parts)
    words = words[rng.permutation(len(words))]
    sh = Shape(len(words), nids, g)
    assert (sh.ra, sh.rb, sh.na) == (5, 5, 20)
    assert int(np.count_nonzero((words >> np.uint64(32 + g + sh.rb)) == np.uint64(7))) == c
    assert sh.fits(words)
    check(words, sh)


def test_a_tmp_region_beyond_its_capacity():
    """110 000 of 300 000 words with i < 256: coarse region 0 outgrows its 103 936 entries.  The flag is up, nothing
    is written outside the buffers, and the step groups by sorting instead"""
    rng = np.random.default_rng(4)
    nids, g, n = 5_000, 3, 300_000
    words = np.concatenate([random_words(rng, 110_000, nids, 0, 256), random_words(rng, n - 110_000, nids, 256, nids)])
    words = words[rng.permutation(n)]
    sh = Shape(n, nids, g)
    assert sh.cap_a == 103_936 and not sh.fits(words)
    got, counts, overflow = scatter(words, sh)
    assert overflow != 0 and got is None
    assert ops.region_unique_scattered(dev(words.view(np.int64)), g, sh.ib, nids) == (None, "cap")
    out = ops.unique_pairs(dev(words.view(np.int64)), nids, {})
    assert np.array_equal(u64(out), O.sort_unique(words))
