"""What tests/test_gpu_sort.py rests on, in numpy (tests/sort_cases.py).  No GPU.

1. The reference of every sort case -- one stable argsort of the whole field -- is what a pass-by-pass LSD sort gives
   when the last pass keeps only the bits below bit_hi.
2. The cases discriminate: wherever the last digit is partial and the word has bits above it, a last pass that takes
   the whole byte (digit_of before the range was made exact) orders the keys differently, on every distribution but
   "zero above" (a constant field included: its keys must stay where they are, and the bits above would move them)
   -- and on "zero above", what every caller in ops.py passes, it does not.
3. ref_emit_pairs is the oracle's candidate set, band repeats aside."""
import numpy as np
import pytest

import sort_cases as SC
from oracle import oracle as O

N_HOST = 1025     # enough keys that two orders of a 1-bit field differ; one more than a multiple of everything


def _modes():
    for lo, hi in SC.ALL_RANGES:
        yield "plain", 0, lo, hi
        yield "mix", 0, lo, hi
    for w in SC.FOLD_WIDTHS:
        for lo, hi in SC.fold_ranges(w):
            yield "fold", w, lo, hi


MODES = list(_modes())


def _seed(*parts):
    return sum((i + 1) * 7919 * int(p) for i, p in enumerate(parts))


def test_mix64_inverse():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 63, size=4096, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=4096, dtype=np.uint64)
    x[:3] = (0, 1, SC.M64)
    assert np.array_equal(SC.np_mix64(SC.np_unmix64(x)), x)
    assert np.array_equal(SC.np_unmix64(SC.np_mix64(x)), x)


@pytest.mark.parametrize("mode,aux,lo,hi", MODES)
def test_reference_equals_masked_lsd_passes(mode, aux, lo, hi):
    for di, dist in enumerate(SC.DISTRIBUTIONS):
        rng = np.random.default_rng(_seed(lo, hi, aux, di, len(mode)))
        keys = SC.make_keys(rng, N_HOST, lo, hi, dist, mode, aux)
        vals = SC.payload(rng, N_HOST)
        order = SC.ref_order(keys, lo, hi, mode, aux)
        assert np.array_equal(order, SC.lsd_order(keys, lo, hi, mode, aux, masked=True)), dist
        rk, rv = SC.ref_sort(keys, vals, lo, hi, mode, aux)
        assert np.array_equal(rk, keys[order]) and np.array_equal(rv, vals[order])
        f = SC.field_of(rk, lo, hi, mode, aux)
        assert np.all(f[1:] >= f[:-1])
        if dist == "constant":
            assert np.array_equal(order, np.arange(N_HOST))         # a constant field: the input order


@pytest.mark.parametrize("mode,aux,lo,hi", MODES)
def test_cases_tell_an_unmasked_last_pass_from_the_field_sort(mode, aux, lo, hi):
    shows = SC.range_shows_bits_above(lo, hi, mode, aux)
    for di, dist in enumerate(SC.DISTRIBUTIONS):
        rng = np.random.default_rng(_seed(lo, hi, aux, di, len(mode)) + 1)
        keys = SC.make_keys(rng, N_HOST, lo, hi, dist, mode, aux)
        same = np.array_equal(SC.ref_order(keys, lo, hi, mode, aux), SC.lsd_order(keys, lo, hi, mode, aux, masked=False))
        if shows and dist != "zero_above":
            # (the constant field too: the field sort leaves the input order, the unmasked pass orders by the bits above)
            assert not same, "%s: an unmasked last pass would go unnoticed" % dist
        else:
            assert same, dist      # today's callers, whole-byte ranges, ranges that end at the top of the word


def test_the_issue_ranges_with_a_partial_last_digit_all_show_bits_above():
    partial = [(lo, hi) for lo, hi in SC.ALL_RANGES if (hi - lo) % 8]
    assert set(partial) == {(57, 64), (0, 1), (11, 12), (0, 20), (3, 16), (32, 45), (5, 38), (9, 29)}
    # [57, 64) ends at bit 64: no bit above it exists, the unmasked digit is the field
    assert [r for r in partial if not SC.range_shows_bits_above(*r)] == [(57, 64)]
    for w in SC.FOLD_WIDTHS:
        assert SC.range_shows_bits_above(0, 2 * w, "fold", w) == (w % 4 != 0)
    # every width of the list is also reached from a bit_lo that is no multiple of 8 (64 bits start at 0 only)
    for wd in {hi - lo for lo, hi in SC.RANGES} - {64}:
        assert any(hi - lo == wd and lo % 8 for lo, hi in SC.ALL_RANGES), wd


@pytest.mark.parametrize("shard,lo", [(1, 0), (3, 35), (1000, 0), (1000, 33), ((1 << 32) - 1, 0), ((1 << 32) - 1, 31)])
def test_owner_field_clips_and_keeps_input_order(shard, lo):
    rng = np.random.default_rng(shard % 1000 + lo)
    keys = SC.owner_keys(rng, 5000, lo, shard)
    owner = (keys >> np.uint64(lo)) // np.uint64(shard)
    f = SC.field_of(keys, lo, lo + 1, "owner", shard)
    assert f.max() <= 255 and np.array_equal(f, np.minimum(owner, 255))
    if shard < (1 << 32) - 1:
        assert owner.max() > 255 and len(np.unique(owner[owner >= 255])) > 1     # clipped ranks of several owners
    else:
        assert len(np.unique(owner)) > 1
    order = SC.ref_order(keys, lo, lo + 1, "owner", shard)
    assert np.array_equal(order, SC.lsd_order(keys, lo, lo + 1, "owner", shard))
    clipped = order[f[order] == 255]
    assert np.all(np.diff(clipped) > 0)


def test_host_field_is_pair_host():
    from dist_worker import pair_host
    rng = np.random.default_rng(5)
    i = rng.integers(0, 70000, size=3000).astype(np.uint64)
    j = rng.integers(0, 70000, size=3000).astype(np.uint64)
    pairs = (np.minimum(i, j) << np.uint64(32)) | (np.maximum(i, j) + np.uint64(1))
    assert np.array_equal(SC.field_of(pairs, 0, 1, "host", 100), np.minimum(pair_host(pairs, 100), 255).astype(np.uint64))
    assert SC.field_of(pairs, 0, 1, "host", 100).max() == 255


@pytest.mark.parametrize("nq,b,nkeys,r", [(300, 3, 40, 2), (2000, 2, 150, 4)])
def test_ref_emit_pairs_is_the_oracle_candidate_set(nq, b, nkeys, r):
    rng = np.random.default_rng(nq)
    keys = SC.emit_case(rng, nq, b, nkeys, r, planted=(35, 120))
    assert np.count_nonzero(keys[1] == np.uint64(SC.empty_key(r))) >= nq // 3 and np.count_nonzero(keys[0] == 0) >= 2
    got = SC.ref_emit_pairs(keys, r)
    assert np.all(got[1:] >= got[:-1]) and np.all((got >> np.uint64(32)) < (got & np.uint64(0xFFFFFFFF)))
    # one word per band a pair collides in: as many words as the oracle counts, the oracle's set once repeats are dropped
    assert len(got) == O.emitted_pairs(np.ascontiguousarray(keys.T), r)
    assert len(np.unique(got)) < len(got)
    assert np.array_equal(np.unique(got), O.candidates(np.ascontiguousarray(keys.T), r))
    # brute force on the first band
    row = keys[0]
    want = sorted((a << 32) | c for a in range(nq) for c in range(a + 1, nq)
                  if row[a] == row[c] and int(row[a]) != SC.empty_key(r))
    assert np.array_equal(SC.ref_emit_pairs(keys[:1], r), np.array(want, dtype=np.uint64))


def test_ref_emit_pairs_degenerate():
    assert SC.ref_emit_pairs(np.zeros((2, 0), dtype=np.uint64), 2).size == 0
    assert SC.ref_emit_pairs(np.zeros((2, 1), dtype=np.uint64), 2).size == 0
    assert SC.ref_emit_pairs(np.full((1, 5), SC.empty_key(2), dtype=np.uint64), 2).size == 0
    assert SC.ref_emit_pairs(np.full((1, 5), SC.empty_key(2), dtype=np.uint64), 4).size == 10     # not the r = 4 empty key
    assert SC.ref_emit_pairs(np.zeros((2, 2), dtype=np.uint64), 4).tolist() == [1, 1]


def test_unique_inputs_are_sorted_and_put_runs_on_the_borders():
    rng = np.random.default_rng(2)
    for n in (0, 1, 2, 511, 512, 513, 2049, 3 * 2048 + 1):
        cases = SC.unique_inputs(rng, n)
        if n > 2048:
            starts = lambda a: set(np.r_[0, np.flatnonzero(a[1:] != a[:-1]) + 1].tolist())
            assert starts(cases["runs_on_slices"]) == set(range(0, n, 512))
            assert starts(cases["runs_on_tiles"]) == set(range(0, n, 2048))
            assert {x for x in (511, 513, 2047, 2049) if x < n} <= starts(cases["runs_around_borders"])
            assert {x for x in (512, 513, 2048, 2049) if x < n} <= starts(cases["single_at_borders"])
            assert any(int(a[-1]) >> 63 for a in cases.values())


def test_topk_reference_cut():
    rng = np.random.default_rng(4)
    keys, src, dst, inv = SC.topk_case(rng, 12, [0, 5, 1, 9, 3])
    assert np.array_equal(keys >> np.uint64(23), src.astype(np.uint64)) and np.all(np.diff(dst) >= 0)
    s, d, v = SC.ref_topk(src, dst, inv, 3)
    assert np.bincount(s, minlength=5).tolist() == [0, 3, 1, 3, 3]
    for q in (1, 3, 4):
        mine = sorted(zip(inv[src == q].tolist(), dst[src == q].tolist()))[:3]
        assert [(1000 - a, c) for a, c in mine] == list(zip(v[s == q].tolist(), d[s == q].tolist()))
