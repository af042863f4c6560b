"""The general path on the GPU, kernel by kernel, against the numpy references of tests/sort_cases.py, bit for bit
(run with -m gpu): qrlsh_sort_u64 in every digit mode and form, qrlsh_owner_bounds, qrlsh_unique_*, qrlsh_topk_* and
qrlsh_pairs_count / fill.  Everything goes through qrlsh.ops.  tests/test_sort_host.py shows, without a GPU, that the
references are what they claim and that the range cases tell an exact sort from one whose last pass reads bits at and
above bit_hi.

Shapes: 4096-key sort tiles (1, 2, 63 .. 65, 1023 / 1025: inside one tile; 4095 .. 4097: the tile border; 8 and
9 * 4096 + 1: the tile remap with and without a remainder; 257 * 4096 + 3: more than one tile per thread of the row scan;
8193 * 4096 + 1: the 1024-thread row scan).  Rows beyond 65 536 tiles (more than 268 M keys per batch) take the chunked
loop of the row scan: out of scope here -- no test of a few seconds reaches it.  With three batches and an odd n the
second batch starts 8 bytes off a 16-byte boundary and the histogram takes its narrow loads.

A test collects every (range, form, distribution) that differs and asserts once, so that one run names all of them."""
import numpy as np
import pytest
import torch

import sort_cases as SC

pytestmark = pytest.mark.gpu

from qrlsh import ops  # noqa: E402

DEV = "cuda"
U = np.uint64
T = 4096
SIZES = [1, 2, 63, 64, 65, 1023, 1025, T - 1, T, T + 1, 8 * T, 9 * T + 1, 257 * T + 3]
DIST_SIZES = [65, T + 1, 9 * T + 1]
SENTINEL = -0x55555556        # 0xAAAAAAAA as int32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u64(t):
    return t.cpu().numpy().view(U)


def gpu_sort(keys, vals, lo, hi, **kw):
    """keys uint64 [nbatch][n] -> (sorted keys, sorted payload | None) as numpy [nbatch][n]; one batch goes in as a
    1-D tensor (the wrapper's other shape)"""
    nb, n = keys.shape
    k = dev(keys.view(np.int64))
    v = None if vals is None else dev(vals)
    if nb == 1:
        k, v = k.view(-1), (None if v is None else v.view(-1))
    ks, vs = ops.sort_u64(k, v, lo, hi, **kw)
    torch.cuda.synchronize()
    return u64(ks).reshape(nb, n), (None if vs is None else vs.cpu().numpy().reshape(nb, n))


def _kw(mode, aux):
    return dict(mix=mode == "mix", fold=aux if mode == "fold" else 0)


def check_sort(bad, tag, rng, keys, lo, hi, mode, aux, forms):
    """every form of one sort against ONE stable argsort of the field; differences are appended to `bad`"""
    nb, n = keys.shape
    order = np.stack([SC.ref_order(keys[bi], lo, hi, mode, aux) for bi in range(nb)])
    want = np.take_along_axis(keys, order, axis=1)
    for form in forms:
        if form == "keys":
            ks, vs = gpu_sort(keys, None, lo, hi, **_kw(mode, aux))
            ok = vs is None and np.array_equal(ks, want)
        elif form == "kv":
            vals = np.stack([SC.payload(rng, n) for _ in range(nb)])
            ks, vs = gpu_sort(keys, vals, lo, hi, **_kw(mode, aux))
            ok = np.array_equal(ks, want) and np.array_equal(vs, np.take_along_axis(vals, order, axis=1))
        else:   # iota: the payload is synthesised by the first pass and must come out as the permutation itself
            ks, vs = gpu_sort(keys, np.full((nb, n), SENTINEL, dtype=np.int32), lo, hi, iota=True, **_kw(mode, aux))
            ok = np.array_equal(ks, want) and np.array_equal(vs, order.astype(np.int32))
        if not ok:
            bad.append("%s [%d,%d) %s" % (tag, lo, hi, form))


def _report(bad):
    """the whole list as the assertion's message (pytest cuts a long list short)"""
    return "%d differ: %s" % (len(bad), "; ".join(bad))


def _keys(rng, nb, n, lo, hi, dist, mode="plain", aux=0):
    return np.stack([SC.make_keys(rng, n, lo, hi, dist, mode, aux) for _ in range(nb)])


# ---------------------------------------------------------------------------- sort: sizes x ranges x forms
@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_plain_sort_every_size_range_and_form(n, nbatch):
    """keys only (the staged scatter), keys + int32 payload, iota payload over one and several passes"""
    rng = np.random.default_rng(1000 * nbatch + n)
    bad = []
    for lo, hi in SC.ALL_RANGES:
        keys = _keys(rng, nbatch, n, lo, hi, "uniform")
        check_sort(bad, "plain", rng, keys, lo, hi, "plain", 0, ("keys", "kv", "iota"))
    assert not bad, _report(bad)


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_mix_sort_is_the_exact_stable_order_by_mix64_digits(n, nbatch):
    """not only "equal keys are grouped": the order the index build and append rely on.  Keys only takes
    sort_scatter_kernel<.., false, false>; iota is what ops.bucket_sort asks for"""
    rng = np.random.default_rng(2000 * nbatch + n)
    bad = []
    for lo, hi in SC.ALL_RANGES:
        keys = _keys(rng, nbatch, n, lo, hi, "uniform", "mix")
        check_sort(bad, "mix", rng, keys, lo, hi, "mix", 0, ("keys", "iota"))
    assert not bad, _report(bad)


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_fold_sort_every_width(n, nbatch):
    """pair words ordered as i << w | (j & (2^w - 1)); i carries bits above w (they reach beyond bit_hi = 2 w) and j
    carries bits above w too (they are not part of the folded word at all)"""
    rng = np.random.default_rng(3000 * nbatch + n)
    bad = []
    for w in SC.FOLD_WIDTHS:
        for lo, hi in SC.fold_ranges(w):
            keys = _keys(rng, nbatch, n, lo, hi, "uniform", "fold", w)
            if n > 64 and w < 32:
                assert (keys >> U(32 + w)).any() and ((keys & U(0xFFFFFFFF)) >> U(w)).any()
            check_sort(bad, "fold %d" % w, rng, keys, lo, hi, "fold", w, ("keys", "kv"))
    assert not bad, _report(bad)


def test_bucket_sort_is_the_mix_iota_sort_of_the_top_bits():
    rng = np.random.default_rng(5)
    n, b = 9 * T + 1, 3
    keys = rng.integers(0, 3000, size=(b, n), dtype=U) * U(0x100000001)
    for hb in (8, 16, 32):
        sk, sid = ops.bucket_sort(dev(keys.view(np.int64)), hash_bits=hb)
        order = np.stack([SC.ref_order(keys[bi], 64 - hb, 64, "mix") for bi in range(b)])
        assert np.array_equal(u64(sk), np.take_along_axis(keys, order, axis=1)), hb
        assert np.array_equal(sid.cpu().numpy(), order.astype(np.int32)), hb


# ---------------------------------------------------------------------------- sort: distributions
def _dist_params():
    for n in DIST_SIZES:
        yield "plain", 0, n
        yield "mix", 0, n
    for w in SC.FOLD_WIDTHS:
        yield "fold", w, DIST_SIZES[(w % 3)]
    yield "fold", 13, DIST_SIZES[2]


@pytest.mark.parametrize("mode,aux,n", list(_dist_params()))
def test_sort_on_every_key_distribution(mode, aux, n):
    """full 64-bit words whose field is constant / two values alternating / 0 and the maximum / ascending / descending /
    90 % one value / uniform, the bits outside the field random -- and "zero above", what today's callers pass"""
    rng = np.random.default_rng(n + 17 * aux + len(mode))
    ranges = SC.fold_ranges(aux) if mode == "fold" else SC.ALL_RANGES
    bad = []
    for dist in SC.DISTRIBUTIONS:
        for lo, hi in ranges:
            keys = _keys(rng, 3, n, lo, hi, dist, mode, aux)
            check_sort(bad, "%s %s" % (mode, dist), rng, keys, lo, hi, mode, aux, ("keys", "kv"))
            if dist == "constant":     # the sort must not move anything
                ks, _ = gpu_sort(keys, None, lo, hi, **_kw(mode, aux))
                if not np.array_equal(ks, keys):
                    bad.append("%s constant [%d,%d) moved keys" % (mode, lo, hi))
    assert not bad, _report(bad)


def test_the_wide_row_scan():
    """8193 tiles: the smallest row that sort_rowscan_kernel<1024> scans.  One 8-bit pass, keys only, one batch; the
    reference is the stable argsort of the uint8 digit"""
    n = 8193 * T + 1
    lo, hi = 13, 21
    rng = np.random.default_rng(8193)
    keys = rng.integers(0, 1 << 63, size=n, dtype=U) << U(1) | rng.integers(0, 2, size=n, dtype=U)
    k = dev(keys.view(np.int64))
    ks, vs = ops.sort_u64(k, None, lo, hi)
    torch.cuda.synchronize()
    want = keys[np.argsort(((keys >> U(lo)) & U(255)).astype(np.uint8), kind="stable")]
    assert vs is None and torch.equal(ks, dev(want.view(np.int64)))


# ---------------------------------------------------------------------------- owner and host grouping
OWNER_CASES = [(1, 0), (3, 35), (1000, 0), (1000, 33), ((1 << 32) - 1, 0), ((1 << 32) - 1, 31)]
WORLDS = [1, 2, 5, 255, 256]


@pytest.mark.parametrize("shard,lo", OWNER_CASES)
def test_owner_grouping_and_bounds(shard, lo):
    """sort_u64(owner_shard=..): one pass by (key >> lo) // shard, ranks past 255 clipped to 255 and left in input
    order.  owner_bounds: bounds[g] = first position whose owner is >= g.  That position is defined for every g <= 255
    whatever the words hold (the clipped words all satisfy it); for g = 256 it is defined only where no owner passes
    255 -- so world = 256 is checked in full on such words, and up to g = 255 on the others"""
    rng = np.random.default_rng(shard % 1000 + lo)
    bad = []
    for n in (1, 4097, 70001):
        for beyond in (True, False):
            keys = SC.owner_keys(rng, n, lo, shard, beyond=beyond)
            vals = SC.payload(rng, n)
            wk, wv = SC.ref_sort(keys, vals, lo, lo + 1, "owner", shard)
            g, gv = ops.sort_u64(dev(keys.view(np.int64)), dev(vals), bit_lo=lo, owner_shard=shard)
            g0, none = ops.sort_u64(dev(keys.view(np.int64)), None, bit_lo=lo, owner_shard=shard)
            if not (np.array_equal(u64(g), wk) and np.array_equal(gv.cpu().numpy(), wv) and none is None and torch.equal(g0, g)):
                bad.append("grouping n=%d beyond=%s" % (n, beyond))
                continue
            owner = (wk >> U(lo)) // U(shard)
            clipped = np.minimum(owner, U(255)).astype(np.int64)
            assert np.all(np.diff(clipped) >= 0)
            for world in WORLDS:
                got = ops.owner_bounds(g, lo, shard, world).cpu().numpy()
                want = np.searchsorted(clipped, np.arange(world + 1))
                upto = world + 1 if owner.max() <= 255 else min(world, 255) + 1
                if got.shape != (world + 1,) or not np.array_equal(got[:upto], want[:upto]):
                    bad.append("bounds n=%d beyond=%s world=%d" % (n, beyond, world))
    assert not bad, _report(bad)


@pytest.mark.parametrize("lo", [-1, 0, 35])
def test_owner_bounds_of_an_empty_input(lo):
    empty = torch.empty((0,), dtype=torch.int64, device=DEV)
    for world in WORLDS:
        got = ops.owner_bounds(empty, lo, 1000, world)
        assert got.shape == (world + 1,) and not got.cpu().numpy().any()
        assert ops.owner_sizes(empty, lo, 1000, world) == [0] * world


@pytest.mark.parametrize("n", [1, 4097, 70001])
def test_host_rank_grouping_and_bounds(n):
    """sort_u64(host_shard=..): pair words grouped by the rank that scores them (qr_pair_host), input order kept"""
    from dist_worker import pair_host
    rng = np.random.default_rng(n)
    nq, q0, nql, world = 100000, 40000, 20000, 5
    a = rng.integers(q0, q0 + nql, size=n).astype(U)
    c = rng.integers(0, nq, size=n).astype(U)
    c[c == a] += U(1)
    pairs = (np.minimum(a, c) << U(32)) | np.maximum(a, c)
    vals = SC.payload(rng, n)
    wk, wv = SC.ref_sort(pairs, vals, 0, 1, "host", nql)
    g, gv = ops.sort_u64(dev(pairs.view(np.int64)), dev(vals), host_shard=nql)
    assert np.array_equal(u64(g), wk) and np.array_equal(gv.cpu().numpy(), wv)
    g0, _ = ops.sort_u64(dev(pairs.view(np.int64)), None, host_shard=nql)
    assert torch.equal(g0, g)
    host = pair_host(wk, nql)
    assert np.all(np.diff(host) >= 0)
    assert np.array_equal(ops.owner_bounds(g, -1, nql, world).cpu().numpy(), np.searchsorted(host, np.arange(world + 1)))
    # shards of 300 ids: ranks 0 .. 333, those past 255 clipped
    wk2, _ = SC.ref_sort(pairs, None, 0, 1, "host", 300)
    g2, _ = ops.sort_u64(dev(pairs.view(np.int64)), None, host_shard=300)
    assert np.array_equal(u64(g2), wk2)
    clipped = np.minimum(pair_host(wk2, 300), 255)
    for w2 in (2, 255):
        assert np.array_equal(ops.owner_bounds(g2, -1, 300, w2).cpu().numpy(), np.searchsorted(clipped, np.arange(w2 + 1)))


# ---------------------------------------------------------------------------- unique compaction
@pytest.mark.parametrize("n", [0, 1, 2, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 1, 70001])
def test_unique_sorted_equals_numpy_unique(n):
    rng = np.random.default_rng(n)
    bad = []
    for name, a in SC.unique_inputs(rng, n).items():
        got = ops.unique_sorted(dev(a.view(np.int64)))
        if got.dtype != torch.int64 or not np.array_equal(u64(got), np.unique(a)):
            bad.append(name)
    assert not bad, _report(bad)


# ---------------------------------------------------------------------------- top-K compaction
CMP_TILE = SC.CMP_TILE


def _straddlers(degrees, K):
    """sources with more than K edges whose run crosses a border of the compaction's 2048-word tiles"""
    end = np.cumsum(degrees)
    start = end - degrees
    return [q for q in range(len(degrees)) if degrees[q] > K and start[q] // CMP_TILE != (end[q] - 1) // CMP_TILE]


@pytest.mark.parametrize("K", [1, 5, 3000])
def test_topk_edges_equals_the_lexsort_cut(K):
    """ops.topk_edges (stable sort on (src, 1000 - value), then keep an edge iff a[t - K] is of another source): K = 1;
    a source with more than K edges across a tile border; K = 3000, more than a tile, so that a[t - K] is read from an
    earlier tile -- and sources of exactly K and K + 1 edges"""
    rng = np.random.default_rng(K)
    if K == 3000:
        ib = 14
        degrees = np.array([5, 3000, 3001, 7000, 1, 2999, 4500, 0, 2, 10000, 3000])
    else:
        ib = 12
        degrees = rng.integers(0, 2 * K + 8, size=2500)
        degrees[[3, 77, 1200]] = (K, K + 1, 2500)
    assert len(_straddlers(degrees, K)) >= 3 and (degrees == K).any() and (degrees == K + 1).any()
    keys, src, dst, inv = SC.topk_case(rng, ib, degrees)
    ws, wd, wv = SC.ref_topk(src, dst, inv, K)
    s, d, v = (t.cpu().numpy() for t in ops.topk_edges(dev(keys.view(np.int64)), K, ib))
    assert len(s) == int(np.minimum(degrees, K).sum())
    assert np.array_equal(s, ws) and np.array_equal(d, wd) and np.array_equal(v, wv)


# ---------------------------------------------------------------------------- general pair emit
_EMIT = {}


def _emit_case(nq, r):
    """keys and reference of one shape, built once and shared by the hash widths (never modified)"""
    if (nq, r) not in _EMIT:
        rng = np.random.default_rng(100 * nq + r)
        if nq >= 50000:
            keys = SC.emit_case(rng, nq, 2, 5000, r, planted=(300, 1500))
        else:
            keys = SC.emit_case(rng, nq, 2, 3, r, planted=())
        keys.setflags(write=False)
        _EMIT[(nq, r)] = (keys, SC.ref_emit_pairs(keys, r))
    return _EMIT[(nq, r)]


def _gpu_emit(keys, r, hb):
    sk, sid = ops.bucket_sort(dev(keys.view(np.int64).copy()), hb)      # the shared keys stay read-only
    out = ops.emit_pairs(sk, sid, r, hb)
    torch.cuda.synchronize()
    return np.sort(u64(out))


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("hash_bits", [8, 16, 32])
def test_general_pair_emit_equals_the_group_reference(hash_bits, r):
    """50 000 queries x 2 bands over ~5000 keys: at hash_bits = 8 a hash run is ~200 records of ~20 interleaved keys
    and passes the 128-record halo into the global-memory walk; a 300-copy and a 1500-copy key cross the 1024-record
    tile borders; key 0 (mix64(0) = 0: the very first records of band 0, next to the zero-filled halo of tile 0); a
    third of band 1 is the empty key"""
    keys, want = _emit_case(50000, r)
    assert np.count_nonzero(keys[0] == 0) == 4 and np.count_nonzero(keys[1] == U(SC.empty_key(r))) >= 50000 // 3
    got = _gpu_emit(keys, r, hash_bits)
    assert got.size == want.size and np.array_equal(got, want)


@pytest.mark.parametrize("nq", [1, 2, 1023, 1024, 1025])
def test_general_pair_emit_small_shapes(nq):
    keys, want = _emit_case(nq, 2)
    for hb in (8, 16, 32):
        got = _gpu_emit(keys, 2, hb)
        assert got.size == want.size and np.array_equal(got, want), hb
