"""References and input builders for the general path: qrlsh_sort_u64 in every digit mode, qrlsh_owner_bounds,
qrlsh_pairs_count / fill, qrlsh_unique_* and qrlsh_topk_* (csrc/sort.hip, csrc/pairs.hip).  Shared by
tests/test_sort_host.py (numpy against numpy: the references are what they claim, and the cases can tell a sort that
honours bit_hi from one that does not) and tests/test_gpu_sort.py (the kernels against the references, bit for bit).

The reference of a sort is ONE stable argsort of the whole field -- by definition what a stable LSD radix sort over that
field must produce.  `lsd_sort` is the pass-by-pass restatement of the kernels (8 bits per pass); with masked=False
its last pass takes a whole byte, the bits at and above bit_hi included, as digit_of did before the range was made
exact.  Pure numpy: nothing here needs the library, torch or a GPU (`pair_host`, the twin of qr_pair_host, is fetched
from dist_worker only when the host mode is asked for)."""
import numpy as np

from bucket_cases import np_mix64

U = np.uint64
M64 = (1 << 64) - 1

# the ranges of the sort tests: whole word, whole bytes, ranges ending at bit 64, and ranges whose width is no
# multiple of 8 bits (the last pass is a partial digit) ...
RANGES = [(0, 64), (8, 16), (40, 64), (57, 64), (0, 1), (11, 12), (0, 20), (3, 16), (32, 45), (5, 38)]
# ... and, so that every width is also reached from a bit_lo that is no multiple of 8: 8, 24 and 20 bits
# (1, 7, 13 and 33 bits are above; 64 bits can only start at bit 0)
RANGES_UNALIGNED = [(13, 21), (35, 59), (9, 29)]
ALL_RANGES = RANGES + RANGES_UNALIGNED

FOLD_WIDTHS = [1, 5, 13, 20, 27, 32]

DISTRIBUTIONS = ["uniform", "constant", "alternating", "extremes", "ascending", "descending", "skewed", "zero_above"]


def fold_ranges(w):
    """ranges of the folded word i << w | j (32 + w bits): what sort_pairs passes, and one that starts inside j"""
    return [(0, 2 * w), (3, min(32 + w, w + 10))]


# ------------------------------------------------------------------------------------------------ digit sources
def _inv_xorshift(z, s):
    out = z.copy()
    for _ in range(64 // s + 1):
        out = z ^ (out >> U(s))
    return out


def np_unmix64(x):
    """inverse of np_mix64 (the splitmix64 finaliser is a bijection): the key whose mix64 is x"""
    z = np.asarray(x).astype(U)
    with np.errstate(over="ignore"):
        z = _inv_xorshift(z, 31) * U(pow(0x94D049BB133111EB, -1, 1 << 64))
        z = _inv_xorshift(z, 27) * U(pow(0xBF58476D1CE4E5B9, -1, 1 << 64))
    return _inv_xorshift(z, 30)


def fold_word(keys, w):
    """the word the fold mode takes its digits from: i << w | (j & (2^w - 1)) of key = i << 32 | j"""
    keys = np.asarray(keys).astype(U)
    return ((keys >> U(32)) << U(w)) | (keys & U((1 << w) - 1))


def digit_source(keys, mode, aux=0):
    """x of the plain / mix / fold modes: the word whose bits [lo, hi) order the keys"""
    keys = np.asarray(keys).astype(U)
    if mode == "plain":
        return keys
    if mode == "mix":
        return np_mix64(keys)
    if mode == "fold":
        return fold_word(keys, aux)
    raise ValueError(mode)


def source_bits(mode, aux=0):
    """bits x can have"""
    return 32 + aux if mode == "fold" else 64


def field_of(keys, lo, hi, mode, aux=0):
    """what the sort orders by (uint64): bits [lo, hi) of x, masked to hi - lo bits; owner / host: the rank, 255 at most"""
    keys = np.asarray(keys).astype(U)
    if mode == "owner":
        return np.minimum((keys >> U(lo)) // U(aux), U(255))
    if mode == "host":
        from dist_worker import pair_host
        return np.minimum(pair_host(keys, aux).astype(U), U(255))
    f = digit_source(keys, mode, aux) >> U(lo)
    if hi - lo < 64:
        f = f & U((1 << (hi - lo)) - 1)
    return f


def _narrow(f, bits):
    """the field in the narrowest unsigned type that holds it (numpy's stable sort of 8- and 16-bit integers is a
    counting sort: the big cases stay cheap)"""
    return f.astype(np.uint8 if bits <= 8 else np.uint16 if bits <= 16 else np.uint32 if bits <= 32 else U)


def ref_order(keys, lo, hi, mode="plain", aux=0):
    """the permutation a stable sort over the field gives: out[t] = in[order[t]]"""
    bits = 8 if mode in ("owner", "host") else hi - lo
    return np.argsort(_narrow(field_of(keys, lo, hi, mode, aux), bits), kind="stable")


def ref_sort(keys, vals, lo, hi, mode="plain", aux=0):
    """keys (uint64 [n]) and payload (or None) in the order of ONE stable sort of the whole field"""
    keys = np.asarray(keys).astype(U)
    o = ref_order(keys, lo, hi, mode, aux)
    return keys[o], (None if vals is None else np.asarray(vals)[o])


def lsd_order(keys, lo, hi, mode="plain", aux=0, masked=True):
    """the kernels' way, pass by pass: 8 bits per pass from bit lo up; the last pass keeps min(8, hi - shift) bits of
    its digit when masked, a whole byte -- bits at and above hi included -- when not"""
    keys = np.asarray(keys).astype(U)
    order = np.arange(len(keys))
    if mode in ("owner", "host"):
        return order[np.argsort(field_of(keys, lo, hi, mode, aux).astype(np.uint8), kind="stable")]
    x = digit_source(keys, mode, aux)
    for shift in range(lo, hi, 8):
        keep = min(8, hi - shift) if masked else 8
        d = ((x[order] >> U(shift)) & U((1 << keep) - 1)).astype(np.uint8)
        order = order[np.argsort(d, kind="stable")]
    return order


def range_shows_bits_above(lo, hi, mode="plain", aux=0):
    """does an unmasked last pass see bits that are not of the field?  (a partial last digit, and bits above it exist)"""
    return (hi - lo) % 8 != 0 and hi < source_bits(mode, aux)


# ------------------------------------------------------------------------------------------------ key distributions
def make_keys(rng, n, lo, hi, dist, mode="plain", aux=0):
    """n keys (uint64) whose FIELD -- bits [lo, hi) of the mode's x -- follows `dist`; every other bit of x is random
    (zero_above: the bits at and above hi are zero, as every caller in ops.py has them), and so are the bits of a
    folded key that x does not hold (j's bits from w up)."""
    wd = hi - lo
    top = (1 << wd) - 1
    x = rng.integers(0, 1 << 63, size=n, dtype=U) << U(1) | rng.integers(0, 2, size=n, dtype=U)
    if dist == "uniform" or dist == "zero_above":
        f = None
    elif dist == "constant":
        f = np.full(n, int(rng.integers(0, top + 1, dtype=U)), dtype=U)
    elif dist == "alternating":
        a = int(rng.integers(0, top + 1, dtype=U))
        b = (a + 1 + int(rng.integers(0, top, dtype=U))) % (top + 1) if top > 1 else 1 - a
        f = np.where(np.arange(n) % 2 == 0, U(a), U(b))
    elif dist == "extremes":
        f = np.where(rng.integers(0, 2, size=n) == 0, U(0), U(top))
    elif dist in ("ascending", "descending"):
        f = np.sort(_field_draw(rng, n, wd))
        if dist == "descending":
            f = f[::-1].copy()
    elif dist == "skewed":
        f = _field_draw(rng, n, wd)
        f[rng.random(n) < 0.9] = U(int(rng.integers(0, top + 1, dtype=U)))
    else:
        raise ValueError(dist)
    if f is not None:
        fmask = U((top << lo) & M64)
        x = (x & ~fmask) | (f.astype(U) << U(lo))
    if dist == "zero_above" and hi < 64:
        x = x & U((1 << hi) - 1)
    if mode == "plain":
        return x
    if mode == "mix":
        return np_unmix64(x)
    if mode == "fold":
        w = aux
        x = x & U((1 << (32 + w)) - 1)
        junk = rng.integers(0, 1 << 32, size=n, dtype=U) & U(~((1 << w) - 1) & 0xFFFFFFFF)   # j's bits above w
        if dist == "zero_above":
            junk = junk * U(0)
        return ((x >> U(w)) << U(32)) | (x & U((1 << w) - 1)) | junk
    raise ValueError(mode)


def _field_draw(rng, n, wd):
    if wd >= 64:
        return rng.integers(0, 1 << 63, size=n, dtype=U) << U(1) | rng.integers(0, 2, size=n, dtype=U)
    return rng.integers(0, 1 << wd, size=n, dtype=U)


def payload(rng, n):
    """arbitrary int32 payload, negative values included"""
    return rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32)


def owner_keys(rng, n, lo, shard, beyond=True):
    """words whose id field (from bit lo up) lands on ranks 0 .. 255 and, with `beyond`, on ranks past 255 too (those
    are clipped to 255 and keep their input order); the bits below lo are random"""
    span = min(shard * (400 if beyond else 256), 1 << (64 - lo))
    ids = (rng.random(n) * span).astype(U)
    ids[rng.random(n) < 0.05] = U(0)
    if beyond and span > shard * 256:
        ids[rng.random(n) < 0.1] = U(min(span - 1, shard * 256 + 1))
    low = rng.integers(0, 1 << lo, size=n, dtype=U) if lo else np.zeros(n, dtype=U)
    return (ids << U(lo)) | low


# ------------------------------------------------------------------------------------------------ pair emit
def empty_key(r):
    """qr_empty_key (csrc/common.h): the key of a band whose r values are all -1"""
    return M64 if r >= 4 else (1 << (16 * r)) - 1


def ref_emit_pairs(keys, r):
    """keys uint64 [b][nq] -> every (i < j) pair of every group of equal keys of every band, except the groups of
    empty_key(r), as sorted uint64 i << 32 | j; a pair that collides in several bands appears once per band.
    Groups are worked size by size: all groups of s members at once, through the s (s - 1) / 2 index pairs."""
    keys = np.asarray(keys).astype(U)
    ek = U(empty_key(r))
    out = []
    for row in keys:
        order = np.argsort(row, kind="stable")       # ids ascend inside a group
        sk = row[order]
        n = len(sk)
        if n == 0:
            continue
        first = np.r_[0, np.flatnonzero(sk[1:] != sk[:-1]) + 1]
        size = np.diff(np.r_[first, n])
        live = (size > 1) & (sk[first] != ek)
        first, size = first[live], size[live]
        for s in np.unique(size):
            at = first[size == s]
            members = order[at[:, None] + np.arange(s)[None, :]].astype(U)      # [groups][s], ascending ids
            a, b = np.triu_indices(int(s), k=1)
            out.append(((members[:, a] << U(32)) | members[:, b]).ravel())
    if not out:
        return np.zeros(0, dtype=U)
    return np.sort(np.concatenate(out))


def emit_case(rng, nq, b, nkeys, r, planted=(300, 1500), zero_first=True, empty_third=True):
    """band keys [b][nq] over ~nkeys distinct values: planted keys of `planted` copies in every band (their runs cross
    the emit's tile borders), key 0 among the first records of band 0, a third of band 1 empty"""
    pool = rng.integers(1, 1 << 62, size=nkeys, dtype=U)
    keys = pool[rng.integers(0, nkeys, size=(b, nq))]
    for band in range(b):
        perm = rng.permutation(nq)
        at = 0
        for copies in planted:
            if at + copies <= nq:
                keys[band, perm[at:at + copies]] = U(int(rng.integers(1, 1 << 62)))
                at += copies
    if empty_third and b > 1:
        keys[1, rng.permutation(nq)[: nq // 3]] = U(empty_key(r))
    if zero_first:
        keys[0, : min(nq, 3)] = U(0)
        if nq > 40:
            keys[0, 40] = U(0)
    return keys


# ------------------------------------------------------------------------------------------------ unique compaction
CMP_SLICE, CMP_TILE = 512, 2048     # words per wave and per workgroup of the compaction kernels (csrc/pairs.hip)


def unique_inputs(rng, n):
    """name -> sorted uint64 [n]: the inputs of ops.unique_sorted (the reference is np.unique)"""
    t = np.arange(n, dtype=np.int64)
    high = U(1 << 63)
    cases = {
        "all_equal": np.full(n, 0xFFFFFFFFFFFFFFF0, dtype=U),
        "all_distinct": (t.astype(U) * U(3)) | np.where(t >= n // 2, high, U(0)),
        # a run per wave slice / per tile: every run starts and ends exactly on a border
        "runs_on_slices": (t // CMP_SLICE).astype(U) | high,
        "runs_on_tiles": (t // CMP_TILE).astype(U),
        # a two-word run across every slice border (and so every tile border): runs start one word before and one after
        "runs_around_borders": ((t + 1) // CMP_SLICE + np.maximum(t - 1, 0) // CMP_SLICE).astype(U),
        # one word of its own exactly at every border, equal words between
        "single_at_borders": (2 * (t // CMP_SLICE) + (t % CMP_SLICE != 0)).astype(U) | np.where(t >= n // 3, high, U(0)),
        "random_runs": np.sort(rng.integers(0, max(2, n // 3), size=n, dtype=U) | (rng.integers(0, 2, size=n, dtype=U) << U(63))),
    }
    for name, a in cases.items():
        assert a.dtype == U and len(a) == n and np.all(a[1:] >= a[:-1]), name
    return cases


# ------------------------------------------------------------------------------------------------ top-K compaction
def topk_case(rng, ib, degrees, ninv=7):
    """directed edge keys src << (ib + 11) | inv << ib | dst (inv = 1000 - value) of sources 0, 1, .. with the given
    degrees; the edges arrive ordered by dst, as the stable (src, inv) sort of ops.topk_edges expects, so the sources
    are interleaved.  Few distinct values: ties at every cut."""
    src = np.repeat(np.arange(len(degrees)), degrees)
    n = len(src)
    dst = np.empty(n, dtype=np.int64)
    at = 0
    for d in degrees:                       # distinct dst per source
        dst[at:at + d] = rng.choice(1 << ib, size=d, replace=False)
        at += d
    inv = rng.integers(0, ninv, size=n)
    o = np.lexsort((src, dst))              # arrival: dst ascending
    src, dst, inv = src[o], dst[o], inv[o]
    keys = (src.astype(U) << U(ib + 11)) | (inv.astype(U) << U(ib)) | dst.astype(U)
    return keys, src, dst, inv


def ref_topk(src, dst, inv, K):
    """the first K of every source by (value descending, dst ascending): -> (src, dst, value) int32"""
    o = np.lexsort((dst, inv, src))
    s, d, v = src[o], dst[o], inv[o]
    first = np.r_[0, np.flatnonzero(s[1:] != s[:-1]) + 1] if len(s) else np.zeros(0, dtype=np.int64)
    pos = np.arange(len(s)) - np.repeat(first, np.diff(np.r_[first, len(s)]))
    keep = pos < K
    return s[keep].astype(np.int32), d[keep].astype(np.int32), (1000 - v[keep]).astype(np.int32)
