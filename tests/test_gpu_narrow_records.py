"""The bucket path's 10-byte records (csrc/bucket.hip): a 64-bit word whose top bits carry the id's bits from 16 up, and
a 16-bit tail.  Each case is the smallest shape at which one piece of that form can go wrong -- tails that wrap, ids
that differ only in the slab of the first partition step, the chunked key layout across a slab boundary, pool and
block kernel on narrow records, id bits high in the finish's field.  Everything goes through ops.emit_pairs_fast and is
compared with the oracle exactly: the emitted count and the unique set."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
R = 4


def u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(autouse=True)
def _oracle_threads():
    O.set_threads(min(16, O.max_threads()))


def build_keys(seed, nq, b, buckets):
    """[b][nq] int64: random distinct background, and in every band one fresh key per planted bucket (a list of query
    ids; the buckets are disjoint)"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(1, 1 << 62, size=(b, nq), dtype=np.int64)
    seen = set()
    for members in buckets:
        assert len(set(members)) == len(members) and not seen.intersection(members), members
        assert 0 <= min(members) and max(members) < nq, members
        seen.update(members)
    for band in range(b):
        for members in buckets:
            keys[band, np.asarray(members, dtype=np.int64)] = int(rng.integers(1, 1 << 62))
    return keys


def oracle_of(keys):
    kq = np.ascontiguousarray(keys.T).view(np.uint64)
    return O.candidates(kq, R), O.emitted_pairs(kq, R)


def planted_pairs(buckets):
    out = []
    for members in buckets:
        m = sorted(members)
        out += [(m[i] << 32) | m[j] for i in range(len(m)) for j in range(i + 1, len(m))]
    return np.array(sorted(out), dtype=np.uint64)


def check_emit(keys_dev, T, want, n_want, chunks=None):
    emitted = ops.emit_pairs_fast(keys_dev, R, part_bits=T, chunks=chunks)
    torch.cuda.synchronize()
    assert emitted is not None, "the partition + LDS finish overflowed"
    assert emitted.numel() == n_want
    assert np.array_equal(O.sort_unique(u64(emitted)), want)


# ---- 1. tails that wrap, one partition step ---------------------------------------------------------------------------
def test_tail_wrap_one_level():
    """T = 8: ids q, q + 65 536, q + 131 072 have equal tails and differ in the bits the word carries; 65 535 / 65 536
    are neighbours across the wrap"""
    nq, b, T = 200_000, 2, 8
    buckets = [[q, q + 65536, q + 131072] for q in (2, 777, 4095, 4096, 40000, 65534, 68927)]
    buckets += [[65535, 65536], [131071, 199_998], [65537, 3]]
    keys = build_keys(801, nq, b, buckets)
    want, n_want = oracle_of(keys)
    assert np.isin(planted_pairs(buckets), want).all()
    check_emit(torch.from_numpy(keys).to(DEV), T, want, n_want)


# ---- 2. - 4. slabs of the first of two steps --------------------------------------------------------------------------
SLAB_T, SLAB = 9, 1 << 21        # c1 = 5: slabs of 2^(16+5) queries
SLAB_NQ, SLAB_B = SLAB + 150_000, 2


def slab_buckets():
    bk = [[SLAB - 1, SLAB, SLAB + 1]]
    bk += [[q, q + SLAB] for q in (2, 5, 4095, 65535, 65536, 100_000, 149_990)]   # equal explicit bits, another slab
    bk += [[SLAB - 2, 2 * 65536 + 7, SLAB + 65536 + 7], [SLAB_NQ - 1, 11], [SLAB_NQ - 2, SLAB - 3, SLAB + 9]]
    return bk


@pytest.fixture(scope="module")
def slab_case():
    """shared by the plain and the chunked run; not modified"""
    assert SLAB_NQ % 4096 != 0 and (SLAB_NQ - SLAB) % 4096 != 0      # the last slab and its last tile are partial
    buckets = slab_buckets()
    keys = build_keys(902, SLAB_NQ, SLAB_B, buckets)
    want, n_want = oracle_of(keys)
    assert np.isin(planted_pairs(buckets), want).all()
    return keys, want, n_want


def test_slabs(slab_case):
    """T = 9: the first step deals two slabs (the second partial, its last tile partial); buckets join ids across the
    slab boundary and ids that differ only in the slab"""
    keys, want, n_want = slab_case
    check_emit(torch.from_numpy(keys).to(DEV), SLAB_T, want, n_want)


def test_slabs_chunked_layout(slab_case):
    """the same keys as three ranks' chunks [rank][band][750 000]: the slab boundary falls inside the third chunk"""
    keys, want, n_want = slab_case
    world, nql = 3, 750_000
    assert world * nql > SLAB_NQ > SLAB > 2 * nql
    # the chunked layout wants world * nql queries: pad with one more distinct key per (band, query)
    nq = world * nql
    rng = np.random.default_rng(903)
    full = np.concatenate([keys, rng.integers(1 << 62, (1 << 62) + (1 << 61), size=(SLAB_B, nq - SLAB_NQ), dtype=np.int64)],
                          axis=1)
    want_full, n_full = oracle_of(full)
    assert np.isin(want, want_full).all()
    chunked = np.ascontiguousarray(full.reshape(SLAB_B, world, nql).transpose(1, 0, 2)).reshape(-1)
    check_emit(torch.from_numpy(chunked).to(DEV), SLAB_T, want_full, n_full, chunks=(world, SLAB_B, nql))


def test_pool_and_block_kernel_on_narrow_records(slab_case):
    """a key with 7 000 copies over the whole id range (both slabs, many 65 536 boundaries): its part spills into the
    pool and the block kernel pairs it; with the block kernel's limit lowered the call reports the overflow and the
    general path gives the same pairs"""
    lib = _lib.load()
    rng = np.random.default_rng(904)
    hot = np.sort(rng.choice(SLAB_NQ, size=7000, replace=False))
    taken = {q for m in slab_buckets() for q in m}
    hot = np.array([q for q in hot if q not in taken], dtype=np.int64)
    assert hot.min() < 65536 and hot.max() > SLAB + 65536 and len(np.unique(hot >> 16)) >= 30
    keys = slab_case[0].copy()
    keys[0, hot] = int(rng.integers(1, 1 << 62))
    want, n_want = oracle_of(keys)
    assert n_want >= len(hot) * (len(hot) - 1) // 2
    dev = torch.from_numpy(keys).to(DEV)
    check_emit(dev, SLAB_T, want, n_want)
    old = lib.qrlsh_set_big_part_limit(6144)
    try:
        assert ops.emit_pairs_fast(dev, R, part_bits=SLAB_T) is None        # the key's part is beyond the limit
        sk, sid = ops.bucket_sort(dev.clone())
        emitted = ops.emit_pairs(sk, sid, R)
        torch.cuda.synchronize()
        assert emitted.numel() == n_want
        assert np.array_equal(O.sort_unique(u64(emitted)), want)
    finally:
        lib.qrlsh_set_big_part_limit(old)
    check_emit(dev, SLAB_T, want, n_want)                                  # the limit is back


# ---- 5. id bits high in the finish's field ----------------------------------------------------------------------------
def test_high_id_bits_in_the_finish():
    """T = 12, ids past 2^24: the word's id field (12 bits above 52 x bits) carries 9 bits; five slabs in the first
    step"""
    nq, T = (1 << 24) + 70_000, 12
    buckets = [[5, (1 << 24) + 5, 65541, (1 << 24) + 65541], [nq - 1, 0], [(1 << 24) - 1, 1 << 24, (1 << 22) + 1, 1 << 22]]
    keys = build_keys(905, nq, 1, buckets)
    want, n_want = oracle_of(keys)
    assert np.isin(planted_pairs(buckets), want).all()
    check_emit(torch.from_numpy(keys).to(DEV), T, want, n_want)
