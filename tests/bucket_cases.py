"""Builders of adversarial band-key matrices for the partition + LDS-finish bucket path (csrc/bucket.hip): planted
multiplicities, several popular keys hashed into ONE part, a part filled to exactly N records.  Shared by
tests/test_gpu_buckets.py and tools/stress_buckets.py.

Every builder returns a BucketCase: the band-major int64 keys [b][nq] and what it meant to build -- the partition depth
T, the band and part it aimed at and the exact number of records that part holds (its background records included).
The part of a key is the top T bits of mix64(key), as the one-kernel partition computes it.  Pure numpy: nothing here
needs the library or a GPU, so a case can be checked on the host before anything runs."""
from typing import NamedTuple

import numpy as np


class BucketCase(NamedTuple):
    name: str
    keys: np.ndarray      # int64 [b][nq], band-major (what emit_pairs_any takes)
    T: int                # partition depth the case is built for (ops.part_bits_for(nq) must agree)
    band: int             # band of the target part
    part: int             # target part: mix64(key) >> (64 - T)
    count: int            # records of that part in that band
    hot: tuple            # the planted keys of the target part (int), for cross-checks of the mixer


def np_mix64(z):
    """splitmix64 finaliser, as qr_mix64 (csrc/common.h) -- on uint64 arrays"""
    z = np.asarray(z).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def parts_of(row, T):
    """part id of every key of one band at depth T (int64)"""
    return (np_mix64(np.asarray(row).view(np.uint64)) >> np.uint64(64 - T)).astype(np.int64)


def part_count(keys, T, band, part):
    return int(np.count_nonzero(parts_of(keys[band], T) == part))


def planted_keys(rng, nq, b, groups, T, name=""):
    """[b][nq] keys: random distinct background + for every (size, count) in groups `count` keys with `size` copies per
    band.  Target: the part of band 0's largest planted key."""
    keys = rng.integers(1, 1 << 62, size=(b, nq), dtype=np.int64)
    big, big_size = None, 0
    for band in range(b):
        perm = rng.permutation(nq)
        at = 0
        for size, count in groups:
            for _ in range(count):
                if at + size > nq:
                    break
                k = int(rng.integers(1, 1 << 62))
                keys[band, perm[at:at + size]] = k
                at += size
                if band == 0 and size > big_size:
                    big, big_size = k, size
    part = int(parts_of(np.array([big], dtype=np.int64), T)[0])
    return BucketCase(name, keys, T, 0, part, part_count(keys, T, 0, part), (big,))


def same_part_keys(rng, nq, T, sizes, fill_to=None, name=""):
    """one band whose popular keys all hash into ONE part of the T-bit partition.
    fill_to: instead of sizes, ONE key with exactly as many copies as bring that part to fill_to records (the part's
    background records stay; records from elsewhere join it)."""
    keys = rng.integers(1, 1 << 62, size=(1, nq), dtype=np.int64)
    want = None
    perm = rng.permutation(nq)
    at = 0
    hot = []
    if fill_to is not None:
        k = int(rng.integers(1, 1 << 62))
        want = int(parts_of(np.array([k], dtype=np.int64), T)[0])
        parts = parts_of(keys[0], T)
        inside = np.flatnonzero(parts == want)
        outside = np.flatnonzero(parts != want)
        size = fill_to - len(inside)
        assert size > 1, "the part's background already holds %d records" % len(inside)
        keys[0, outside[:size]] = k
        hot.append(k)
    else:
        for size in sizes:
            while True:
                k = int(rng.integers(1, 1 << 62))
                part = int(parts_of(np.array([k], dtype=np.int64), T)[0])
                if want is None:
                    want = part
                if part == want:
                    break
            keys[0, perm[at:at + size]] = k
            at += size
            hot.append(k)
    return BucketCase(name, keys, T, 0, want, part_count(keys, T, 0, want), tuple(hot))


def two_group_keys(rng, nq, b, T, heavy=(30000, 9000), name=""):
    """b bands split by the emit into two band groups (b * nq >= 2^26): ordinary buckets of 2 .. 7 members, and in the
    first band of each half the popular keys `heavy` (each one's part spills into the overflow pool).  Target: the part
    of the first popular key of the SECOND half."""
    keys = rng.integers(1, 1 << 62, size=(b, nq), dtype=np.int64)
    half = (b + 1) // 2
    for band in range(b):
        perm = rng.permutation(nq)
        at = 0
        for size, count in ((2, 20000), (3, 5000), (7, 2000)):
            for _ in range(count):
                keys[band, perm[at:at + size]] = int(rng.integers(1, 1 << 62))
                at += size
        if band in (0, half):
            hot = []
            for size in heavy:
                k = int(rng.integers(1, 1 << 62))
                keys[band, perm[at:at + size]] = k
                at += size
                hot.append(k)
    part = int(parts_of(np.array([hot[0]], dtype=np.int64), T)[0])
    return BucketCase(name, keys, T, half, part, part_count(keys, T, half, part), (hot[0],))


# queries per case at each depth: the mean part (nq >> T) is what picks the finish form -- 1024 .. 2800 records: the
# 4096-record small-part image (packed counters at T >= 12, separate counters below); 1 M queries at T = 8: one-step
# partition, regions of one 6144-record image
FILL_NQ = {8: 1_000_000, 11: 5_500_000, 12: 10_000_000}
FILLS = {12: (4094, 4095, 4096, 4097, 6143, 6144, 6145), 11: (4095, 4096, 4097), 8: (6143, 6144, 6145)}
MIX = [(2, 20000), (3, 5000), (7, 2000), (40, 300), (300, 40), (1700, 6), (4100, 2), (9000, 1)]


def fill_case(T, N):
    """a part of exactly N records at depth T (one seed per case)"""
    return same_part_keys(np.random.default_rng(1000 * T + N), FILL_NQ[T], T, None, fill_to=N,
                          name="T=%d, a part of exactly %d records" % (T, N))


def two_group_case():
    """12 M queries x 6 bands (>= 2^26 records: the emit's two band groups), spills in a band of each group"""
    return two_group_keys(np.random.default_rng(77), 12_000_000, 6, 12, heavy=(9000, 5000),
                          name="two band groups, popular keys in both")
