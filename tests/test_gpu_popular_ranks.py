"""Own-pair ranks of the block kernel of the bucket finish (csrc/bucket.hip: bucket_finish_big_kernel).  A record's rank
among its bucket-mates decides which of the eight slice workgroups writes its pairs; runs up to FIN_RANK_SORT copies
are ranked by a lane per record, longer ones are sorted in LDS by the workgroup and ranked by position.  One part of a
one-band key matrix is filled to just beyond the LDS image, so that the block kernel works it and its first block holds
(all but at most a few of) the copies of the planted keys: run lengths on both sides of the threshold, a run of a whole
block and one more, two long runs in one block, long runs split over two blocks -- emitted pairs (with multiplicity) and
the unique set against the oracle."""
import numpy as np
import pytest
import torch

import bucket_cases as B

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
R = 4
T, NQ = 8, 1_000_000      # one-step partition, parts of ~3 900 background records, regions of one 6144-record image
FIN_CAP = 6144            # csrc/common.h: records of an LDS image = a block of the big kernel
FIN_RANK_SORT = 256       # csrc/bucket.hip: runs beyond this are sorted


def planted_part(seed, sizes, total):
    """one band of NQ distinct keys; keys with sizes[k] copies all in ONE part, and (total is not None) one more key
    there with as many copies as bring the part to exactly `total` records.  -> (keys [1][NQ], part, records of it)"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(1, 1 << 62, size=(1, NQ), dtype=np.int64)
    hot, want = [], None
    while len(hot) < len(sizes) + (total is not None):
        k = int(rng.integers(1, 1 << 62))
        part = int(B.parts_of(np.array([k], dtype=np.int64), T)[0])
        if want is None:
            want = part
        if part == want:
            hot.append(k)
    parts = B.parts_of(keys[0], T)
    inside, outside = int(np.count_nonzero(parts == want)), np.flatnonzero(parts != want)
    sizes = list(sizes)
    if total is not None:
        sizes.append(total - inside - sum(sizes))
        assert sizes[-1] > 1, (inside, sizes)
    at = 0
    for k, size in zip(hot, sizes):
        keys[0, outside[at:at + size]] = k
        at += size
    n = B.part_count(keys, T, 0, want)
    assert n == inside + sum(sizes) and (total is None or n == total)
    return keys, want, n


def emit_and_check(keys):
    stats = {}
    old = _lib.load().qrlsh_set_big_part_limit(0)          # the default limit, whatever an earlier test left
    try:
        emitted = ops.emit_pairs_any(torch.from_numpy(keys).to(DEV), R, stats)
        torch.cuda.synchronize()
    finally:
        _lib.load().qrlsh_set_big_part_limit(old)
    assert stats["bucket_path"] == "partition+lds", stats
    O.set_threads(min(16, O.max_threads()))
    kq = np.ascontiguousarray(keys.T).view(np.uint64)
    assert emitted.numel() == O.emitted_pairs(kq, R)
    assert np.array_equal(O.sort_unique(emitted.cpu().numpy().view(np.uint64)), O.candidates(kq, R))


@pytest.mark.parametrize("copies,total", [(63, FIN_CAP + 1), (64, FIN_CAP + 1), (65, FIN_CAP + 1),
                                          (FIN_RANK_SORT - 1, FIN_CAP + 1), (FIN_RANK_SORT, FIN_CAP + 1),
                                          (FIN_RANK_SORT + 1, FIN_CAP + 1), (FIN_RANK_SORT + 2, FIN_CAP + 1),
                                          (FIN_RANK_SORT + 2, FIN_CAP + 2), (1700, FIN_CAP + 1), (2000, FIN_CAP + 40)])
def test_one_key_either_side_of_the_rank_threshold(copies, total):
    """the part holds one record (or a few) more than a block: the first block carries the key's copies but for at most
    total - FIN_CAP of them, so the run lengths 254 .. 258 fall on both sides of the threshold"""
    assert ops.part_bits_for(NQ) == T
    keys, _, n = planted_part(1000 + copies + total, [copies], total)
    assert n == total > FIN_CAP
    emit_and_check(keys)


@pytest.mark.parametrize("copies", [FIN_CAP, FIN_CAP + 1])
def test_one_key_of_a_block_and_one_more(copies):
    """6 144 / 6 145 copies beside the part's ~3 900 background records: two blocks, the run split between them"""
    keys, _, n = planted_part(copies, [copies], None)
    assert n > FIN_CAP + 3000
    emit_and_check(keys)


def test_two_long_runs_in_one_block():
    keys, _, n = planted_part(77, [1200, 900], FIN_CAP + 1)
    assert n == FIN_CAP + 1
    emit_and_check(keys)


def test_long_runs_split_over_two_blocks():
    keys, _, n = planted_part(78, [3000, 2500], None)
    assert FIN_CAP + 2000 < n <= 2 * FIN_CAP
    emit_and_check(keys)
