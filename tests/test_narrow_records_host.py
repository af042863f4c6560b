"""Host side of the bucket path's 10-byte records (csrc/bucket.hip: a 64-bit word + a 16-bit tail): buffer sizes and the
workspace of the first partition step's [band][slab][part] cursors.  No GPU."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from qrlsh import _lib
    return _lib.load()


def coarse_bits(T):
    return (T + 1) // 2


def slabs(nq, T):
    """slabs of 2^(16 + c1) consecutive queries the first step of a two-step partition deals separately"""
    size = 1 << (16 + coarse_bits(T))
    return (nq + size - 1) // size if T > 8 else 1


def test_part_words_are_what_they_were(lib):
    """part_keys / part_ids keep their sizes: the tails use the id buffer's storage"""
    assert lib.qrlsh_bucket_part_words(1_000_000, 32, 8) == 32 * 256 * 6144 + 32 * 1_000_000 // 16
    assert lib.qrlsh_bucket_part_words(1000, 4, 8) >= 4 * 1000
    assert lib.qrlsh_bucket_part_words(10_000_000, 32, 12) == 32 * 4096 * 4096 + 32 * 10_000_000 // 16
    assert lib.qrlsh_bucket_part_words(100_000_000, 8, 15) == 8 * 32768 * 6144 + 8 * 100_000_000 // 16
    assert lib.qrlsh_bucket_part_words(1 << 25, 2, 9) == 2 * (1 << 25)


@pytest.mark.parametrize("T,b", [(9, 2), (12, 32), (16, 1)])
def test_tmp_words_hold_the_records_and_grow_across_a_slab_boundary(lib, T, b):
    slab = 1 << (16 + coarse_bits(T))
    sizes = [1000, slab // 2, slab - 1, slab, slab + 1, slab + 4097, 2 * slab, 2 * slab + 1, 3 * slab - 5]
    words = [lib.qrlsh_bucket_tmp_words(nq, b, T) for nq in sizes]
    for nq, w in zip(sizes, words):
        assert w >= b * nq, (T, nq)
    assert words == sorted(words), list(zip(sizes, words))
    # a query past the boundary opens a slab of its own: a second set of coarse regions
    at, past = lib.qrlsh_bucket_tmp_words(slab, b, T), lib.qrlsh_bucket_tmp_words(slab + 1, b, T)
    assert past == 2 * at
    assert lib.qrlsh_bucket_tmp_words(1_000_000, b, 8) == 0


@pytest.mark.parametrize("T,b,nq", [(12, 32, 10_000_000), (9, 2, (1 << 21) + 150_000), (12, 1, (1 << 24) + 70_000),
                                    (9, 2, 1 << 21), (8, 2, 200_000)])
def test_workspace_covers_the_slab_cursors(lib, T, b, nq):
    """first-step cursors [band][slab][part], second-step cursors, fill marks and the big-part lists, at least"""
    c1 = coarse_bits(T)
    slots = b << T
    cur1 = 4 * ((b * slabs(nq, T)) << c1) if T > 8 else 0
    floor = cur1 + 4 * slots + 4 * slots + 8 * slots
    ws = lib.qrlsh_bucket_workspace_bytes(nq, b, T)
    assert ws >= floor, (ws, floor)
    if T > 8:
        # one more slab: one more set of b << c1 cursors
        slab = 1 << (16 + c1)
        more = lib.qrlsh_bucket_workspace_bytes(nq + slab, b, T)
        assert more - ws >= 4 * (b << c1)
    assert slabs(10_000_000, 12) == 3
