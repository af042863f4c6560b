"""The answer-set reference and the planted tables of tests/answers_cases.py hold (no GPU): the reference against the
oracle, the planted sizes and places against what the builders promise, and the host side of qrlsh/answers.py (the
bitmaps and the query encoding) against the reference by AND-ing the bitmaps with numpy."""
import numpy as np
import pytest

import answers_cases as A
from oracle import oracle as O  # checker only
from qrlsh import answers


def host_answer_sets(index, qrows):
    """what the kernel computes, from the host copy of the bitmaps: AND of the chosen bitmap rows, rows below D"""
    bm = index.bitmaps.numpy().view(np.uint32)
    bits = np.unpackbits(bm.view(np.uint8), axis=1, bitorder="little")[:, :index.D].astype(bool)
    sets = []
    for q in qrows:
        mask = np.ones(index.D, dtype=bool)
        for r in q:
            if r >= 0:
                mask &= bits[r]
        sets.append(np.flatnonzero(mask).astype(np.int32))
    off = np.zeros(len(sets) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    return off, np.concatenate(sets + [np.zeros(0, np.int32)]).astype(np.int32)


def test_reference_equals_oracle_on_random_tables():
    rng = np.random.default_rng(4)
    for (D, nfeat, card, nq) in [(1, 1, 1, 3), (33, 2, 3, 40), (1000, 5, 7, 120), (2500, 3, 50, 100)]:
        cols = [rng.integers(0, card, size=D).astype(str) for _ in range(nfeat)]
        q = np.full((nq, nfeat), "", dtype=object)
        for i in range(nq):
            for f in range(nfeat):
                u = rng.random()
                if u < 0.5:
                    q[i, f] = str(rng.integers(0, card))
                elif u < 0.55:
                    q[i, f] = "no-such-value"
        q[0, :] = ""
        off, rows = A.ref_answer_sets(cols, q)
        roff, rrows = O.answer_sets(cols, q)
        assert off.dtype == np.int64 and rows.dtype == np.int32
        assert np.array_equal(off, roff) and np.array_equal(rows, rrows)
        assert off[1] == D


@pytest.mark.parametrize("D", A.D_EDGES)
def test_planted_tables_hold_exactly_what_they_promise(D):
    assert {1, 31, 32, 33, 2047, 2048, 2049, 8065, 8191, 8192, 8193} <= set(A.D_EDGES)
    seen = set()
    for variant in range(4):
        plants = A.plants_for(D, variant)
        cols, _ = A.planted_columns(D, 3, variant)
        taken = np.zeros(D, dtype=int)
        for value, k, start in plants:
            taken[start:start + k] += 1
            assert np.array_equal(np.flatnonzero(cols[0] == value), np.arange(start, start + k))   # exactly k rows
            seen |= {(k, "first")} if start == 0 else set()
            seen |= {(k, "last")} if start + k == D else set()
            edge = A.step_rows(D) * ((D - 1) // A.step_rows(D))
            seen |= {(k, "step")} if start < edge < start + k else set()
        assert taken.max(initial=0) <= 1
        ks = {k for _, k, _ in plants}
        if D < 63:
            assert ks == {1}
        if D >= 2047:
            assert ks == set(A.PLANT_SIZES)
            assert any(s == 0 for _, _, s in plants) and any(s + k == D for _, k, s in plants)     # first and last rows
            assert any(s < 128 < s + k for _, k, s in plants)                                      # a lane's four words
            assert any(s % 32 + k > 32 for _, k, s in plants)                                      # a 32-row word
        step = A.step_rows(D)
        if D > step:                                                                               # a wave step
            assert any(s < step * ((D - 1) // step) < s + k for _, k, s in plants), (D, plants)
    if D >= 2047:     # over the variants every size of 63 and more sits at the head, at the tail and on a step boundary
        for k in (63, 64, 65):
            assert {(k, "first"), (k, "last")} <= seen, (D, seen)
            assert (k, "step") in seen or D <= A.step_rows(D), (D, seen)
    assert A.step_rows(2048) == 8192 and A.step_rows(2049) == 2048 and A.step_rows(8193) == 2048 and A.step_rows(8320) == 8192


@pytest.mark.parametrize("nfeat", A.NFEATS)
@pytest.mark.parametrize("D", [1, 33, 2049, 8192])
def test_query_pool_and_route_batches(D, nfeat):
    cols, plants = A.planted_columns(D, nfeat, variant=nfeat % 4)
    pool = A.query_pool(D, nfeat, plants)
    assert pool.shape == (131, nfeat)
    off, rows = A.ref_answer_sets(cols, pool)
    roff, rrows = O.answer_sets(cols, pool)
    assert np.array_equal(off, roff) and np.array_equal(rows, rrows)
    sizes = A.sizes_of(off)
    want = {0, D} | {k for _, k, _ in plants}
    assert want <= set(sizes.tolist()), (want, set(sizes.tolist()))
    if D >= 2047:
        assert {0, 1, 63, 64, 65, D} <= set(sizes.tolist())
    if nfeat >= 2:        # the last feature is constrained in some queries (with nfeat = 64: the last lane's bitmap row)
        assert np.count_nonzero(pool[:, nfeat - 1] != "") >= 10
    compact, refill = A.route_batches(pool, sizes)
    csz = A.sizes_of(A.ref_answer_sets(cols, compact)[0])
    assert csz.max() == min(A.SLOT, D) and 0 in csz
    if D > A.SLOT:
        rsz = A.sizes_of(A.ref_answer_sets(cols, refill)[0])
        assert rsz.max() == A.SLOT + 1 and np.count_nonzero(rsz > A.SLOT) == 1 and len(rsz) == len(csz) + 1
    else:
        assert refill is None


def test_encode_queries_and_bitmaps_on_the_host():
    cols, plants = A.planted_columns(300, 4, variant=1)
    idx = answers.build_answer_index(cols, device="cpu")
    assert idx.D == 300 and idx.wpr == 10 and idx.nfeat == 4
    pool = A.query_pool(300, 4, plants, n=60)
    extra = np.full((5, 4), "", dtype=object)
    extra[0, 0], extra[1, 0], extra[2, 0] = A.ABSENT          # before, between and after the column's values
    extra[3, 3] = "zz-after-every-value"
    q = np.concatenate([pool, extra])                         # (extra[4]: fully unconstrained)
    qr = answers.encode_queries(idx, q)
    assert qr.dtype == np.int32 and qr.shape == q.shape
    vals0 = idx.value_rows[0][0]
    assert A.ABSENT[0] < vals0[0] and vals0[2] < A.ABSENT[1] < vals0[3] and A.ABSENT[2] > vals0[-1]
    assert np.all(qr[-5:-2, 0] == idx.zero_row) and qr[-2, 3] == idx.zero_row and np.all(qr[-1] == -1)
    assert np.all((qr == -1) == (q == ""))
    for f in range(4):
        v, base = idx.value_rows[f]
        for i in range(len(q)):
            if q[i, f] != "" and q[i, f] in set(v.tolist()):
                assert qr[i, f] == base + sorted(v.tolist()).index(q[i, f])
    off, rows = host_answer_sets(idx, qr)
    roff, rrows = A.ref_answer_sets(cols, q)
    assert np.array_equal(off, roff) and np.array_equal(rows, rrows)
    assert off[-1] - off[-2] == 300 and np.all(np.diff(off)[-5:-1] == 0)


def test_encode_queries_keeps_a_longer_query_value_whole():
    """fixed-width string columns: a query value longer than every value of the table is absent -- it must not be cut
    to the column's width and then found"""
    cols = [np.array(["12", "7", "12", "30"]), np.array(["x", "y", "x", "y"])]
    assert cols[0].dtype.kind == "U"
    idx = answers.build_answer_index(cols, device="cpu")
    q = np.array([["12", ""], ["123", ""], ["7", "x"], ["70", "y"], ["", "yy"], ["3", ""], ["", ""]], dtype=object)
    qr = answers.encode_queries(idx, q)
    off, rows = host_answer_sets(idx, qr)
    roff, rrows = A.ref_answer_sets(cols, q)
    assert np.array_equal(off, roff) and np.array_equal(rows, rrows)
    assert np.diff(off).tolist() == [2, 0, 0, 0, 0, 0, 4]
    assert qr[1, 0] == idx.zero_row and qr[4, 1] == idx.zero_row
