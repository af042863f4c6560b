"""The answer-set kernels (csrc/answers.hip) against the plain reference of tests/answers_cases.py on planted tables:
sets of exactly 0, 1, 63, 64, 65 and D rows at the first rows, the last rows and across a word, a lane's words and a
wave step; D at the edges of a step at both load widths; up to 64 features; both forms (one sweep + compact or refill,
count then fill), the route each batch takes, bits beyond D in the bitmaps, and the CSR handed on to MinHash.  Every
comparison is exact and covers whole outputs."""
import numpy as np
import pytest
import torch

import answers_cases as A
import minhash_cases as M

pytestmark = pytest.mark.gpu

from qrlsh import _lib, answers, ops  # noqa: E402
from qrlsh.ops import _ptr, _stream  # noqa: E402

DEV = "cuda"
_CASES = {}


def case(D, nfeat):
    """(index on the device, query pool, encoded pool, reference CSR of the pool) -- built once per (D, nfeat)"""
    if (D, nfeat) not in _CASES:
        variant = A.NFEATS.index(nfeat)
        cols, plants = A.planted_columns(D, nfeat, variant)
        idx = answers.build_answer_index(cols, DEV)
        pool = A.query_pool(D, nfeat, plants)
        _CASES[(D, nfeat)] = (cols, idx, pool, answers.encode_queries(idx, pool), A.ref_answer_sets(cols, pool))
    return _CASES[(D, nfeat)]


def ref_slice(ref, nq):
    off, rows = ref
    return off[:nq + 1], rows[:off[nq]]


def raw_sizes(idx, qr, sweep):
    """the sizes straight from qrlsh_answer_sets_count or qrlsh_answer_sets_sweep (+ the slots of the sweep)"""
    lib = _lib.load()
    d_qr = torch.from_numpy(np.ascontiguousarray(qr, dtype=np.int32)).to(DEV)
    nq, nfeat = d_qr.shape
    sizes = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    if not sweep:
        _lib.check(lib.qrlsh_answer_sets_count(_ptr(idx.bitmaps), idx.wpr, idx.D, _ptr(d_qr), nq, nfeat, _ptr(sizes), _stream()))
        return sizes, None
    slots = torch.full((nq, answers.SLOT), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.qrlsh_answer_sets_sweep(_ptr(idx.bitmaps), idx.wpr, idx.D, _ptr(d_qr), nq, nfeat, _ptr(sizes), _ptr(slots),
                                           _stream()))
    return sizes, slots


def check_both_forms(idx, qr, ref, what):
    off, rows = ref
    for one_sweep in (True, False):
        g_off, g_rows = answers.answer_sets(idx, qr, one_sweep=one_sweep)
        assert g_off.dtype == torch.int64 and g_rows.dtype == torch.int32
        assert np.array_equal(g_off.cpu().numpy(), off), (what, one_sweep)
        assert np.array_equal(g_rows.cpu().numpy(), rows), (what, one_sweep)


@pytest.mark.parametrize("nfeat", A.NFEATS)
@pytest.mark.parametrize("D", A.D_EDGES)
def test_both_forms_equal_the_reference(D, nfeat):
    assert answers.SLOT == A.SLOT
    cols, idx, pool, qr, ref = case(D, nfeat)
    assert idx.wpr == A.words_per_row(D)
    for nq in A.NQS:
        check_both_forms(idx, qr[:nq], ref_slice(ref, nq), (D, nfeat, nq))
    # the sizes of the count pass and of the sweep agree with the reference and with each other
    want = torch.from_numpy(A.sizes_of(ref[0]).astype(np.int32))
    counted, _ = raw_sizes(idx, qr, sweep=False)
    swept, _ = raw_sizes(idx, qr, sweep=True)
    assert torch.equal(counted.cpu(), want) and torch.equal(swept.cpu(), want)


@pytest.mark.parametrize("nfeat", A.NFEATS)
@pytest.mark.parametrize("D", A.D_EDGES)
def test_route_of_a_batch_with_exactly_64_and_with_one_set_of_65(D, nfeat):
    cols, idx, pool, qr, ref = case(D, nfeat)
    sizes = A.sizes_of(ref[0])
    compact, refill = A.route_batches(pool, sizes)
    # largest set exactly SLOT rows (or D, for a smaller table): the compact route
    c_ref = A.ref_answer_sets(cols, compact)
    c_qr = answers.encode_queries(idx, compact)
    check_both_forms(idx, c_qr, c_ref, (D, nfeat, "compact"))
    g_off, _ = answers.answer_sets(idx, c_qr, one_sweep=True)
    assert int(np.diff(g_off.cpu().numpy()).max()) == min(A.SLOT, D)
    # ... and by hand, so that the route is not a matter of trust: sweep, scan, compact
    lib = _lib.load()
    swept, slots = raw_sizes(idx, c_qr, sweep=True)
    assert np.array_equal(swept.cpu().numpy(), A.sizes_of(c_ref[0]))
    offsets = torch.zeros((len(compact) + 1,), dtype=torch.int64, device=DEV)
    torch.cumsum(swept, dim=0, out=offsets[1:])
    rows = torch.full((int(c_ref[0][-1]) + 8,), -9, dtype=torch.int32, device=DEV)
    _lib.check(lib.qrlsh_answer_sets_compact(_ptr(slots), _ptr(offsets), len(compact), _ptr(rows), _stream()))
    assert np.array_equal(rows.cpu().numpy()[:-8], c_ref[1]) and torch.all(rows[-8:] == -9)
    # the parked ids are the sets themselves, nothing is written behind a set's last id
    h_slots = slots.cpu().numpy()
    for q in range(len(compact)):
        n = int(c_ref[0][q + 1] - c_ref[0][q])
        assert np.array_equal(h_slots[q, :n], c_ref[1][c_ref[0][q]:c_ref[0][q + 1]]) and np.all(h_slots[q, n:] == -7)
    if D <= A.SLOT:
        assert refill is None
        return
    # one set of SLOT + 1 rows among them: the refill
    r_ref = A.ref_answer_sets(cols, refill)
    r_qr = answers.encode_queries(idx, refill)
    check_both_forms(idx, r_qr, r_ref, (D, nfeat, "refill"))
    g_off, _ = answers.answer_sets(idx, r_qr, one_sweep=True)
    assert int(np.diff(g_off.cpu().numpy()).max()) == A.SLOT + 1
    swept, slots = raw_sizes(idx, r_qr, sweep=True)
    assert np.array_equal(swept.cpu().numpy(), A.sizes_of(r_ref[0]))
    big = int(np.argmax(A.sizes_of(r_ref[0])))
    lo = int(r_ref[0][big])
    assert np.array_equal(slots[big].cpu().numpy(), r_ref[1][lo:lo + A.SLOT])      # the first 64 ids, not one more


@pytest.mark.parametrize("nfeat", [1, 3, 64])
@pytest.mark.parametrize("D", [D for D in A.D_EDGES if D % 32])
def test_bits_beyond_d_in_the_bitmaps_change_nothing(D, nfeat):
    """every bit at positions >= D of the last word of every bitmap row set (the all-zero row included): constrained
    and unconstrained queries give what they gave"""
    if nfeat == 3:
        cols, plants = A.planted_columns(D, 3, 2)
        idx = answers.build_answer_index(cols, DEV)
        pool = A.query_pool(D, 3, plants)
        qr, ref = answers.encode_queries(idx, pool), A.ref_answer_sets(cols, pool)
    else:
        cols, idx, pool, qr, ref = case(D, nfeat)
    bm = idx.bitmaps.clone()
    bm[:, idx.wpr - 1] |= -(1 << (D % 32))
    assert int((bm[idx.zero_row] != 0).sum()) == 1
    dirty = answers.AnswerIndex(bm, idx.D, idx.wpr, idx.value_rows, idx.zero_row)
    assert np.count_nonzero(qr == idx.zero_row) > 0 and np.count_nonzero(np.all(qr == -1, axis=1)) > 0
    check_both_forms(dirty, qr, ref, (D, nfeat, "dirty"))
    compact, _ = A.route_batches(pool, A.sizes_of(ref[0]))
    check_both_forms(dirty, answers.encode_queries(idx, compact), A.ref_answer_sets(cols, compact), (D, nfeat, "dirty compact"))
    want = torch.from_numpy(A.sizes_of(ref[0]).astype(np.int32))
    assert torch.equal(raw_sizes(dirty, qr, sweep=False)[0].cpu(), want) and torch.equal(raw_sizes(dirty, qr, sweep=True)[0].cpu(), want)


def test_absent_value_gives_an_empty_set_between_undisturbed_neighbours():
    cols, idx, pool, qr, ref = case(2049, 2)
    sizes = A.sizes_of(ref[0])
    plant = pool[int(np.flatnonzero((sizes > 1) & (sizes <= A.SLOT))[0])].copy()
    absent = np.array([A.ABSENT[1], ""], dtype=object)
    q = np.stack([plant, absent, plant, np.array(["", ""], dtype=object), absent, plant])
    r_off, r_rows = A.ref_answer_sets(cols, q)
    n = int(r_off[1])
    assert n > 0 and r_off.tolist() == [0, n, n, 2 * n, 2 * n + 2049, 2 * n + 2049, 3 * n + 2049]
    check_both_forms(idx, answers.encode_queries(idx, q), (r_off, r_rows), "absent")
    q2 = np.stack([plant, absent, plant, absent, plant])          # the same on the compact route
    ref2 = A.ref_answer_sets(cols, q2)
    assert A.sizes_of(ref2[0]).max() <= A.SLOT
    check_both_forms(idx, answers.encode_queries(idx, q2), ref2, "absent compact")


def test_a_batch_of_nothing_but_empty_sets():
    """every query of the batch names an absent value: offsets all zero, no rows, on both routes (this raised "null
    pointer" from the compact and the fill pass: the rows tensor is empty; found through Recommender.add_queries of one
    query that no row answers, by the random schedules of test_gpu_live_sequence.py)"""
    cols, idx, pool, qr, ref = case(2049, 2)
    absent = np.array([A.ABSENT[1], ""], dtype=object)
    for nq in (1, 3, 65):
        q = np.stack([absent] * nq)
        r_off, r_rows = A.ref_answer_sets(cols, q)
        assert r_off.tolist() == [0] * (nq + 1) and len(r_rows) == 0
        check_both_forms(idx, answers.encode_queries(idx, q), (r_off, r_rows), ("nothing but empty sets", nq))


@pytest.mark.parametrize("D,nfeat,kind,P,b", [(2049, 2, "u16", 100, 20), (8193, 64, "i32", 33, 11)])
def test_device_answer_sets_feed_minhash(D, nfeat, kind, P, b):
    """the producer -> consumer contract: ascending ids in range, offsets[-1] == len(rows) -- checked by
    ops.minhash(validate=True) on the device CSR, and by the signatures of the reference CSR"""
    cols, idx, pool, qr, ref = case(D, nfeat)
    values = M.table_values(P, D, seed=D + P)
    table = ops.perm_table(values, DEV, force_i32=(kind == "i32"))
    want = M.ref_minhash(ref[0], ref[1], values)
    for one_sweep in (True, False):
        off, rows = answers.answer_sets(idx, qr, one_sweep=one_sweep)
        sig, norm2, keys = ops.minhash(off, rows, table, b=b, validate=True)
        assert np.array_equal(sig.cpu().numpy(), want)
        assert np.array_equal(norm2.cpu().numpy(), M.ref_norm2(want))
        assert np.array_equal(keys.cpu().numpy().view(np.uint64).T, M.ref_band_keys(want, b))
