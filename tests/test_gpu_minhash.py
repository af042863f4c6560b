"""The kernels of csrc/minhash.hip against the plain references of tests/minhash_cases.py, bit for bit: every
instantiation of the group kernel and the wave-per-query kernel at the set sizes where their loops turn, both sides of
the switch between them, the fused and the standalone band keys (packed and hashed), the norms, the compact rows, the
stores at the end of a row, and the CSR check.  Every comparison is exact and covers whole outputs."""
import numpy as np
import pytest
import torch

import minhash_cases as M

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402

DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def make_table(values, kind):
    table = ops.perm_table(values, DEV, force_i32=(kind == "i32"))
    assert table.code == (_lib.PERM_I32 if kind == "i32" else _lib.PERM_U16)
    return table


def check_minhash(off, rows, table, ref, bands, what):
    """ops.minhash in every combination of its optional outputs against the reference signatures `ref`"""
    d_off, d_rows = dev(off), dev(rows)
    want_sig = torch.from_numpy(ref.astype(np.int32))
    want_norm = torch.from_numpy(M.ref_norm2(ref))
    forms = [False] + ([True] if ops.can_compact(table) else [])
    for compact in forms:
        def same_sig(sig):
            if compact:
                assert sig.dtype == torch.int16
            return torch.equal(ops.sig_to_int32(sig).cpu(), want_sig)
        for b in bands:
            sig, norm2, keys = ops.minhash(d_off, d_rows, table, b=b, compact=compact)
            assert same_sig(sig), (what, b, compact)
            assert torch.equal(norm2.cpu(), want_norm), (what, b, compact)
            assert np.array_equal(u64(keys).T, M.ref_band_keys(ref, b)), (what, b, compact)
            sig, norm2, keys = ops.minhash(d_off, d_rows, table, b=b, want_norm=False, compact=compact)
            assert norm2 is None and same_sig(sig), (what, b, compact)
            assert np.array_equal(u64(keys).T, M.ref_band_keys(ref, b)), (what, b, compact)
        sig, norm2, keys = ops.minhash(d_off, d_rows, table, b=None, compact=compact)
        assert keys is None and same_sig(sig) and torch.equal(norm2.cpu(), want_norm), (what, compact)
        sig, norm2, keys = ops.minhash(d_off, d_rows, table, b=None, want_norm=False, compact=compact)
        assert keys is None and norm2 is None and same_sig(sig), (what, compact)


SHAPE_PARAMS = [(kind, P, bands, plain, keyed) for kind in ("u16", "i32") for P, bands, plain, keyed in M.SHAPES[kind]]


# ---------------------------------------------------------------------------- forms x set sizes
@pytest.mark.parametrize("kind,P,bands,plain,keyed", SHAPE_PARAMS, ids=["%s-P%d" % (k, p) for k, p, *_ in SHAPE_PARAMS])
def test_every_form_at_its_set_size_edges(kind, P, bands, plain, keyed):
    D, nq = 1500, 131
    values = M.table_values(P, D, seed=P)
    table = make_table(values, kind)
    assert ops.can_compact(table) == (kind == "u16")
    # the set sizes of the form that runs without keys and (where it differs) of the one that runs with keys
    for form in dict.fromkeys((plain, keyed)):
        LPR = 64 if form == M.WAVE_PER_QUERY else form
        off, rows = M.shuffled_sizes(LPR, nq, D, seed=1000 + P + (7 if form == M.WAVE_PER_QUERY else 0))
        check_minhash(off, rows, table, M.ref_minhash(off, rows, values), bands, (kind, P, form))


# ---------------------------------------------------------------------------- nq edges
@pytest.mark.parametrize("kind,P", [(k, p) for k in ("u16", "i32") for p in M.NQ_EDGE_P[k]])
def test_nq_edges_with_lonely_empty_and_whole_table_sets(kind, P):
    b = next(b for pp, bands, *_ in M.SHAPES[kind] if pp == P for b in bands)
    D, Dsmall = 1200, 97
    values, small = M.table_values(P, D, seed=P + 1), M.table_values(P, Dsmall, seed=P + 2)
    table, tsmall = make_table(values, kind), make_table(small, kind)
    for nq in M.NQ_EDGES:
        for name, (off, rows), tab, vals in (("lonely_long", M.lonely_long(nq, D, seed=nq), table, values),
                                             ("all_empty", M.all_empty(nq), table, values),
                                             ("whole_table", M.whole_table(nq, Dsmall), tsmall, small)):
            ref = M.ref_minhash(off, rows, vals)
            sig, norm2, keys = ops.minhash(dev(off), dev(rows), tab, b=b)
            assert np.array_equal(sig.cpu().numpy(), ref), (name, nq)
            assert np.array_equal(norm2.cpu().numpy(), M.ref_norm2(ref)), (name, nq)
            assert np.array_equal(u64(keys).T, M.ref_band_keys(ref, b)), (name, nq)
            sig2, _, _ = ops.minhash(dev(off), dev(rows), tab, b=None, want_norm=False)
            assert np.array_equal(sig2.cpu().numpy(), ref), (name, nq)
            if name == "all_empty":
                assert np.all(ref == -1) and np.all(u64(keys) == np.uint64(ops_empty_key(P // b)))


def ops_empty_key(r):
    return M.M64 if r >= 4 else (1 << (16 * r)) - 1


# ---------------------------------------------------------------------------- the switch between the two kernels
@pytest.mark.parametrize("P", [510, 511, 512])
def test_key_image_switch_gives_the_same_signatures_and_norms(P):
    """uint16 table: 510 runs the group kernel either way, 511 and 512 run it without keys and the wave-per-query
    kernel with keys (tests/minhash_cases.py states the rule)"""
    assert M.expected_form("u16", P, False) == 64
    assert M.expected_form("u16", P, True) == (64 if P == 510 else M.WAVE_PER_QUERY)
    D, nq = 1500, 131
    values = M.table_values(P, D, seed=P + 7)
    table = make_table(values, "u16")
    off, rows = M.shuffled_sizes(64, nq, D, seed=P + 8)
    ref = M.ref_minhash(off, rows, values)
    b = next(b for pp, bands, *_ in M.U16_SHAPES if pp == P for b in bands)
    s_keys, n_keys, keys = ops.minhash(dev(off), dev(rows), table, b=b)
    s_plain, n_plain, _ = ops.minhash(dev(off), dev(rows), table, b=None)
    assert torch.equal(s_keys, s_plain) and torch.equal(n_keys, n_plain)
    assert np.array_equal(s_keys.cpu().numpy(), ref) and np.array_equal(n_keys.cpu().numpy(), M.ref_norm2(ref))
    assert np.array_equal(u64(keys).T, M.ref_band_keys(ref, b))


def test_lane_switch_of_the_int32_table_256_against_257():
    """int32 table: P = 256 is 64 lanes (the group kernel), P = 257 is 65 (the wave-per-query kernel with its column
    loop); the first 256 columns are the same table, so they must give the same signatures"""
    assert M.expected_form("i32", 256, True) == 64 and M.expected_form("i32", 257, True) == M.WAVE_PER_QUERY
    D, nq = 1500, 131
    values = M.table_values(257, D, seed=5)
    off, rows = M.shuffled_sizes(64, nq, D, seed=6)
    ref = M.ref_minhash(off, rows, values)
    s257, n257, k257 = ops.minhash(dev(off), dev(rows), make_table(values, "i32"), b=1)
    s256, n256, k256 = ops.minhash(dev(off), dev(rows), make_table(values[:256], "i32"), b=1)
    assert np.array_equal(s257.cpu().numpy(), ref) and np.array_equal(s256.cpu().numpy(), ref[:, :256])
    assert np.array_equal(n257.cpu().numpy(), M.ref_norm2(ref)) and np.array_equal(n256.cpu().numpy(), M.ref_norm2(ref[:, :256]))
    assert np.array_equal(u64(k257).T, M.ref_band_keys(ref, 1)) and np.array_equal(u64(k256).T, M.ref_band_keys(ref[:, :256], 1))


# ---------------------------------------------------------------------------- D edges
def test_d_65535_is_the_largest_table_with_compact_rows():
    D, P = 65535, 16
    values = M.table_values(P, D, seed=11)
    assert values.max() == 65534
    table = make_table(values, "u16")
    assert ops.can_compact(table)
    off, rows = M.shuffled_sizes(4, 131, D, seed=12)
    sets = [rows[off[q]:off[q + 1]] for q in range(131)] + [np.array([0], np.int32), np.array([D - 1], np.int32)]
    off, rows = M.csr_of(sets)          # (row D - 1 alone: column 1 holds 65 534 there, column 0 holds it at row 0)
    ref = M.ref_minhash(off, rows, values)
    assert ref.max() == 65534
    check_minhash(off, rows, table, ref, (4, 2), "D=65535")


def test_d_65536_where_65535_is_a_value_and_the_padding_and_minus_one():
    D, P = 65536, 16
    values = M.table_values(P, D, seed=13)
    values[4:8, 777] = 65535            # one row holds 65 535 in every column of band 1 (b = 4) ...
    values[8:, 777] = np.arange(8)      # ... and small values elsewhere
    table = make_table(values, "u16")
    assert table.code == _lib.PERM_U16 and not ops.can_compact(table)
    off, rows = M.shuffled_sizes(4, 131, D, seed=14)
    sets = [rows[off[q]:off[q + 1]] for q in range(131)]
    sets[64:64] = [np.array([777], np.int32), np.zeros(0, np.int32), np.array([D - 1], np.int32)]
    off, rows = M.csr_of(sets)
    ref = M.ref_minhash(off, rows, values)
    assert ref.max() == 65535 and np.all(ref[64, 4:8] == 65535) and np.all(ref[65] == -1)
    assert M.ref_norm2(ref)[64] != M.ref_norm2(ref)[65]
    kref = M.ref_band_keys(ref, 4)
    assert kref[64, 1] == kref[65, 1] == np.uint64(M.M64) and kref[64, 2] != kref[65, 2]    # as the low-16 image has it
    check_minhash(off, rows, table, ref, (4, 2, 8), "D=65536")
    with pytest.raises(ValueError):
        ops.minhash(dev(off), dev(rows), table, b=4, compact=True)


def test_d_65537_takes_the_int32_table_and_keys_take_the_low_16_bits():
    D, P = 65537, 12
    values = M.table_values(P, D, seed=15)
    table = ops.perm_table(values, DEV)
    assert table.code == _lib.PERM_I32 and not ops.can_compact(table)
    off, rows = M.shuffled_sizes(4, 131, D, seed=16)
    sets = [rows[off[q]:off[q + 1]] for q in range(131)] + [np.array([D - 1], np.int32), np.array([0], np.int32)]
    off, rows = M.csr_of(sets)
    ref = M.ref_minhash(off, rows, values)
    assert ref.max() == 65536 and ref[131, 1] == 65536 and M.ref_band_keys(ref, 12)[131, 1] == 0
    check_minhash(off, rows, table, ref, (3, 12, 2), "D=65537")


# ---------------------------------------------------------------------------- the 24-bit guard
@pytest.mark.parametrize("D", [1 << 24, (1 << 24) + 1])
def test_row_ids_at_the_24_bit_guard(D):
    """D = 2^24 is the last table the group kernel takes (its row offset is a 24-bit multiply), D = 2^24 + 1 goes to the
    wave-per-query kernel; row ids 0, 2^24 - 1 and 2^24 are gathered alone and inside larger sets.
    NOT covered: the other guard of that switch, the 32-bit byte offset (D * P_stride * element size < 2^32) -- a 4 GiB
    table is too heavy for a unit test."""
    P = 4
    assert M.expected_form("i32", P, True, D=D) == (4 if D == 1 << 24 else M.WAVE_PER_QUERY)
    rng = np.random.default_rng(D & 0xFF)
    values = rng.integers(0, 1 << 30, size=(P, D), dtype=np.int32)      # arbitrary values (norms stay below 2^63)
    edges = [0, (1 << 24) - 1] + ([1 << 24] if D > 1 << 24 else [])
    sets = [np.array([e], np.int32) for e in edges] + [np.array(edges, np.int32)]
    for q in range(66):
        ids = rng.choice(D, size=int(rng.integers(0, 40)), replace=False)
        if q % 2:
            ids = np.concatenate([ids, edges])
        sets.append(np.unique(ids).astype(np.int32))
    off, rows = M.csr_of(sets)
    ref = M.ref_minhash(off, rows, values)
    for q, e in enumerate(edges):
        assert np.array_equal(ref[q], values[:, e])
    table = ops.perm_table(values, DEV)
    assert table.code == _lib.PERM_I32 and table.P_stride == 4
    sig, norm2, keys = ops.minhash(dev(off), dev(rows), table, b=2, validate=True)
    assert np.array_equal(sig.cpu().numpy(), ref)
    assert np.array_equal(norm2.cpu().numpy(), M.ref_norm2(ref))
    assert np.array_equal(u64(keys).T, M.ref_band_keys(ref, 2))
    sig, _, _ = ops.minhash(dev(off), dev(rows), table, b=None, want_norm=False, validate=True)
    assert np.array_equal(sig.cpu().numpy(), ref)


# ---------------------------------------------------------------------------- no byte outside the outputs
@pytest.mark.parametrize("kind,compact", [("u16", False), ("u16", True), ("i32", False)])
@pytest.mark.parametrize("P,b", [(5, 5), (12, 4), (100, 20), (128, 32)])
def test_out_slices_keep_their_neighbours(P, b, kind, compact):
    D, nq = 1500, 67
    values = M.table_values(P, D, seed=P + 20)
    table = make_table(values, kind)
    off, rows = M.shuffled_sizes(8, nq, D, seed=P + 21)
    ref = M.ref_minhash(off, rows, values)
    PAD = 64                                           # elements: 128 bytes or more, so the slices start 16-byte aligned
    sdt, s_fill = (torch.int16, 0x5A5A) if compact else (torch.int32, 0x5A5A5A5A)
    n_fill, k_fill = 0x5A5A5A5A5A5A5A5A, -0x2525252525252526
    sig_buf = torch.full((PAD + nq * P + PAD,), s_fill, dtype=sdt, device=DEV)
    norm_buf = torch.full((PAD + nq + PAD,), n_fill, dtype=torch.int64, device=DEV)
    key_buf = torch.full((3, b, nq), k_fill, dtype=torch.int64, device=DEV)
    sig = sig_buf[PAD:PAD + nq * P].view(nq, P)
    norm2 = norm_buf[PAD:PAD + nq]
    keys = key_buf[1]
    assert sig.data_ptr() % 16 == 0 and norm2.data_ptr() % 16 == 0
    got = ops.minhash(dev(off), dev(rows), table, b=b, compact=compact, out=(sig, norm2, keys))
    assert got[0] is sig and got[1] is norm2 and got[2] is keys
    assert np.array_equal(ops.sig_to_int32(sig).cpu().numpy(), ref)
    assert np.array_equal(norm2.cpu().numpy(), M.ref_norm2(ref))
    assert np.array_equal(u64(keys).T, M.ref_band_keys(ref, b))
    for buf, fill, inner in ((sig_buf, s_fill, nq * P), (norm_buf, n_fill, nq)):
        assert torch.all(buf[:PAD] == fill) and torch.all(buf[PAD + inner:] == fill)
    assert torch.all(key_buf[0] == k_fill) and torch.all(key_buf[2] == k_fill)
    # signatures alone, and signatures + norms, into the same slices
    sig_buf.fill_(s_fill)
    ops.minhash(dev(off), dev(rows), table, b=None, want_norm=False, compact=compact, out=(sig, None, None))
    assert np.array_equal(ops.sig_to_int32(sig).cpu().numpy(), ref)
    assert torch.all(sig_buf[:PAD] == s_fill) and torch.all(sig_buf[PAD + nq * P:] == s_fill)


# ---------------------------------------------------------------------------- standalone band keys
def _signature_matrix(rng, nq, P):
    """int32 signatures with everything the key kernels must not trip over: values at and above 65 536, rows of -1,
    single bands of -1, and 65 535 (whose low-16 image is that of -1)"""
    sig = rng.integers(0, 200000, size=(nq, P)).astype(np.int32)
    sig[rng.random((nq, P)) < 0.05] = -1
    sig[rng.random((nq, P)) < 0.03] = 65535
    sig[::5] = -1
    if nq > 1:
        sig[1, : max(1, P // 2)] = -1
    if nq > 2:
        sig[2] = sig[nq - 1]
    return sig


@pytest.mark.parametrize("P", [5, 96, 128, 254, 255, 520, 1022, 1023])
def test_standalone_band_keys_and_norms_around_the_workgroup_size(P):
    qpb = M.band_keys_qpb(P)
    rng = np.random.default_rng(P)
    rs = list(dict.fromkeys([r for r in range(1, 9) if P % r == 0] + [P]))
    for nq in (qpb - 1, qpb, qpb + 1, 2 * qpb + 3):
        sig = _signature_matrix(rng, nq, P)
        d_sig = dev(sig)
        for r in rs:
            b = P // r
            keys, norm2 = ops.band_keys(d_sig, b, want_norm=True)
            assert np.array_equal(u64(keys).T, M.ref_band_keys(sig, b)), (P, nq, r)
            assert np.array_equal(norm2.cpu().numpy(), M.ref_norm2(sig)), (P, nq, r)
            assert torch.equal(ops.band_keys(d_sig, b), keys)


@pytest.mark.parametrize("kind,P,bands", [("u16", 100, (20, 25, 1)), ("u16", 520, (65, 104)), ("i32", 96, (12, 24, 96)),
                                          ("i32", 260, (52, 1))])
def test_fused_keys_equal_standalone_keys(kind, P, bands):
    D, nq = 70000 if kind == "i32" else 1500, 131
    values = M.table_values(P, D, seed=P + 30)
    table = make_table(values, kind)
    off, rows = M.shuffled_sizes(16, nq, D, seed=P + 31)
    for b in bands:
        sig, norm2, keys = ops.minhash(dev(off), dev(rows), table, b=b)
        k2, n2 = ops.band_keys(sig, b, want_norm=True)
        assert torch.equal(k2, keys) and torch.equal(n2, norm2)
        assert torch.equal(ops.row_norms(sig), norm2)


# ---------------------------------------------------------------------------- row norms
@pytest.mark.parametrize("P", [1, 63, 64, 65, 2047, 2048, 2049])
def test_row_norms_both_kernels(P):
    rng = np.random.default_rng(P)
    nq = 37
    sig = rng.integers(-(1 << 20), 1 << 20, size=(nq, P)).astype(np.int32)
    sig[3] = 0
    sig[4] = -1
    sig[5] = 0                           # +-(2^31 - 1) in two columns: 2 (2^31 - 1)^2 < 2^63
    sig[5, 0] = (1 << 31) - 1
    sig[5, P - 1] = -((1 << 31) - 1)
    want = M.ref_norm2(sig)
    assert want[5] == (2 if P > 1 else 1) * ((1 << 31) - 1) ** 2
    assert np.array_equal(ops.row_norms(dev(sig)).cpu().numpy(), want)


def test_row_norms_wave_form_takes_a_second_trip():
    """one wave per row in at most 8192 workgroups of 4 waves: rows 32 768 and up are a wave's second row"""
    nq, P = 32769 + 5, 64
    rng = np.random.default_rng(1)
    sig = rng.integers(-70000, 70000, size=(nq, P)).astype(np.int32)
    assert np.array_equal(ops.row_norms(dev(sig)).cpu().numpy(), M.ref_norm2(sig))


def test_row_norms_workgroup_form_takes_a_second_trip():
    """one workgroup per row in at most 65 536 workgroups: rows 65 536 and up are a workgroup's second row.  The
    matrix is a block of 4099 distinct rows repeated on the device; the reference is computed once for the block."""
    nq, P, nblock = 65536 + 3, 2048, 4099
    rng = np.random.default_rng(2)
    block = rng.integers(-70000, 70000, size=(nblock, P)).astype(np.int32)
    reps = (nq + nblock - 1) // nblock
    sig = dev(block).repeat(reps, 1)[:nq]
    assert sig.is_contiguous() and tuple(sig.shape) == (nq, P)
    want = np.tile(M.ref_norm2(block), reps)[:nq]
    got = ops.row_norms(sig).cpu().numpy()
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------- the CSR check
def raw_flags(off, rows, D):
    lib = _lib.load()
    d_off, d_rows = dev(np.asarray(off, np.int64)), dev(np.asarray(rows, np.int32))
    flags = torch.full((1,), 0x55, dtype=torch.int32, device=DEV)      # the entry point clears it itself
    _lib.check(lib.qrlsh_check_csr(ops._ptr(d_off), ops._ptr(d_rows) if len(rows) else None, len(off) - 1, len(rows), int(D),
                                   ops._ptr(flags), ops._stream()))
    return int(flags.item())


def check_both_ways(off, rows, D, want):
    assert M.ref_check_csr(off, rows, D) == want
    assert raw_flags(off, rows, D) == want
    d_off, d_rows = dev(np.asarray(off, np.int64)), dev(np.asarray(rows, np.int32))
    if want == 0:
        ops.check_csr(d_off, d_rows, D)
        return
    with pytest.raises(ValueError) as e:
        ops.check_csr(d_off, d_rows, D)
    msg = str(e.value)
    assert ("offsets[0]" in msg) == bool(want & M.CSR_BAD_ENDS)
    assert ("offsets decrease" in msg) == bool(want & M.CSR_DECREASING)
    assert ("row id outside" in msg) == bool(want & M.CSR_ROW_RANGE)


def _good_csr(rng, nq, nnz, D):
    cuts = np.sort(rng.integers(0, nnz + 1, size=nq - 1)) if nq > 1 else np.zeros(0, np.int64)
    off = np.concatenate([[0], cuts, [nnz]]).astype(np.int64)
    rows = rng.integers(0, D, size=nnz).astype(np.int32)
    if nnz:
        rows[0] = D - 1                  # the largest legal id is accepted
        rows[-1] = 0
    return off, rows


def test_check_csr_accepts_good_inputs_of_every_proportion():
    rng = np.random.default_rng(0)
    D = 1000
    for nq, nnz in [(3, 5000), (5000, 3), (700, 0), (1, 1), (256, 256), (257, 255)]:
        off, rows = _good_csr(rng, nq, nnz, D)
        check_both_ways(off, rows, D, 0)
        if nnz:
            rows[:] = D - 1
            check_both_ways(off, rows, D, 0)


@pytest.mark.parametrize("at", [0, 255, 256, 257, -1])
def test_check_csr_finds_a_single_fault_wherever_it_sits(at):
    """a thread per element in workgroups of 256: the fault sits in the first thread, at both sides of the first
    workgroup's end, and in the last element"""
    rng = np.random.default_rng(1)
    D, nq, nnz = 1000, 600, 900
    off, rows = _good_csr(rng, nq, nnz, D)
    off[1:-1] = np.maximum(off[1:-1], 1)
    off[1:-1] = np.minimum(off[1:-1], nnz - 1)         # room to move any inner offset by one
    check_both_ways(off, rows, D, 0)
    k = at % nnz
    for bad in (D, -1, D + 1, -(1 << 31), (1 << 31) - 1):
        r2 = rows.copy()
        r2[k] = bad
        check_both_ways(off, r2, D, M.CSR_ROW_RANGE)
    r2 = rows.copy()
    r2[k] = D - 1
    check_both_ways(off, r2, D, 0)
    # offsets[t + 1] < offsets[t] at t = `at`: by lowering offsets[1] below 0 at t = 0, by raising offsets[t] elsewhere
    t = at % nq
    o2 = off.copy()
    if t == 0:
        o2[1] = -1
    else:
        o2[t] = o2[t + 1] + 1
    check_both_ways(o2, rows, D, M.CSR_DECREASING)


def test_check_csr_ends_and_two_faults_at_once():
    rng = np.random.default_rng(2)
    D, nq, nnz = 50, 300, 700
    off, rows = _good_csr(rng, nq, nnz, D)
    off[1:-1] = np.maximum(off[1:-1], 1)
    o2 = off.copy()
    o2[0] = 1
    check_both_ways(o2, rows, D, M.CSR_BAD_ENDS)
    for last in (nnz - 1, nnz + 1):
        o2 = off.copy()
        o2[1:] = np.minimum(o2[1:], last)
        o2[-1] = last
        check_both_ways(o2, rows, D, M.CSR_BAD_ENDS)
    o2, r2 = off.copy(), rows.copy()
    o2[0] = 1
    r2[nnz // 2] = D
    check_both_ways(o2, r2, D, M.CSR_BAD_ENDS | M.CSR_ROW_RANGE)
    o2 = off.copy()
    o2[200] = o2[201] + 1
    check_both_ways(o2, r2, D, M.CSR_DECREASING | M.CSR_ROW_RANGE)
    o2[0] = 1
    check_both_ways(o2, r2, D, 7)
