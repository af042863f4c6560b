"""The references and case builders of tests/minhash_cases.py hold (no GPU): against the oracle where the oracle
reaches, against a second scalar statement of the wide-band hash where it does not, and against the library's host
export of the mixer.  The shape tables follow from the lane arithmetic they state."""
import numpy as np
import pytest

import minhash_cases as M
from oracle import oracle as O  # checker only


def _cases(D):
    return [("shuffled_4", M.shuffled_sizes(4, 40, D, seed=1)), ("shuffled_16", M.shuffled_sizes(16, 40, D, seed=2)),
            ("lonely", M.lonely_long(33, D, seed=3, n=min(1000, D))), ("empty", M.all_empty(17)),
            ("whole", M.whole_table(5, D))]


def test_ref_minhash_equals_both_oracles_on_true_permutations():
    P, D = 7, 120
    perm = O.legacy_permutations(5, P, D)
    for name, (off, rows) in _cases(D):
        want = O.minhash(off, rows, perm)
        got = M.ref_minhash(off, rows, perm)
        assert got.dtype == np.int64 and np.array_equal(got, want), name
        assert np.array_equal(got, O.naive_minhash(off, rows, perm)), name
    # a larger table through the C oracle alone (the naive one is quadratic)
    P, D = 20, 1500
    perm = O.legacy_permutations(6, P, D)
    for name, (off, rows) in _cases(D):
        assert np.array_equal(M.ref_minhash(off, rows, perm), O.minhash(off, rows, perm)), name


def test_case_builders_are_what_they_say():
    D = 1500
    for LPR in (4, 8, 16, 32, 64):
        sizes = M.set_sizes(LPR)
        assert len(sizes) == len(set(sizes)) and {0, 1, LPR - 1, LPR, LPR + 1, 2 * LPR + 1, 3 * LPR + 2, 1000} <= set(sizes)
        off, rows = M.shuffled_sizes(LPR, 131, D, seed=LPR)
        assert M.ref_check_csr(off, rows, D) == 0
        n = np.diff(off)
        assert set(n.tolist()) == set(sizes)                     # every size occurs
        for w in range(0, 131 - 16, 16):                         # every full wave mixes empty, short and long sets
            assert n[w:w + 16].min() <= 1 and n[w:w + 16].max() >= 2 * LPR
        assert rows.min() == 0 and rows.max() == D - 1
        for q in range(131):                                     # ascending and distinct: well-formed answer sets
            assert np.all(np.diff(rows[off[q]:off[q + 1]]) > 0)
    for nq in M.NQ_EDGES:
        off, rows = M.lonely_long(nq, D, seed=nq)
        n = np.diff(off)
        assert set(n.tolist()) <= {0, 1000} and n.max() == 1000 and rows.min() == 0 and rows.max() == D - 1
        for w in range(0, nq - 15, 16):
            assert np.count_nonzero(n[w:w + 16]) == 1
        off, rows = M.all_empty(nq)
        assert len(off) == nq + 1 and not off.any() and len(rows) == 0
        off, rows = M.whole_table(nq, 97)
        assert np.all(np.diff(off) == 97) and rows.min() == 0 and rows.max() == 96
    tab = M.table_values(9, 65536, seed=0)
    assert tab.min() == 0 and tab.max() == 65535 and tab.dtype == np.int64


@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_ref_band_keys_equals_oracle_for_packed_bands(r):
    rng = np.random.default_rng(r)
    b = 6
    sig = rng.integers(-1, 70000, size=(50, b * r)).astype(np.int32)
    sig[3] = -1
    sig[4, :r] = -1
    sig[5] = 65535
    got = M.ref_band_keys(sig, b)
    assert got.dtype == np.uint64 and np.array_equal(got, O.band_keys(sig, b))
    empty = (1 << (16 * r)) - 1
    assert np.all(got[3] == empty) and got[4, 0] == empty and np.all(got[5] == empty)


@pytest.mark.parametrize("r", [5, 6, 16])
def test_ref_band_keys_equals_scalar_loop_for_wide_bands(r):
    rng = np.random.default_rng(r)
    b = 3
    sig = rng.integers(-1, 70000, size=(40, b * r)).astype(np.int32)
    sig[0] = -1                         # every band empty
    sig[1] = -1
    sig[1, r] = 7                       # band 1: one value that is not -1
    sig[2] = sig[7]                     # equal tuples
    sig[3, :r] = 65535                  # the low-16 image of -1: the same key as the empty band
    got = M.ref_band_keys(sig, b)
    for q in range(len(sig)):
        for band in range(b):
            assert int(got[q, band]) == M.scalar_band_key(sig[q, band * r:(band + 1) * r]), (q, band)
    assert np.all(got[0] == np.uint64(M.M64))
    assert got[1, 0] == np.uint64(M.M64) and got[1, 1] != np.uint64(M.M64) and got[1, 2] == np.uint64(M.M64)
    assert np.array_equal(got[2], got[7]) and got[3, 0] == np.uint64(M.M64)
    assert len(np.unique(got[8:])) == got[8:].size        # distinct random tuples: distinct keys
    with pytest.raises(ValueError):
        O.band_keys(sig, b)                               # (the oracle refuses wide bands: hence this reference)


def test_ref_mixer_equals_the_library_host_export():
    from qrlsh import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    vals = np.concatenate([rng.integers(0, 1 << 63, size=300, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                           np.array([0, 1, M.M64, M.M64 - 1, M.HASH_SEED, 1 << 63], dtype=np.uint64)])
    got = M.ref_mix64(vals)
    for v, g in zip(vals.tolist(), got.tolist()):
        assert lib.qrlsh_mix64_host(v) == g


def test_ref_check_csr_on_hand_written_inputs():
    good_off, good_rows = [0, 2, 2, 5], [3, 15, 0, 7, 9]
    assert M.ref_check_csr(good_off, good_rows, 16) == 0
    assert M.ref_check_csr([0], [], 1) == 0 and M.ref_check_csr([0, 0, 0], [], 4) == 0
    assert M.ref_check_csr(good_off, [3, 16, 0, 7, 9], 16) == M.CSR_ROW_RANGE
    assert M.ref_check_csr(good_off, [3, -1, 0, 7, 9], 16) == M.CSR_ROW_RANGE
    assert M.ref_check_csr(good_off, good_rows, 15) == M.CSR_ROW_RANGE          # D - 1 is the largest legal id
    assert M.ref_check_csr([0, 3, 2, 5], good_rows, 16) == M.CSR_DECREASING
    assert M.ref_check_csr([1, 2, 2, 5], good_rows, 16) == M.CSR_BAD_ENDS
    assert M.ref_check_csr([0, 2, 2, 4], good_rows, 16) == M.CSR_BAD_ENDS
    assert M.ref_check_csr([0, 2, 1, 4], [3, 99, 0, 7, 9], 16) == 7


def test_shape_tables_follow_from_the_lane_arithmetic():
    assert [p for p, *_ in M.U16_SHAPES] == [5, 12, 32, 33, 64, 65, 100, 128, 129, 256, 257, 260, 510, 511, 512, 513, 520]
    assert [p for p, *_ in M.I32_SHAPES] == [5, 16, 17, 32, 33, 64, 65, 100, 128, 129, 256, 257, 260]
    rs, forms = set(), {"u16": set(), "i32": set()}
    for kind, shapes in M.SHAPES.items():
        for P, bands, plain, keyed in shapes:
            assert plain == M.expected_form(kind, P, False) and keyed == M.expected_form(kind, P, True), (kind, P)
            assert bands and all(P % b == 0 for b in bands), (kind, P)
            if all(P % k for k in range(2, P)):
                assert sorted(bands) == [1, P], (kind, P)            # a prime P: b = 1 and b = P
            rs |= {P // b for b in bands}
            forms[kind] |= {plain, keyed}
        assert forms[kind] == {4, 8, 16, 32, 64, M.WAVE_PER_QUERY}
        assert {M.expected_form(kind, P, True) for P in M.NQ_EDGE_P[kind]} == {4, 8, 16, 32, 64, M.WAVE_PER_QUERY}
    assert {1, 2, 3, 4, 5, 8} <= rs
    assert any(1 in bands for _, bands, *_ in M.U16_SHAPES) and any(P in bands for P, bands, *_ in M.U16_SHAPES)
    # the key-image switch sits between 510 and 511, the 24-bit switch between 2^24 and 2^24 + 1
    assert 64 * (510 + 2) * 2 == 65536
    assert M.expected_form("i32", 4, True, D=1 << 24) == 4
    assert M.expected_form("i32", 4, True, D=(1 << 24) + 1) == M.WAVE_PER_QUERY
    assert [M.band_keys_qpb(P) for P in (5, 96, 128, 254, 255, 520, 1022, 1023)] == [64, 64, 64, 64, 32, 16, 16, 8]
