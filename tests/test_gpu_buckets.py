"""Boundary cases of the candidate-pair path on the GPU: adversarial bucket structures through the partition + overflow
pool + LDS finish (every form: the library picks it from the size and the depth) + block kernel, one and two band
groups, the pair de-duplication on their output and the two forms of pair scoring -- all against the oracle.  The
cases come from tests/bucket_cases.py; every one is checked on the host first, so it cannot quietly stop aiming at its
boundary."""
import numpy as np
import pytest
import torch

import bucket_cases as B

pytestmark = pytest.mark.gpu

from qrlsh import _lib, ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (checker only)

DEV = "cuda"
R = 4


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def coarse_region(nq, c1):
    """records a coarse region of the two-step partition holds (bucket.hip: coarse_region); it does not spill"""
    a = nq / (1 << c1)
    slack = 0.25 * a + 8192.0 if a >= 4096.0 else 6.0 * a ** 0.5 + 2.0 * a + 64.0
    return (int(a + slack) + 63) // 64 * 64


def check_case_on_host(case, count=None, at_least=None):
    """the case is what it says: the depth the library picks for its size, the numpy mixer agrees with the library's
    on the planted keys and a sample of the background, the target part holds `count` (or >= at_least) records, and
    (T > 8) no coarse region of the first partition step overflows -- that would send the whole call to the general
    path by design, and the case would no longer reach the pool and the block kernel"""
    lib = _lib.load()
    b, nq = case.keys.shape
    assert ops.part_bits_for(nq) == case.T, (case.name, ops.part_bits_for(nq))
    if case.T > 8:
        c1 = (case.T + 1) // 2
        for band in range(b):
            assert np.bincount(B.parts_of(case.keys[band], c1)).max() <= coarse_region(nq, c1), (case.name, band)
    sample = [int(k) for k in case.keys[case.band, ::max(1, nq // 97)]] + list(case.hot)
    for k in sample:
        assert int(B.np_mix64(np.array([k], dtype=np.int64).view(np.uint64))[0]) == lib.qrlsh_mix64_host(k)
        if k in case.hot:
            assert lib.qrlsh_mix64_host(k) >> (64 - case.T) == case.part
    parts = B.parts_of(case.keys[case.band], case.T)
    n = int(np.count_nonzero(parts == case.part))
    assert n == case.count
    if count is not None:
        assert n == count, (case.name, n)
    if at_least is not None:
        assert n >= at_least, (case.name, n)


def emit_and_check(case, want_path="partition+lds", dedup=False):
    """emit_pairs_any on the case against the oracle: multiplicity (emitted words) and the sorted unique set;
    dedup: the emitted words through ops.unique_pairs as well.  -> stats"""
    keys = case.keys
    nq = keys.shape[1]
    stats = {}
    emitted = ops.emit_pairs_any(torch.from_numpy(keys).to(DEV), R, stats)
    torch.cuda.synchronize()
    kq = np.ascontiguousarray(keys.T).view(np.uint64)
    want = O.candidates(kq, R)
    assert stats["bucket_path"] == want_path, (case.name, stats)
    assert emitted.numel() == O.emitted_pairs(kq, R), case.name
    assert np.array_equal(O.sort_unique(u64(emitted)), want), case.name
    if dedup:
        st = {}
        pairs = ops.unique_pairs(emitted, nq, st)
        assert st["group_bits"] >= ops.REGION_MIN_GROUP_BITS, st     # the fixed-region grouping ran
        assert np.array_equal(u64(pairs), want), (case.name, st)
        stats.update(st)
        del pairs
    del emitted
    torch.cuda.empty_cache()
    return stats


@pytest.fixture(autouse=True)
def _oracle_threads():
    O.set_threads(min(16, O.max_threads()))


# ---- planted multiplicities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,nq,b,extra,seed", [(8, 900_000, 3, [], 101), (11, 5_500_000, 2, [(25000, 1)], 112),
                                               (12, 10_000_000, 2, [(30000, 1)], 121),
                                               (13, 20_000_000, 1, [(12000, 2)], 131)])
def test_planted_multiplicities(T, nq, b, extra, seed):
    """buckets of 2 .. 9 000 copies (and 12 000 - 30 000 at the deeper partitions) in every band: small parts, parts
    between one image and two, parts of many blocks -- the region prefix, spilled runs and the block kernel at once"""
    case = B.planted_keys(np.random.default_rng(seed), nq, b, B.MIX + extra, T, name="planted T=%d" % T)
    biggest = max(s for s, _ in B.MIX + extra)
    check_case_on_host(case, at_least=biggest)
    emit_and_check(case, dedup=(T == 13))


# ---- several popular keys in one part ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T,nq,sizes,seed", [(12, 10_000_000, [3000, 2500, 900, 5000, 1200], 212),
                                             (11, 5_500_000, [2000, 2100, 1500, 7000], 211),
                                             (8, 1_000_000, [4000, 2500, 800], 208)])
def test_several_popular_keys_in_one_part(T, nq, sizes, seed):
    """one part carries several popular keys: its region prefix, many spilled runs, several blocks of the big kernel"""
    case = B.same_part_keys(np.random.default_rng(seed), nq, T, sizes, name="%d keys in one part, T=%d" % (len(sizes), T))
    check_case_on_host(case, at_least=sum(sizes))
    assert len(set(case.hot)) == len(sizes)
    emit_and_check(case, dedup=(T >= 11))


# ---- a part of exactly N records --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(T, N) for T in (12, 11, 8) for N in B.FILLS[T]])
def test_part_of_exactly_n_records(T, N):
    """parts at the image boundaries: 4095 / 4096 / 4097 (the small-part image and the 12-bit packed count), 6143 /
    6144 / 6145 (the full image and the block size of the big kernel)"""
    case = B.fill_case(T, N)
    nq = case.keys.shape[1]
    if T >= 11:
        assert 1024 <= (nq >> T) <= 2800      # the small-part form of the finish (4096-record image)
    check_case_on_host(case, count=N)
    emit_and_check(case)


# ---- two band groups --------------------------------------------------------------------------------------------------
def test_two_band_groups_with_spills_in_both_stay_exact_and_fast():
    """b * nq >= 2^26: the emit works the bands in two groups on two streams, and a group's gather of spilled runs scans
    the run descriptors while the other group's partition adds to them.  Repeated calls on the same keys (descriptors of
    the previous call still in the workspace) and a call with the overlap off: every one exact and on the fast path."""
    lib = _lib.load()
    case = B.two_group_case()
    b, nq = case.keys.shape
    assert b * nq >= 64 << 20
    check_case_on_host(case, at_least=9000)
    assert np.bincount(B.parts_of(case.keys[0], case.T)).max() > 6144          # and a part beyond the image in group 0
    kq = np.ascontiguousarray(case.keys.T).view(np.uint64)
    want = O.candidates(kq, R)
    n_want = O.emitted_pairs(kq, R)

    def once():
        stats = {}
        emitted = ops.emit_pairs_any(torch.from_numpy(case.keys).to(DEV), R, stats)
        torch.cuda.synchronize()
        assert stats["bucket_path"] == "partition+lds", stats
        assert emitted.numel() == n_want
        assert np.array_equal(O.sort_unique(u64(emitted)), want)
        del emitted
        torch.cuda.empty_cache()

    once()
    once()
    lib.qrlsh_set_overlap(0)
    try:
        once()
    finally:
        lib.qrlsh_set_overlap(1)


# ---- scoring forms ----------------------------------------------------------------------------------------------------
SENT_MILLI = -7777


def _score_raw(sig, norm2, pairs, id_bits):
    """qrlsh_score_pairs with outputs pre-filled with values no score produces (an unwritten entry cannot pass)"""
    lib = _lib.load()
    n = pairs.numel()
    milli = torch.full((n,), SENT_MILLI, dtype=torch.int32, device=DEV)
    cosv = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    edges = torch.full((2 * n,), -1, dtype=torch.int64, device=DEV)
    _lib.check(lib.qrlsh_score_pairs(ops._ptr(sig), _lib.SIG_U16, ops._ptr(norm2), sig.shape[1], ops._ptr(pairs), n,
                                     ops._ptr(milli), ops._ptr(cosv), ops._ptr(edges), id_bits, None, ops._stream()))
    return milli, cosv, edges


def _score_rev_raw(sig, norm2, pairs, id_bits):
    lib = _lib.load()
    n = pairs.numel()
    milli = torch.full((n,), SENT_MILLI, dtype=torch.int32, device=DEV)
    rev = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    _lib.check(lib.qrlsh_score_pairs_rev(ops._ptr(sig), _lib.SIG_U16, ops._ptr(norm2), sig.shape[1], ops._ptr(pairs), n,
                                         ops._ptr(milli), ops._ptr(rev), id_bits, None, ops._stream()))
    return milli, rev


def _score_split_raw(sig_a, norm_a, sig_b, norm_b, pairs):
    lib = _lib.load()
    n = pairs.numel()
    milli = torch.full((n,), SENT_MILLI, dtype=torch.int32, device=DEV)
    _lib.check(lib.qrlsh_score_pairs_split(ops._ptr(sig_a), ops._ptr(norm_a), sig_a.shape[0], ops._ptr(sig_b),
                                           ops._ptr(norm_b), _lib.SIG_U16, sig_a.shape[1], ops._ptr(pairs), n,
                                           ops._ptr(milli), ops._stream()))
    return milli


def _score_pair_lists(rng, nrows):
    """pair lists (i < j, sorted like the pipeline's) that hit the run form's edges"""
    lists = {}
    runs = []
    i = 0
    for L in (1, 15, 16, 17, 33, 1, 16, 33, 15, 17):          # runs of equal i across the 16-pair chunk borders
        js = np.sort(rng.choice(np.arange(i + 1, nrows), size=L, replace=False))
        runs += [(i << 32) | int(j) for j in js]
        i += 1 + int(rng.integers(0, 3))
    lists["runs"] = np.array(runs, dtype=np.uint64)
    for m in range(1, 16):                                    # n = 16 k + m: a last chunk of m pairs
        n = 16 * int(rng.integers(0, 4)) + m
        a = rng.integers(0, nrows - 1, size=n)
        b = rng.integers(0, nrows - 1, size=n)
        lo, hi = np.minimum(a, b), np.maximum(a, b) + 1
        lists["tail%d" % m] = np.sort((lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64))
    a = rng.integers(0, nrows - 1, size=5000)
    b = rng.integers(0, nrows - 1, size=5000)
    lo, hi = np.minimum(a, b), np.maximum(a, b) + 1
    lists["random"] = np.unique((lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64))
    return lists


@pytest.mark.parametrize("P", [128, 256])
def test_score_forms_equal_each_other_and_the_oracle(P):
    """the run form (score_runs_kernel: 16 pairs per lane group, the first row kept while i does not change) and the
    generic form of pair scoring on compact uint16 rows: milli, cos and the edge words bit for bit the same, milli equal
    to the oracle's -- on runs of equal i of 1 / 15 / 16 / 17 / 33 pairs, every n mod 16, identical rows (1000), rows of
    empty answer sets (all -1) and of zeros, values past 2^15; score_pairs_split and score_pairs_rev likewise; and a
    sig at an odd element offset (the unaligned fallback in both settings)"""
    lib = _lib.load()
    rng = np.random.default_rng(P)
    nrows = 3000
    s32 = rng.integers(0, 65535, size=(nrows, P)).astype(np.int32)
    s32[rng.random((nrows, P)) < 0.1] = -1
    s32[10:1010] = s32[5]                 # 1000 identical rows (and row 5): scores of 1000
    s32[1100:1120] = -1                   # empty answer sets
    s32[1120:1130] = 0                    # zero norm
    s32[1130:1200] = rng.integers(0, 1 << 15, size=(70, P))
    pairs_all = _score_pair_lists(rng, nrows)
    ident = np.array([(5 << 32) | j for j in range(10, 1010)] + [(i << 32) | (i + 1) for i in range(10, 1009)] +
                     [(i << 32) | j for i in range(1095, 1135) for j in range(i + 1, 1135)], dtype=np.uint64)
    pairs_all["identical_empty_zero"] = ident
    s16 = np.where(s32 < 0, 0xFFFF, s32).astype(np.uint16).view(np.int16)
    sig = torch.from_numpy(s16).to(DEV)
    norm2 = ops.row_norms(torch.from_numpy(s32).to(DEV))
    odd_buf = torch.empty((nrows * P + 1,), dtype=torch.int16, device=DEV)
    sig_odd = odd_buf[1:].view(nrows, P)
    sig_odd.copy_(sig)
    assert sig_odd.data_ptr() % 16 != 0
    split = 1500
    sig_a, sig_b = sig[:split].clone(), sig[split:].clone()
    norm_a, norm_b = norm2[:split].clone(), norm2[split:].clone()
    id_bits = 12
    old = lib.qrlsh_set_score_runs(1)
    try:
        for name, hp in pairs_all.items():
            pairs = torch.from_numpy(hp.view(np.int64)).to(DEV)
            m_ref, c_ref = O.score_pairs(s32, hp, mode=1, want_cos=True)
            got = {}
            for runs in (1, 0):
                lib.qrlsh_set_score_runs(runs)
                milli, cosv, edges = _score_raw(sig, norm2, pairs, id_bits)
                mr, rev = _score_rev_raw(sig, norm2, pairs, id_bits)
                ms = _score_split_raw(sig_a, norm_a, sig_b, norm_b, pairs)
                mo, co, eo = _score_raw(sig_odd, norm2, pairs, id_bits)
                torch.cuda.synchronize()
                got[runs] = [t.cpu().numpy() for t in (milli, cosv.view(torch.int64), edges, mr, rev, ms, mo,
                                                      co.view(torch.int64), eo)]
                assert np.array_equal(got[runs][0], m_ref), (name, runs, P)
                assert np.array_equal(cosv.cpu().numpy(), c_ref), (name, runs, P)
                for k in (3, 5, 6):
                    assert np.array_equal(got[runs][k], m_ref), (name, runs, P, k)
            for k, (a, b) in enumerate(zip(got[1], got[0])):
                assert np.array_equal(a, b), (name, P, k)
            if name == "identical_empty_zero":
                assert np.all(got[1][0][:1999] == 1000)
    finally:
        lib.qrlsh_set_score_runs(old if old >= 0 else 1)
