"""References and case builders for the front of the pipeline (csrc/minhash.hip): MinHash signatures, their squared
norms, the band keys (packed for r <= 4, hashed beyond) and the CSR precondition check.  Shared by
tests/test_minhash_host.py (the references hold, no GPU) and tests/test_gpu_minhash.py (the kernels against them).

Pure numpy: nothing here needs the library, torch or a GPU.  The references are written for clarity and use only
int64 / uint64 arrays or Python integers.

WHICH KERNEL A SHAPE RUNS (launch_minhash, stated once here -- move the cases below when that rule moves):
  * one lane holds 16 bytes of a table row: 8 uint16 or 4 int32 values, so lanes = ceil(P / 8) or ceil(P / 4);
  * the group kernel minhash_group_kernel<TabT, LPR> runs with LPR = 4 / 8 / 16 / 32 / 64 for up to that many lanes;
  * the wave-per-query kernel minhash_kernel runs when lanes > 64, or WITH KEYS once the group kernel's key image
    64 * (P + 2) * 2 bytes exceeds 65 536 (P > 510), or when D > 2^24, or when the table reaches 4 GiB.
"""
import numpy as np

WAVE_PER_QUERY = "wave-per-query"
MH_CH = 4                      # table rows gathered per sub-step of the group kernel
GROUP_KEY_IMAGE_MAX_P = 510    # 64 * (P + 2) * 2 <= 65 536
GROUP_MAX_D = 1 << 24          # __umul24(row id, row bytes) is exact up to here

NQ_EDGES = (1, 15, 16, 17, 63, 64, 65, 129)    # a wave owns 16 queries, a workgroup 64

# (P, bands to test, expected form without keys, expected form with keys); the bands cover r = 1, 2, 3, 4, 5, 8,
# b = 1 (r = P) and b = P; a prime P has only b = 1 and b = P
U16_SHAPES = (
    (5, (1, 5), 4, 4),
    (12, (3, 4, 6), 4, 4),
    (32, (4, 8), 4, 4),
    (33, (11, 3), 8, 8),
    (64, (16, 8), 8, 8),
    (65, (13, 5), 16, 16),
    (100, (20, 25), 16, 16),
    (128, (32, 16), 16, 16),
    (129, (43,), 32, 32),
    (256, (64, 32, 1), 32, 32),
    (257, (1, 257), 64, 64),
    (260, (52, 65), 64, 64),
    (510, (102, 255), 64, 64),
    (511, (73, 7), 64, WAVE_PER_QUERY),
    (512, (128, 64), 64, WAVE_PER_QUERY),
    (513, (171,), WAVE_PER_QUERY, WAVE_PER_QUERY),
    (520, (130, 104, 65), WAVE_PER_QUERY, WAVE_PER_QUERY),
)
I32_SHAPES = (
    (5, (1, 5), 4, 4),
    (16, (4, 2, 16), 4, 4),
    (17, (1, 17), 8, 8),
    (32, (8, 16), 8, 8),
    (33, (11,), 16, 16),
    (64, (16, 8), 16, 16),
    (65, (13,), 32, 32),
    (100, (20, 50), 32, 32),
    (128, (32, 16), 32, 32),
    (129, (43,), 64, 64),
    (256, (64, 32), 64, 64),
    (257, (1, 257), WAVE_PER_QUERY, WAVE_PER_QUERY),
    (260, (52, 65), WAVE_PER_QUERY, WAVE_PER_QUERY),
)
SHAPES = {"u16": U16_SHAPES, "i32": I32_SHAPES}
# one P per form of each table type, for the nq edges
NQ_EDGE_P = {"u16": (12, 64, 100, 256, 260, 520), "i32": (5, 32, 64, 100, 256, 260)}


def expected_form(kind, P, with_keys, D=1000):
    """the kernel form launch_minhash picks: the group kernel's LPR, or WAVE_PER_QUERY (the 4 GiB guard is not
    modelled: no test builds such a table)"""
    vec = 8 if kind == "u16" else 4
    lanes = (P + vec - 1) // vec
    if lanes > 64 or D > GROUP_MAX_D or (with_keys and P > GROUP_KEY_IMAGE_MAX_P):
        return WAVE_PER_QUERY
    for lpr in (4, 8, 16, 32, 64):
        if lanes <= lpr:
            return lpr
    raise AssertionError("unreachable")


def set_sizes(LPR):
    """set sizes at the group kernel's loop edges: the sub-step (MH_CH), the step (LPR rows), the prefetch of the next
    LPR row ids, and a set of many steps"""
    out = []
    for n in (0, 1, 3, 4, 5, LPR - 1, LPR, LPR + 1, 2 * LPR - 1, 2 * LPR, 2 * LPR + 1, 3 * LPR + 2, 1000):
        if n not in out:
            out.append(n)
    return out


# ---------------------------------------------------------------------------- references
def ref_minhash(offsets, rows, table_values):
    """sig[q][p] = min over the rows d of query q's set of table_values[p][d], -1 for an empty set.  table_values is
    an integer [P][D] array of arbitrary values (it need not hold permutations).  -> int64 [nq][P]"""
    table_values = np.asarray(table_values)
    nq = len(offsets) - 1
    sig = np.full((nq, table_values.shape[0]), -1, dtype=np.int64)
    for q in range(nq):
        ids = np.asarray(rows[offsets[q]:offsets[q + 1]], dtype=np.int64)
        if len(ids):
            sig[q] = table_values[:, ids].astype(np.int64).min(axis=1)
    return sig


def ref_norm2(sig):
    s = np.asarray(sig).astype(np.int64)
    return (s * s).sum(axis=1)


M64 = (1 << 64) - 1
HASH_SEED = 0x243F6A8885A308D3
HASH_MUL = 0x9E3779B97F4A7C15


def ref_mix64(z):
    """splitmix64 finaliser on uint64 arrays (qr_mix64 in csrc/common.h, restated)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def ref_band_keys(sig, b):
    """band keys of a signature matrix -> uint64 [nq][b].  Only the low 16 bits of a value count.  r <= 4: the r
    values packed, value j at bits 16 j.  r > 4: the project's hash of the tuple (qr_make_key in csrc/common.h); the
    all-0xFFFF tuple gives ~0 and no other tuple does (a hash that equals ~0 is moved to ~0 - 1)."""
    sig = np.asarray(sig)
    nq, P = sig.shape
    assert b > 0 and P % b == 0
    r = P // b
    lo = (sig.astype(np.int64) & 0xFFFF).astype(np.uint64).reshape(nq, b, r)
    if r <= 4:
        k = np.zeros((nq, b), dtype=np.uint64)
        for j in range(r):
            k |= lo[:, :, j] << np.uint64(16 * j)
        return k
    h = np.full((nq, b), HASH_SEED, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(r):
            h = (h ^ lo[:, :, j]) * np.uint64(HASH_MUL)
            h ^= h >> np.uint64(29)
    h = ref_mix64(h)
    h = np.where(h == np.uint64(M64), np.uint64(M64 - 1), h)
    empty = np.all(lo == np.uint64(0xFFFF), axis=2)
    return np.where(empty, np.uint64(M64), h)


def scalar_band_key(values):
    """the wide-band key (r > 4) of ONE tuple with Python integers: a second, independent statement of the hash"""
    h = HASH_SEED
    for v in values:
        h = ((h ^ (int(v) & 0xFFFF)) * HASH_MUL) & M64
        h ^= h >> 29
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & M64
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & M64
    h ^= h >> 31
    if all((int(v) & 0xFFFF) == 0xFFFF for v in values):
        return M64
    return M64 - 1 if h == M64 else h


CSR_BAD_ENDS, CSR_DECREASING, CSR_ROW_RANGE = 1, 2, 4


def ref_check_csr(offsets, rows, D):
    """the flag bits of qrlsh_check_csr: 1 = offsets[0] != 0 or offsets[-1] != len(rows), 2 = offsets decrease
    somewhere, 4 = a row id outside [0, D)"""
    offsets = [int(x) for x in offsets]
    flags = 0
    if offsets[0] != 0 or offsets[-1] != len(rows):
        flags |= CSR_BAD_ENDS
    if any(offsets[t + 1] < offsets[t] for t in range(len(offsets) - 1)):
        flags |= CSR_DECREASING
    if any(int(d) < 0 or int(d) >= D for d in rows):
        flags |= CSR_ROW_RANGE
    return flags


def band_keys_qpb(P):
    """queries per workgroup of the standalone band_keys kernel (pick_qpb): the LDS image qpb * (P + 2) * 2 bytes is
    kept within 32 KiB"""
    qpb = 64
    while qpb > 4 and qpb * (P + 2) * 2 > 32768:
        qpb >>= 1
    return qpb


# ---------------------------------------------------------------------------- tables
def table_values(P, D, seed, top=None):
    """int64 [P][D] of values in [0, top) (default D): column p is, by p % 4, descending in the row id (the LAST row of
    an ascending set decides the minimum), ascending (the first row decides, and a stray gather of row 0 shows), a random
    permutation-like draw, or a draw from a few values with the extremes 0 and top - 1 among them (ties).  Every lane
    of the kernel holds at least 4 consecutive columns, so it sees all four kinds."""
    top = D if top is None else top
    rng = np.random.default_rng(seed)
    d = np.arange(D, dtype=np.int64)
    tab = np.empty((P, D), dtype=np.int64)
    for p in range(P):
        kind = p % 4
        if kind == 0:
            tab[p] = (top - 1) - (d * top // D)
        elif kind == 1:
            tab[p] = d * top // D
        elif kind == 2:
            tab[p] = rng.integers(0, top, size=D)
        else:
            tab[p] = rng.choice(np.array([0, 1, top // 2, top - 2, top - 1], dtype=np.int64), size=D)
    return tab


# ---------------------------------------------------------------------------- answer sets (CSR)
def csr_of(sets):
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in sets])
    rows = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets] + [np.zeros(0, np.int32)]).astype(np.int32)
    return offsets, rows


def _draw_set(rng, D, n, ends):
    """n distinct ascending row ids of [0, D); ends: row ids 0 and D - 1 are among them (n >= 2)"""
    ids = np.sort(rng.choice(D, size=n, replace=False)).astype(np.int32)
    if ends and n >= 2:
        ids[0], ids[-1] = 0, D - 1
    return ids


def shuffled_sizes(LPR, nq, D, seed):
    """consecutive queries cycle through set_sizes(LPR), every cycle in a fresh shuffled order: every wave (16
    queries) and every batch of 64 / LPR groups mixes long, short and empty sets.  Every third non-trivial set holds
    row ids 0 and D - 1."""
    rng = np.random.default_rng(seed)
    sizes = [n for n in set_sizes(LPR) if n <= D]
    sets, order = [], []
    for q in range(nq):
        if not order:
            order = list(rng.permutation(len(sizes)))
        n = sizes[order.pop()]
        sets.append(_draw_set(rng, D, n, ends=(q % 3 == 0)))
    return csr_of(sets)


def lonely_long(nq, D, seed, n=1000):
    """one set of n rows per 16 queries (its place in the wave moves from wave to wave), every other set empty: the
    wave's loops run to the longest set of its groups while the other groups idle"""
    rng = np.random.default_rng(seed)
    sets = []
    for q in range(nq):
        long_one = (q % 16) == ((q // 16) * 5 + 3) % 16 or (nq < 4 and q == nq - 1)
        sets.append(_draw_set(rng, D, n, ends=True) if long_one else np.zeros(0, np.int32))
    return csr_of(sets)


def all_empty(nq):
    return np.zeros(nq + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)


def whole_table(nq, D):
    """every query's set is the whole table"""
    return csr_of([np.arange(D, dtype=np.int32)] * nq)
