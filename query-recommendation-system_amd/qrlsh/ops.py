"""Thin torch-tensor wrappers over the C ABI (include/qrlsh.h).

Tensors are device buffers only: every function checks device / dtype / contiguity, passes
raw pointers and the current HIP stream to libqrlsh, and returns tensors.  64-bit unsigned
words (band keys, pairs, edge keys) are carried in torch.int64 tensors (bit patterns).
"""
import ctypes

import numpy as np
import torch

from . import _lib

_vp = ctypes.c_void_p


def _stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    return _vp(t.data_ptr())


def _need(t, dtype, name, ndim=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA/HIP tensor" % name)
    if t.dtype != dtype:
        raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must have %d dimensions" % (name, ndim))
    return t


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def to_host(t):
    """device tensor -> numpy array through PINNED host memory (torch's caching host allocator: the first copy of a
    size pays for the pinning, later ones reuse the block once the array it backed is gone).  A plain `.cpu()` lands
    in pageable memory at ~6 GB/s -- 139 ms for the 786 MB of top-K rows of a 10 M-query step, 7 x the step itself;
    the pinned copy runs at the link's rate.  The array owns its buffer (nothing is shared between calls)."""
    if not isinstance(t, torch.Tensor):
        return np.asarray(t)
    if not t.is_cuda:
        return t.numpy()
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return h.numpy()


def id_bits_for(nq):
    """bits needed for a query id in [0, nq)"""
    return max(1, int(nq - 1).bit_length()) if nq > 1 else 1


# ---------------------------------------------------------------------------
# permutation table (host side; recommender.py:120)
# ---------------------------------------------------------------------------
def legacy_permutations(P, D, seed=None, rng=None):
    """The P consecutive np.random.permutation(D) draws of recommender.py:120.

    seed given -> RandomState(seed) (the same stream np.random.seed(seed) selects);
    otherwise `rng` (default: the global legacy np.random, consumed exactly like the
    reference consumes it).  Returns int32 [P][D].
    """
    if seed is not None:
        rng = np.random.RandomState(seed)
    elif rng is None:
        rng = np.random
    out = np.empty((P, D), dtype=np.int32)
    for p in range(P):
        out[p] = rng.permutation(D)
    return out


class PermTable:
    """Transposed permutation table resident in HBM: tab[d][0..P) = perm_0[d] .. perm_{P-1}[d]."""

    def __init__(self, tab, code, P, P_stride, D):
        self.tab, self.code, self.P, self.P_stride, self.D = tab, code, P, P_stride, D


def perm_table(perms, device="cuda", force_i32=False):
    """Upload int [P][D] permutations as the transposed [D][P_stride] table the MinHash
    kernel gathers from: uint16 when D <= 65536 (half the gather bytes), else int32."""
    perms = np.asarray(perms)
    P, D = perms.shape
    if D <= 65536 and not force_i32:
        stride = (P + 7) // 8 * 8
        tab = np.full((D, stride), 0xFFFF, dtype=np.uint16)
        tab[:, :P] = perms.T
        t = torch.from_numpy(tab.view(np.int16)).to(device)
        code = _lib.PERM_U16
    else:
        stride = (P + 3) // 4 * 4
        tab = np.full((D, stride), 0x7FFFFFFF, dtype=np.int32)
        tab[:, :P] = perms.T
        t = torch.from_numpy(tab).to(device)
        code = _lib.PERM_I32
    return PermTable(t, code, P, stride, D)


# ---------------------------------------------------------------------------
# a1 / a2
# ---------------------------------------------------------------------------
def can_compact(table):
    """compact uint16 signature rows are lossless iff every value < 65535 (0xFFFF encodes -1)"""
    return table.D <= 65535 and table.code == _lib.PERM_U16


def sig_to_int32(sig):
    """signature tensor (int32, or compact uint16 rows carried as torch.int16) -> int32"""
    if sig.dtype == torch.int32:
        return sig
    v = sig.to(torch.int32) & 0xFFFF
    return torch.where(v == 0xFFFF, torch.full_like(v, -1), v)


def check_csr(offsets, rows, D):
    """raise ValueError unless (offsets, rows) is a well-formed CSR of row ids in [0, D): the kernel gathers
    table rows by these ids without a bounds check (one small kernel + one read-back)"""
    lib = _lib.load()
    nq = offsets.numel() - 1
    flags = torch.zeros((1,), dtype=torch.int32, device=offsets.device)
    _lib.check(lib.qrlsh_check_csr(_ptr(offsets), _ptr(rows), nq, rows.numel(), int(D), _ptr(flags), _stream()))
    f = int(flags.item())
    if f:
        what = [m for bit, m in ((1, "offsets[0] != 0 or offsets[-1] != len(rows)"), (2, "offsets decrease"),
                                 (4, "row id outside [0, %d)" % D)) if f & bit]
        raise ValueError("malformed answer sets: " + "; ".join(what))


def minhash(offsets, rows, table, b=None, want_norm=True, compact=False, validate=True, out=None):
    """sig[q][p] = min over the answer set of perm_p (recommender.py:105-143), -1 if empty.
    Returns (sig [nq,P], norm2 int64 [nq] | None, keys int64 [b,nq] | None).  sig is int32, or
    with compact=True (needs can_compact(table)) the uint16 rows (torch.int16 bit patterns,
    0xFFFF = -1) that qrlsh_score_pairs reads at half the bytes; see sig_to_int32.
    validate: check the CSR first (check_csr); callers that built it with the library's own kernels
    (answer_sets, synth_csr) may pass False.
    out=(sig, norm2, keys): write into these contiguous tensors (slices of larger buffers) instead of new ones."""
    lib = _lib.load()
    _need(offsets, torch.int64, "offsets", 1)
    _need(rows, torch.int32, "rows", 1)
    nq = offsets.numel() - 1
    if nq < 0:
        raise ValueError("offsets must have nq+1 entries")
    if validate and nq > 0:
        check_csr(offsets, rows, table.D)
    P = table.P
    dev = offsets.device
    if b is not None and P % b != 0:
        raise AssertionError("signature length %d not divisible by b=%d" % (P, b))  # lsh.py:20
    if compact and not can_compact(table):
        raise ValueError("compact signatures need D <= 65535")
    if out is not None:
        sig, norm2, keys = out
        _need(sig, torch.int16 if compact else torch.int32, "out sig", 2)
        if tuple(sig.shape) != (nq, P) or (norm2 is not None and norm2.numel() != nq) or \
                (keys is not None and (b is None or tuple(keys.shape) != (b, nq))):
            raise ValueError("out buffers do not match (nq=%d, P=%d, b=%s)" % (nq, P, b))
        if norm2 is not None:
            _need(norm2, torch.int64, "out norm2", 1)
        if keys is not None:
            _need(keys, torch.int64, "out keys", 2)
        if (b is not None) != (keys is not None) or want_norm != (norm2 is not None):
            raise ValueError("out must hold exactly the outputs asked for")
    else:
        sig = torch.empty((nq, P), dtype=torch.int16 if compact else torch.int32, device=dev)
        norm2 = torch.empty((nq,), dtype=torch.int64, device=dev) if want_norm else None
        keys = torch.empty((b, nq), dtype=torch.int64, device=dev) if b is not None else None
    _lib.check(lib.qrlsh_minhash(_ptr(offsets), _ptr(rows), nq, _ptr(table.tab), table.code, P, table.P_stride,
                                 table.D, None if compact else _ptr(sig), _ptr(sig) if compact else None,
                                 _ptr(norm2), _ptr(keys), b if b is not None else 0, _stream()))
    return sig, norm2, keys


def band_keys(sig, b, want_norm=False):
    """Band keys of an int32 signature matrix (lsh.py:17-38) -> int64 [b,nq] (+ norm2)."""
    lib = _lib.load()
    _need(sig, torch.int32, "sig", 2)
    nq, P = sig.shape
    if b <= 0 or P % b != 0:
        raise AssertionError("signature length %d not divisible by b=%d" % (P, b))  # lsh.py:20
    keys = torch.empty((b, nq), dtype=torch.int64, device=sig.device)
    norm2 = torch.empty((nq,), dtype=torch.int64, device=sig.device) if want_norm else None
    _lib.check(lib.qrlsh_band_keys(_ptr(sig), nq, P, b, _ptr(keys), _ptr(norm2), _stream()))
    return (keys, norm2) if want_norm else keys


def row_norms(sig):
    lib = _lib.load()
    _need(sig, torch.int32, "sig", 2)
    nq, P = sig.shape
    out = torch.empty((nq,), dtype=torch.int64, device=sig.device)
    _lib.check(lib.qrlsh_row_norms(_ptr(sig), nq, P, _ptr(out), _stream()))
    return out


# ---------------------------------------------------------------------------
# radix sort
# ---------------------------------------------------------------------------
def sort_u64(keys, vals=None, bit_lo=0, bit_hi=64, mix=False, iota=False, fold=0, owner_shard=0, host_shard=0):
    """Stable LSD radix sort of each row of keys (int64 bit patterns, unsigned order) over
    bits [bit_lo, bit_hi) (of mix64(key) when mix, of i << fold | j when fold).  The range is exact:
    bits at and above bit_hi never influence the order, also when bit_hi - bit_lo is no multiple of 8.
    `keys` (and vals) are consumed as one of the two ping-pong buffers.
    Returns (sorted_keys, sorted_vals | None)."""
    lib = _lib.load()
    _need(keys, torch.int64, "keys")
    k2 = keys if keys.dim() == 2 else keys.view(1, -1)
    nbatch, n = k2.shape
    if iota and vals is None:
        vals = torch.empty((nbatch, n), dtype=torch.int32, device=keys.device)
    if vals is not None:
        _need(vals, torch.int32, "vals")
        if vals.numel() != k2.numel():
            raise ValueError("vals must match keys")
    kb = torch.empty_like(k2)
    vb = torch.empty_like(vals) if vals is not None else None
    ws = _ws(lib.qrlsh_sort_workspace_bytes(n, nbatch), keys.device)
    flags = (_lib.SORT_MIX if mix else 0) | (_lib.SORT_IOTA if iota else 0)
    aux = 0
    if fold:
        flags |= _lib.SORT_FOLD
        aux = int(fold)
    if owner_shard:   # one pass: digit = (key >> bit_lo) // owner_shard  (rank owning that id)
        flags |= _lib.SORT_OWNER
        aux = int(owner_shard)
        bit_hi = bit_lo + 1
    if host_shard:    # one pass over pair words: digit = the rank that scores the pair (common.h: qr_pair_host)
        flags |= _lib.SORT_HOST
        aux = int(host_shard)
        bit_lo, bit_hi = 0, 1
    rc = _lib.check(lib.qrlsh_sort_u64(_ptr(k2), _ptr(kb), _ptr(vals), _ptr(vb), n, nbatch, bit_lo, bit_hi, flags, aux,
                                       _ptr(ws), ws.numel(), _stream()))
    ko = kb if rc == 1 else k2
    vo = (vb if rc == 1 else vals) if vals is not None else None
    if keys.dim() == 1:
        ko = ko.view(-1)
        vo = vo.view(-1) if vo is not None else None
    elif vo is not None:
        vo = vo.view(nbatch, n)
    return ko, vo


def hash_bits_for(n):
    """Bits of mix64(key) the grouping sort orders by: enough that a run of equal hash bits
    holds ~1/8 foreign keys on average (n / 2^bits <= 1/8), in whole 8-bit passes."""
    need = max(1, int(n - 1).bit_length()) + 3 if n > 1 else 8
    return min(32, max(8, (need + 7) // 8 * 8))


def owner_bounds(words, bit_lo, shard, world):
    """split points (device int64 [world + 1]) of words already grouped by owner = (word >> bit_lo) // shard;
    bit_lo = -1: pair words grouped by their scoring rank (sort_u64(host_shard=...))"""
    lib = _lib.load()
    _need(words, torch.int64, "words", 1)
    bounds = torch.empty((world + 1,), dtype=torch.int64, device=words.device)
    _lib.check(lib.qrlsh_owner_bounds(_ptr(words), words.numel(), bit_lo, shard, world, _ptr(bounds), _stream()))
    return bounds


def owner_sizes(words, bit_lo, shard, world):
    """per-rank counts of words already grouped by owner (a host list: one read-back)"""
    bl = owner_bounds(words, bit_lo, shard, world).tolist()
    return [bl[g + 1] - bl[g] for g in range(world)]


def bucket_sort(keys, hash_bits=None):
    """Group equal band keys (replaces the dict buckets of lsh.py:31-38): per band, sort
    (key, query id) by the top hash_bits bits of mix64(key).  keys int64 [b,nq] (consumed).
    Returns (sorted_keys [b,nq], sorted_ids int32 [b,nq])."""
    _need(keys, torch.int64, "keys", 2)
    hb = hash_bits if hash_bits is not None else hash_bits_for(keys.shape[1])
    return sort_u64(keys, None, 64 - hb, 64, mix=True, iota=True)


# ---------------------------------------------------------------------------
# a3: pairs
# ---------------------------------------------------------------------------
def emit_pairs(sorted_keys, sorted_ids, r, hash_bits=None):
    """All (i<j) pairs of every non-empty bucket with > 1 member, every band
    (lsh.py:42-53), as int64 i<<32|j, duplicates across bands included."""
    lib = _lib.load()
    _need(sorted_keys, torch.int64, "sorted_keys", 2)
    _need(sorted_ids, torch.int32, "sorted_ids", 2)
    b, nq = sorted_keys.shape
    dev = sorted_keys.device
    hb = hash_bits if hash_bits is not None else hash_bits_for(nq)
    ws = _ws(lib.qrlsh_pairs_workspace_bytes(nq, b), dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_pairs_count(_ptr(sorted_keys), nq, b, r, hb, _ptr(ws), ws.numel(), _ptr(total), _stream()))
    n = int(total.item())
    pairs = torch.empty((n,), dtype=torch.int64, device=dev)
    if n:
        _lib.check(lib.qrlsh_pairs_fill(_ptr(sorted_keys), _ptr(sorted_ids), nq, b, r, hb, _ptr(ws), _ptr(pairs),
                                        _stream()))
    return pairs


def unique_sorted(a):
    lib = _lib.load()
    _need(a, torch.int64, "a", 1)
    n = a.numel()
    ws = _ws(lib.qrlsh_compact_workspace_bytes(n), a.device)
    total = torch.zeros(1, dtype=torch.int64, device=a.device)
    _lib.check(lib.qrlsh_unique_count(_ptr(a), n, _ptr(ws), ws.numel(), _ptr(total), _stream()))
    m = int(total.item())
    out = torch.empty((m,), dtype=torch.int64, device=a.device)
    if m:
        _lib.check(lib.qrlsh_unique_fill(_ptr(a), n, _ptr(ws), _ptr(out), _stream()))
    return out


def sort_pairs(pairs, nq):
    """sort i<<32|j words: LSD over j's bits, then i's bits"""
    ib = id_bits_for(nq)
    p, _ = sort_u64(pairs, None, 0, 2 * ib, fold=ib)   # digits of i << ib | j: ceil(2 ib / 8) passes
    return p


def row_group_bits(id_bits, words_per_row=0.0):
    """low bits of i the grouping sort may ignore (rows of 2^g consecutive i, finished in LDS) when that
    saves its last 8-bit pass: the id bits left over above a multiple of 8, if at most 4 -- and only while
    the grouped rows stay short (words_per_row = emitted pairs per query: rows of 2^g queries beyond ~1000
    words would all go through the long-row kernel, or overflow it)"""
    g = id_bits % 8
    if not (id_bits > 8 and 0 < g <= 4):
        return 0
    return g if words_per_row * (1 << g) <= 1024 else 0


def group_pairs_by_i(pairs, nq, group_bits=0):
    """pairs i<<32|j ordered by i >> group_bits only (arbitrary order inside a row)"""
    p, _ = sort_u64(pairs, None, 32 + group_bits, 32 + id_bits_for(nq))
    return p


def row_unique(grouped, group_bits=0, id_bits=32):
    """Sorted unique pairs from pairs grouped by i >> group_bits (group_pairs_by_i); None when a row is
    too long even for the one-row-per-workgroup kernel (heavily skewed data) -- use
    unique_sorted(sort_pairs(...)) then."""
    lib = _lib.load()
    _need(grouped, torch.int64, "grouped", 1)
    n = grouped.numel()
    if n == 0:
        return grouped
    dev = grouped.device
    tmp = torch.empty_like(grouped)
    ws = _ws(lib.qrlsh_row_unique_workspace_bytes(n), dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_row_unique_count(_ptr(grouped), n, int(group_bits), int(id_bits), _ptr(tmp), _ptr(ws),
                                          ws.numel(), _ptr(tot), _stream()))
    total, overflow = tot.tolist()
    if overflow:
        return None
    out = torch.empty((total,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_row_unique_fill(_ptr(tmp), n, _ptr(ws), _ptr(out), _stream()))
    return out


def region_group_bits(id_bits, nids, words_per_query=0.0):
    """group bits of the region form of the de-duplication (regions of 2^g consecutive queries finished by one
    workgroup each): as many as fit the 32-bit (i's low bits, j) value, at most 8, fewer while a region would
    hold more than ~16 K words; None when fewer than 3 remain (single-i rows: use row_unique)"""
    g = min(8, 32 - id_bits, id_bits)    # (no more than the id has: everything is one region then)
    if g + id_bits == 32 and nids >= (1 << id_bits):
        g -= 1
    while g > 0 and words_per_query * (1 << g) > 16384:
        g -= 1
    return g if g >= 3 else None


def region_unique(grouped, group_bits, id_bits, nids):
    """Sorted unique pairs from pairs grouped by i >> group_bits (group_pairs_by_i), one workgroup per region of
    2^group_bits queries; None when a region holds more than ~11 K distinct pairs (use the general path)."""
    lib = _lib.load()
    _need(grouped, torch.int64, "grouped", 1)
    n = grouped.numel()
    if n == 0:
        return grouped
    dev = grouped.device
    tmp = torch.empty_like(grouped)
    ws = _ws(lib.qrlsh_region_unique_workspace_bytes(nids, group_bits), dev)
    tot = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_region_unique_count(_ptr(grouped), n, int(group_bits), int(id_bits), int(nids), _ptr(tmp), _ptr(ws),
                                             ws.numel(), _ptr(tot), _stream()))
    total, overflow = tot.tolist()
    if overflow:
        return None
    out = torch.empty((total,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_region_unique_fill(_ptr(tmp), n, int(group_bits), int(nids), _ptr(ws), _ptr(out), _stream()))
    return out


REGION_MIN_GROUP_BITS = 6               # below: the general sort + unique instead of the region form (see unique_pairs)
REGION_SCATTER_MAX_BYTES = 48 << 30    # the fixed-region grouping is skipped when its buffers would exceed this


def region_values_fit(group_bits, id_bits, nids):
    """the final regions can hold the 32-bit value (i's low group_bits, j) instead of the pair word: it fits, and is
    never the finish's empty-slot marker 0xFFFFFFFF"""
    return group_bits + id_bits < 32 or (group_bits + id_bits == 32 and nids < (1 << id_bits))


def region_unique_scattered(emitted, group_bits, id_bits, nids, words_per_query=0.0):
    """Sorted unique pairs straight from the emitted words: dealt into fixed regions of 2^group_bits queries by two
    histogram-free partition steps (qrlsh_pair_regions_scatter32: nothing inside a region is ordered -- the region
    finish does not need it; an entry is the 32-bit value (i's low group_bits, j)), then the region finish on those
    regions.  -> (pairs, "") or (None, why): "cap" when a region outgrew its capacity or the buffers would be too large
    (the caller then groups by sorting), "distinct" when a region holds more distinct pairs than the finish's LDS set
    (sorting by region would meet the same: the caller sorts everything).  ValueError unless region_values_fit
    (region_group_bits never returns such group bits)."""
    lib = _lib.load()
    _need(emitted, torch.int64, "emitted", 1)
    n = emitted.numel()
    if n == 0:
        return emitted, ""
    dev = emitted.device
    wpq = float(words_per_query)
    words = lib.qrlsh_pair_regions_words(n, nids, group_bits, wpq)
    twords = lib.qrlsh_pair_regions_tmp_words(n, nids, group_bits, wpq)
    if not region_values_fit(group_bits, id_bits, nids):
        raise ValueError("group_bits=%d + id_bits=%d (nids=%d) do not fit a 32-bit region value" % (group_bits, id_bits, nids))
    # per entry: 4 bytes of the final regions + 8 of tmp (the finish's output keeps pair words)
    if words == 0 or n >= (1 << 32) or words * 12 + twords * 8 > REGION_SCATTER_MAX_BYTES:
        return None, "cap"          # (words == 0: more than 65536 regions -- two levels of 256 digits do not reach)
    cap = lib.qrlsh_pair_regions_cap(n, nids, group_bits, wpq)
    nreg = lib.qrlsh_pair_regions_count(n, nids, group_bits, wpq)
    try:      # fixed regions trade memory for passes: when the device is short of it, group by sorting instead
        regions = torch.empty((words,), dtype=torch.int32, device=dev)
        tmpr = torch.empty((twords,), dtype=torch.int64, device=dev) if twords else None
        tmp = torch.empty((words,), dtype=torch.int64, device=dev)
    except torch.cuda.OutOfMemoryError:
        regions = tmpr = tmp = None
        torch.cuda.empty_cache()
        return None, "cap"
    counts = torch.empty((nreg + 256,), dtype=torch.int32, device=dev)
    ovf = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.check(lib.qrlsh_pair_regions_scatter32(_ptr(emitted), n, int(group_bits), int(id_bits), int(nids), wpq, _ptr(tmpr),
                                                _ptr(regions), _ptr(counts), _ptr(ovf), _stream()))
    del tmpr
    ws = _ws(lib.qrlsh_region_unique_workspace_bytes(nids, group_bits), dev)
    tot = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_region_unique_count_regions32(_ptr(regions), _ptr(counts), cap, n, int(group_bits), int(id_bits),
                                                       int(nids), _ptr(tmp), _ptr(ws), ws.numel(), _ptr(ovf), _ptr(tot),
                                                       _stream()))
    total, overflow, capped = tot.tolist()  # one read-back: the scatter's flag is the third word
    if capped:
        return None, "cap"
    if overflow:
        return None, "distinct"
    del regions
    out = torch.empty((total,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_region_unique_fill(_ptr(tmp), n, int(group_bits), int(nids), _ptr(ws), _ptr(out), _stream()))
    return out, ""


def unique_pairs(emitted, nq, stats=None, words_per_query=None, scatter=True):
    """the Python set of lsh.py:41,53: sorted unique words of the emitted pairs (consumed).
    words_per_query: emitted words per query id of the id space (default: emitted / nq).
    scatter: group by the histogram-free fixed-region partition (default); False: by the stable radix sort."""
    ib = id_bits_for(nq)
    wpq = emitted.numel() / max(nq, 1) if words_per_query is None else words_per_query
    g = region_group_bits(ib, nq, wpq)
    pairs = None
    if g is not None and g < REGION_MIN_GROUP_BITS:
        # ids of 27 bits and more leave at most 5 group bits: regions of 32 queries, a workgroup per ~2 000 words, three
        # grouping passes before it -- the plain 7-pass sort + unique is faster there (configs[4], one rank: 4 ms against
        # 9.6 for 93 M words, 39 against 70.6 for the 897 M it really receives, where the regions would give up anyway)
        grouped, g = emitted, 0
    elif g is not None:
        path, why = "regions-in-lds", "cap"
        if scatter:
            pairs, why = region_unique_scattered(emitted, g, ib, nq, wpq)
            path = "regions-in-lds (scattered)"
        if pairs is None and why == "distinct":
            grouped = emitted                       # straight to the full sort below
        elif pairs is None:
            grouped = group_pairs_by_i(emitted, nq, g)
            pairs = region_unique(grouped, g, ib, nq)
            path = "regions-in-lds"
    else:
        g = row_group_bits(ib, wpq)
        grouped = group_pairs_by_i(emitted, nq, g)
        pairs = row_unique(grouped, g, ib)
        path = "rows-in-lds"
    if stats is not None:
        stats["dedup_path"] = path if pairs is not None else "full-sort"
        stats["group_bits"] = g
    if pairs is None:
        pairs = unique_sorted(sort_pairs(grouped, nq))
    return pairs


def part_bits_for(n):
    """T = bits of the hash partition of the fast bucket path: parts of <= ~4400 records on
    average (the LDS image holds 6144; the room above the mean is for popular keys -- with parts of ~4900
    on average the 10 M-query bench workload overflows a part), at least 8, at most 16."""
    t = 8
    while t < 16 and n > 4400 * (1 << t):
        t += 1
    return t


_EMIT_HINT = {}   # (nq, b, r) -> pairs emitted by the last call of that shape: the next call's capacity guess


def emit_pairs_fast(keys, r, part_bits=None, capacity=None, chunks=None):
    """emit_pairs for unsorted band-major keys through the partition + LDS-finish path.
    Returns the pairs tensor, or None when a part overflowed the LDS image (skewed data).
    The parts reserve their output ranges on a device cursor (qrlsh_bucket_pairs_emit), so
    no count pass runs; the output buffer is sized by `capacity` (default: 1.25 x what the last call
    of this shape emitted, else 24 pairs per query) and the call is repeated once, exactly sized,
    if that was too small.
    chunks=(world, nb, nql[, stride]): `keys` is the [world][nb][nql] buffer a band-partitioned all-to-all delivers
    (band t, query q at [q // nql][t][q % nql]); it is read in place.  stride (default nb * nql):
    words between two ranks' chunks -- nb of each rank's b bands, read out of a [world][b][nql] buffer."""
    lib = _lib.load()
    if chunks is not None:
        world, b, nql = chunks[:3]
        stride = chunks[3] if len(chunks) > 3 else b * nql     # words between the chunks of two ranks
        nq = world * nql
        _need(keys, torch.int64, "keys")
        if stride < b * nql or keys.numel() < (world - 1) * stride + b * nql:
            raise ValueError("chunked keys: need (world - 1) * stride + nb * nql words")
        layout = (nql, stride, nql)
    else:
        _need(keys, torch.int64, "keys", 2)
        b, nq = keys.shape
        layout = (0, 0, 0)
    dev = keys.device
    T = part_bits if part_bits is not None else part_bits_for(nq)
    if nq > 6144 * (1 << T):
        return None  # cannot fit even with the finest partition
    words = lib.qrlsh_bucket_part_words(nq, b, T)
    pk = torch.empty((words,), dtype=torch.int64, device=dev)
    pid = torch.empty((words,), dtype=torch.int32, device=dev)
    twords = lib.qrlsh_bucket_tmp_words(nq, b, T) if T > 8 else 0
    tk = torch.empty((twords,), dtype=torch.int64, device=dev) if T > 8 else None
    tid = torch.empty((twords,), dtype=torch.int32, device=dev) if T > 8 else None
    ws = _ws(lib.qrlsh_bucket_workspace_bytes(nq, b, T), dev)
    tot = torch.zeros(2, dtype=torch.int64, device=dev)
    shape = (nq, b, r)
    if capacity is None:
        capacity = _EMIT_HINT[shape] * 5 // 4 + 1024 if shape in _EMIT_HINT else 24 * nq + 1024
    while True:
        pairs = torch.empty((capacity,), dtype=torch.int64, device=dev)
        _lib.check(lib.qrlsh_bucket_pairs_emit_chunked(_ptr(keys), layout[0], layout[1], layout[2], _ptr(pk),
                                                       _ptr(pid), _ptr(tk), _ptr(tid), nq, b, r, T, _ptr(ws),
                                                       ws.numel(), _ptr(pairs), capacity, _ptr(tot), _stream()))
        n, overflow = tot.tolist()
        if overflow:
            return None
        _EMIT_HINT[shape] = n
        if n <= capacity:
            return pairs[:n]
        del pairs
        capacity = n       # the cursor counted everything: the second run fits exactly


def emit_pairs_any(keys, r, stats=None):
    """All (i<j) pairs of every non-empty bucket, every band, from unsorted band-major keys
    [b,nq] (keys may be consumed): fast path, or the general sort path when it overflows."""
    emitted = emit_pairs_fast(keys, r)
    if stats is not None:
        stats["bucket_path"] = "partition+lds" if emitted is not None else "general-sort"
        stats["part_bits"] = part_bits_for(keys.shape[1])
    if emitted is None:
        sk, sid = bucket_sort(keys)
        emitted = emit_pairs(sk, sid, r)
    return emitted


def verify_pairs(sig, b, pairs):
    """Exact candidate test of lsh.py:31-53 per pair (shares a non-empty band): uint8 flags.
    Needed only for wide bands (r = P / b > 4), whose bucket ids are hashes."""
    lib = _lib.load()
    if not isinstance(sig, torch.Tensor) or sig.dtype not in (torch.int32, torch.int16):
        raise TypeError("sig must be an int32 or int16 (compact) tensor")
    _need(sig, sig.dtype, "sig", 2)
    _need(pairs, torch.int64, "pairs", 1)
    n = pairs.numel()
    flags = torch.empty((n,), dtype=torch.uint8, device=sig.device)
    code = _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32
    _lib.check(lib.qrlsh_verify_pairs(_ptr(sig), code, sig.shape[1], b, _ptr(pairs), n, _ptr(flags), _stream()))
    return flags


def drop_unverified(sig, b, pairs, stats=None):
    """wide bands: keep only the pairs that really share a band (hash collisions of the bucket
    ids, astronomically rare, are removed here so the candidate set stays exact)"""
    if pairs.numel() == 0:
        return pairs
    flags = verify_pairs(sig, b, pairs)
    bad = int((flags == 0).sum().item())
    if stats is not None:
        stats["hash_collision_pairs_dropped"] = bad
    return pairs if bad == 0 else pairs[flags.bool()]


def candidate_pairs(keys, r, stats=None, sig=None):
    """get_candidates (lsh.py:40-55) on band-major keys [b,nq] (consumed): sorted unique
    int64 array of i<<32|j, i<j.  For wide bands (r > 4) pass the signature matrix `sig`: the
    hashed bucket ids are verified against it."""
    b, nq = keys.shape
    if r > 4 and sig is None:
        raise ValueError("band width r=%d > 4 needs the signatures for exact verification" % r)
    emitted = emit_pairs_any(keys, r, stats)
    if stats is not None:
        stats["emitted_pairs"] = int(emitted.numel())
    if emitted.numel() == 0:
        return emitted
    pairs = unique_pairs(emitted, nq, stats)
    if r > 4:
        pairs = drop_unverified(sig, b, pairs, stats)
    return pairs


# ---------------------------------------------------------------------------
# a5: scoring and top-K
# ---------------------------------------------------------------------------
def wide_ids(id_bits):
    """two ids + 11 score bits do not fit one 64-bit top-K key: use key + payload edges"""
    return 2 * id_bits + 11 > 64


def score_pairs(sig, norm2, pairs, want_cos=False, edge_id_bits=None, wide=None):
    """milli = rint(1000 * cosine(sig_i, sig_j)) per pair (recommender.py:203-204).  sig: int32
    rows or compact uint16 rows (torch.int16).
    Returns (milli int32, cos float64 | None, edges | None); edges is the int64 [2n] packed key
    tensor, or with wide ids (forced by wide=True) the tuple (keys int64 [2n], dst int32 [2n])."""
    lib = _lib.load()
    if not isinstance(sig, torch.Tensor) or sig.dtype not in (torch.int32, torch.int16):
        raise TypeError("sig must be an int32 or int16 (compact) tensor")
    _need(sig, sig.dtype, "sig", 2)
    if norm2 is not None:       # None: the kernel sums the norms from the rows itself (exact too, but slower)
        _need(norm2, torch.int64, "norm2", 1)
    _need(pairs, torch.int64, "pairs", 1)
    n = pairs.numel()
    dev = sig.device
    milli = torch.empty((n,), dtype=torch.int32, device=dev)
    cosv = torch.empty((n,), dtype=torch.float64, device=dev) if want_cos else None
    edges = torch.empty((2 * n,), dtype=torch.int64, device=dev) if edge_id_bits is not None else None
    if wide is None:
        wide = edge_id_bits is not None and wide_ids(edge_id_bits)
    edst = torch.empty((2 * n,), dtype=torch.int32, device=dev) if (wide and edges is not None) else None
    code = _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32
    _lib.check(lib.qrlsh_score_pairs(_ptr(sig), code, _ptr(norm2), sig.shape[1], _ptr(pairs), n, _ptr(milli),
                                     _ptr(cosv), _ptr(edges), edge_id_bits if edge_id_bits is not None else 0,
                                     _ptr(edst), _stream()))
    return milli, cosv, ((edges, edst) if edst is not None else edges)


class RemoteIds:
    """the set of remote query ids a rank's pairs touch (bitmap + rank structure on the device)"""

    def __init__(self, ws, nids, q0, nql, bounds):
        self.ws, self.nids, self.q0, self.nql, self.bounds = ws, nids, q0, nql, bounds


def remote_ids(pairs, q0, nql, nids, world):
    """-> RemoteIds of the endpoints of `pairs` outside [q0, q0 + nql); .bounds (device int64 [world + 1]) =
    number of such ids below g * nql, i.e. the per-owner request sizes, [-1] = the total"""
    lib = _lib.load()
    _need(pairs, torch.int64, "pairs", 1)
    dev = pairs.device
    ws = _ws(lib.qrlsh_idset_workspace_bytes(nids), dev)
    bounds = torch.empty((world + 1,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_idset_build(_ptr(pairs), pairs.numel(), int(q0), int(nql), int(nids), int(nql), world,
                                     _ptr(ws), ws.numel(), _ptr(bounds), _stream()))
    return RemoteIds(ws, nids, q0, nql, bounds)


def remote_id_list(rid, total):
    """the ids of the set, ascending (int64 [total])"""
    lib = _lib.load()
    out = torch.empty((total,), dtype=torch.int64, device=rid.ws.device)
    if total:
        _lib.check(lib.qrlsh_idset_list(_ptr(rid.ws), rid.nids, _ptr(out), _stream()))
    return out


def remap_pairs_ids(pairs, rid):
    """pairs (global ids) -> slot(i) << 32 | slot(j) over the row table [local rows | rows of rid's ids]"""
    lib = _lib.load()
    _need(pairs, torch.int64, "pairs", 1)
    out = torch.empty_like(pairs)
    _lib.check(lib.qrlsh_idset_remap(_ptr(pairs), pairs.numel(), int(rid.q0), int(rid.nql), _ptr(rid.ws), rid.nids,
                                     _ptr(out), _stream()))
    return out


def gather_rows(sig, norm2, ids, q0):
    """signature rows + norms of the global ids `ids` (all owned by this rank: row = id - q0)"""
    lib = _lib.load()
    _need(ids, torch.int64, "ids", 1)
    n = ids.numel()
    rows = torch.empty((n, sig.shape[1]), dtype=sig.dtype, device=sig.device)
    norms = torch.empty((n,), dtype=torch.int64, device=sig.device)
    _lib.check(lib.qrlsh_gather_rows(_ptr(sig), sig.shape[1] * sig.element_size(), _ptr(norm2), _ptr(ids), n, int(q0),
                                     _ptr(rows), _ptr(norms), _stream()))
    return rows, norms


def gather_sets(ids, offs_all, rows_all, nql):
    """CSR (offsets int64 [n + 1], rows int32) of the answer sets of the global query ids `ids` (int64, ascending or
    not) out of the replicated per-shard arrays: offs_all [world, nql + 1] int32 / int64, rows_all [world, max_nnz]
    int16 (unsigned 16-bit row ids) / int32 (one read-back: the number of row ids)"""
    lib = _lib.load()
    _need(ids, torch.int64, "ids", 1)
    if offs_all.dtype not in (torch.int32, torch.int64) or rows_all.dtype not in (torch.int16, torch.int32):
        raise TypeError("offs_all must be int32 / int64, rows_all int16 / int32")
    _need(offs_all, offs_all.dtype, "offs_all", 2)
    _need(rows_all, rows_all.dtype, "rows_all", 2)
    world, max_nnz = rows_all.shape
    if tuple(offs_all.shape) != (world, nql + 1):
        raise ValueError("offs_all must be [world, nql + 1]")
    n, dev = ids.numel(), ids.device
    off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    ws = _ws(lib.qrlsh_gather_sets_workspace_bytes(n), dev)
    _lib.check(lib.qrlsh_gather_sets_count(_ptr(ids), n, _ptr(offs_all), offs_all.element_size(), int(nql), world, _ptr(off),
                                           _ptr(ws), ws.numel(), _stream()))
    total = int(off[-1].item())
    rows = torch.empty((total,), dtype=torch.int32, device=dev)
    if total:
        _lib.check(lib.qrlsh_gather_sets_fill(_ptr(ids), n, _ptr(offs_all), offs_all.element_size(), _ptr(rows_all),
                                              rows_all.element_size(), int(nql), max_nnz, _ptr(off), _ptr(rows), _stream()))
    return off, rows


def score_pairs_split(sig, norm2, sig_b, norm2_b, pairs):
    """milli of pairs whose halves index the two-piece row table [sig | sig_b]"""
    lib = _lib.load()
    _need(pairs, torch.int64, "pairs", 1)
    n = pairs.numel()
    milli = torch.empty((n,), dtype=torch.int32, device=pairs.device)
    code = _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32
    _lib.check(lib.qrlsh_score_pairs_split(_ptr(sig), _ptr(norm2), sig.shape[0], _ptr(sig_b), _ptr(norm2_b), code,
                                           sig.shape[1], _ptr(pairs), n, _ptr(milli), _stream()))
    return milli


def pair_edges_interleaved(pairs, milli, id_bits, wide=False):
    """both directed edges of every scored pair, [2t] = i -> j, [2t + 1] = j -> i (what score_pairs writes):
    packed int64 [2n], or with wide ids (keys int64 [2n], dst int32 [2n])"""
    lib = _lib.load()
    n, dev = pairs.numel(), pairs.device
    e = torch.empty((2 * n,), dtype=torch.int64, device=dev)
    d = torch.empty((2 * n,), dtype=torch.int32, device=dev) if wide else None
    _lib.check(lib.qrlsh_pair_edges(_ptr(pairs), _ptr(milli), n, 0 if wide else int(id_bits), _ptr(e), None, _ptr(d),
                                    None, _stream()))
    return (e, d) if wide else e


def local_bits_for(nql):
    return max(1, int(nql - 1).bit_length()) if nql > 1 else 1


def topk_edges_local(edges, edst, K, id_bits, q0, nql, select=True):
    """Per-query top-K from edges that arrived from several scoring ranks (no useful order): re-base the
    src field to this rank's id range, sort the whole (src, 1000 - milli, dst) key, cut.  edst: the dst
    payload of key + payload edges, or None for packed ones."""
    lib = _lib.load()
    dev = edges.device
    n = edges.numel()
    if n == 0:
        z = torch.empty((0,), dtype=torch.int32, device=dev)
        return z, z.clone(), z.clone()
    lb = local_bits_for(nql)
    if lb + 11 + id_bits > 64:
        raise NotImplementedError("%d local + %d global id bits do not fit the 64-bit top-K key" % (lb, id_bits))
    loc = torch.empty_like(edges)
    _lib.check(lib.qrlsh_edges_localize(_ptr(edges), _ptr(edst), n, id_bits, int(q0), int(nql), _ptr(loc), _stream()))
    if select and K <= SELECT_MAX_K and n < (1 << 31):
        # select form: the re-based keys ARE reverse words (src = a local query); sorted on the src bits alone
        # (ceil(lb / 8) passes instead of ceil((lb + 11 + id_bits) / 8)), every edge then ranks itself in its query's run
        src, dst, val = topk_select(None, None, loc, K, id_bits, int(nql))
        src += int(q0)
        return src, dst, val
    se, _ = sort_u64(loc, None, 0, lb + 11 + id_bits)
    ws = _ws(lib.qrlsh_compact_workspace_bytes(n), dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_topk_count(_ptr(se), n, K, id_bits, _ptr(ws), ws.numel(), _ptr(total), _stream()))
    m = int(total.item())
    src = torch.empty((m,), dtype=torch.int32, device=dev)
    dst = torch.empty((m,), dtype=torch.int32, device=dev)
    val = torch.empty((m,), dtype=torch.int32, device=dev)
    _lib.check(lib.qrlsh_topk_fill_based(_ptr(se), None, n, K, id_bits, int(q0), _ptr(ws), _ptr(src), _ptr(dst),
                                         _ptr(val), _stream()))
    return src, dst, val


def score_pairs_rev(sig, norm2, pairs, id_bits, wide=None):
    """milli per pair + the reverse edge word of every pair (src = j): -> (milli int32, rev) with rev the packed
    int64 [n] words, or with wide ids the tuple (keys int64 [n], dst int32 [n]).  Input of topk_select."""
    lib = _lib.load()
    _need(sig, sig.dtype, "sig", 2)
    if norm2 is not None:
        _need(norm2, torch.int64, "norm2", 1)
    _need(pairs, torch.int64, "pairs", 1)
    n, dev = pairs.numel(), sig.device
    if wide is None:
        wide = wide_ids(id_bits)
    milli = torch.empty((n,), dtype=torch.int32, device=dev)
    rev = torch.empty((n,), dtype=torch.int64, device=dev)
    rdst = torch.empty((n,), dtype=torch.int32, device=dev) if wide else None
    code = _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32
    _lib.check(lib.qrlsh_score_pairs_rev(_ptr(sig), code, _ptr(norm2), sig.shape[1], _ptr(pairs), n, _ptr(milli), _ptr(rev),
                                         0 if wide else int(id_bits), _ptr(rdst), _stream()))
    return milli, ((rev, rdst) if wide else rev)


SELECT_MAX_K = 256   # SEL_MAXK in csrc/topk.hip


def topk_select(pairs, milli, rev, K, id_bits, nq):
    """Per-query top-K (recommender.py:206-210) from the sorted scored pairs and their reverse words
    (score_pairs_rev): the reverse words are sorted on j's bits only, then every directed edge ranks itself
    inside its query's two runs.  -> (src, dst, milli) int32, the same COO topk_edges returns.
    pairs = milli = None: the lists are made of the reverse words alone (packed words src << (id_bits + 11) |
    inv << id_bits | neighbour with src < nq: topk_edges_local)."""
    lib = _lib.load()
    rdst = None
    if isinstance(rev, tuple):
        rev, rdst = rev
    dev = rev.device
    n = rev.numel()
    if n == 0:
        z = torch.empty((0,), dtype=torch.int32, device=dev)
        return z, z.clone(), z.clone()
    if K > SELECT_MAX_K:
        raise ValueError("topk_select handles K <= %d; use topk_edges (the sort form) beyond" % SELECT_MAX_K)
    if rdst is None:
        src_bits = id_bits if pairs is not None else local_bits_for(nq)
        rs, rd = sort_u64(rev, None, id_bits + 11, id_bits + 11 + src_bits)
    else:
        rs, rd = sort_u64(rev, rdst, 11, 11 + id_bits)
    ws = _ws(lib.qrlsh_topk_select_workspace_bytes(nq), dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_topk_select_count(_ptr(pairs), n, _ptr(rs), _ptr(rd), int(nq), K, int(id_bits), _ptr(ws), ws.numel(),
                                           _ptr(total), _stream()))
    m = int(total.item())
    src = torch.empty((m,), dtype=torch.int32, device=dev)
    dst = torch.empty((m,), dtype=torch.int32, device=dev)
    val = torch.empty((m,), dtype=torch.int32, device=dev)
    _lib.check(lib.qrlsh_topk_select_fill(_ptr(pairs), _ptr(milli), n, _ptr(rs), _ptr(rd), int(nq), K, int(id_bits), _ptr(ws),
                                          _ptr(src), _ptr(dst), _ptr(val), _stream()))
    return src, dst, val


def remap_pairs(pairs, q0, nql, need):
    """pairs (i local to [q0, q0+nql), j anywhere) -> (i - q0) << 32 | slot(j) over the row table
    [local rows | rows of the ascending global ids `need`] (multi-GPU scoring, qrlsh/dist.py)"""
    lib = _lib.load()
    _need(pairs, torch.int64, "pairs", 1)
    _need(need, torch.int64, "need", 1)
    out = torch.empty_like(pairs)
    _lib.check(lib.qrlsh_remap_pairs(_ptr(pairs), pairs.numel(), int(q0), int(nql), _ptr(need), need.numel(),
                                     _ptr(out), _stream()))
    return out


def pair_edges(pairs, milli, id_bits, wide=False):
    """forward / reverse directed edge keys of scored pairs: (fwd, rev) int64, or with wide ids
    ((fwd_keys, fwd_dst), (rev_keys, rev_dst))"""
    lib = _lib.load()
    _need(pairs, torch.int64, "pairs", 1)
    _need(milli, torch.int32, "milli", 1)
    n, dev = pairs.numel(), pairs.device
    fwd = torch.empty((n,), dtype=torch.int64, device=dev)
    rev = torch.empty((n,), dtype=torch.int64, device=dev)
    fd = torch.empty((n,), dtype=torch.int32, device=dev) if wide else None
    rd = torch.empty((n,), dtype=torch.int32, device=dev) if wide else None
    _lib.check(lib.qrlsh_pair_edges(_ptr(pairs), _ptr(milli), n, 0 if wide else int(id_bits), _ptr(fwd), _ptr(rev),
                                    _ptr(fd), _ptr(rd), _stream()))
    return ((fwd, fd), (rev, rd)) if wide else (fwd, rev)


def topk_edges(edges, K, id_bits):
    """Per-query top-K (recommender.py:206-210) from the directed edges written by score_pairs
    (packed int64 keys, or the (keys, dst) tuple of the wide-id format):
    -> (src, dst, milli) int32, sorted by src, value desc, dst asc; <= K per src."""
    lib = _lib.load()
    edst = None
    if isinstance(edges, tuple):
        edges, edst = edges
    _need(edges, torch.int64, "edges", 1)
    dev = edges.device
    n = edges.numel()
    if n == 0:
        z = torch.empty((0,), dtype=torch.int32, device=dev)
        return z, z.clone(), z.clone()
    # Sorting on (src, 1000-milli) alone is enough: the sort is stable and, per src, the edges
    # arrive with dst ascending (pairs are sorted by (i, j); edge 2t is i->j, 2t+1 is j->i, so a
    # src first meets its smaller neighbours, then its larger ones) -- 4 passes instead of 7.
    if edst is None:
        se, sd = sort_u64(edges, None, id_bits, 2 * id_bits + 11)
        kb = id_bits
    else:
        se, sd = sort_u64(edges, edst, 0, id_bits + 11)
        kb = 0
    ws = _ws(lib.qrlsh_compact_workspace_bytes(n), dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_topk_count(_ptr(se), n, K, kb, _ptr(ws), ws.numel(), _ptr(total), _stream()))
    m = int(total.item())
    src = torch.empty((m,), dtype=torch.int32, device=dev)
    dst = torch.empty((m,), dtype=torch.int32, device=dev)
    val = torch.empty((m,), dtype=torch.int32, device=dev)
    _lib.check(lib.qrlsh_topk_fill(_ptr(se), _ptr(sd), n, K, kb, _ptr(ws), _ptr(src), _ptr(dst), _ptr(val), _stream()))
    return src, dst, val


# ---------------------------------------------------------------------------
# serving new queries: band-key index, probe, column prediction (csrc/index.hip, csrc/predict.hip)
# ---------------------------------------------------------------------------
def index_build(keys):
    """keys int64 [b, n] band keys of the indexed queries (consumed) -> (sorted keys int64 [b, n], ids int32 [b, n],
    directory int32 [qrlsh_index_dir_words])"""
    lib = _lib.load()
    _need(keys, torch.int64, "keys", 2)
    b, n = keys.shape
    dev = keys.device
    ids = torch.empty((b, n), dtype=torch.int32, device=dev)
    ktmp, itmp = torch.empty_like(keys), torch.empty_like(ids)
    dirw = torch.empty((max(int(lib.qrlsh_index_dir_words(n, b)), 1),), dtype=torch.int32, device=dev)
    ws = _ws(lib.qrlsh_index_build_workspace_bytes(n, b), dev)
    _lib.check(lib.qrlsh_index_build(_ptr(keys), _ptr(ktmp), _ptr(ids), _ptr(itmp), n, b, _ptr(dirw), _ptr(ws),
                                     ws.numel(), _stream()))
    return keys, ids, dirw


def index_append(keys, ids, dirw, new_keys):
    """a built index (index_build's or an earlier index_append's keys int64 [b, n], ids int32 [b, n], directory) and
    the band keys int64 [b, m] of m new queries (consumed) -> (keys [b, n + m], ids [b, n + m], directory) of the
    grown index: the new queries get the ids n .. n + m - 1, and the arrays are byte for byte index_build's of the
    concatenated keys.  m == 0 returns the arguments."""
    lib = _lib.load()
    _need(keys, torch.int64, "keys", 2)
    _need(ids, torch.int32, "ids", 2)
    _need(dirw, torch.int32, "dirw", 1)
    _need(new_keys, torch.int64, "new_keys", 2)
    b, n = keys.shape
    m = new_keys.shape[1]
    if tuple(ids.shape) != (b, n) or new_keys.shape[0] != b or new_keys.device != keys.device:
        raise ValueError("ids must be [b, n] and new_keys [b, m] = [%d, m] on the index's device" % b)
    if n and dirw.numel() < int(lib.qrlsh_index_dir_words(n, b)):
        raise ValueError("the directory is shorter than qrlsh_index_dir_words(n, b)")
    if n + m >= 2**32 - 1:
        raise ValueError("at most 2^32 - 2 indexed queries")
    if m == 0:
        return keys, ids, dirw
    dev = keys.device
    keys_out = torch.empty((b, n + m), dtype=torch.int64, device=dev)
    ids_out = torch.empty((b, n + m), dtype=torch.int32, device=dev)
    dir_out = torch.empty((int(lib.qrlsh_index_dir_words(n + m, b)),), dtype=torch.int32, device=dev)
    ws = _ws(lib.qrlsh_index_append_workspace_bytes(m, b), dev)
    _lib.check(lib.qrlsh_index_append(_ptr(keys), _ptr(ids), _ptr(dirw), n, b, _ptr(new_keys), m, _ptr(keys_out),
                                      _ptr(ids_out), _ptr(dir_out), _ptr(ws), ws.numel(), _stream()))
    return keys_out, ids_out, dir_out


def index_probe(sorted_keys, ids, dirw, r, probe_keys):
    """raw candidate words (q * b + band) << 32 | id of every (new query, band) key hit, and the probe workspace
    (per-(query, band) offsets) that index_finish reads"""
    lib = _lib.load()
    b, n = sorted_keys.shape
    _need(probe_keys, torch.int64, "probe_keys", 2)
    m = probe_keys.shape[1]
    dev = probe_keys.device
    ws = _ws(lib.qrlsh_index_probe_workspace_bytes(m, b), dev)
    total = torch.zeros((1,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_index_probe_count(_ptr(sorted_keys), _ptr(dirw), n, b, r, _ptr(probe_keys), m, _ptr(ws),
                                           ws.numel(), _ptr(total), _stream()))
    n_raw = int(total.item())
    raw = torch.empty((max(n_raw, 1),), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_index_probe_fill(_ptr(sorted_keys), _ptr(ids), _ptr(dirw), n, b, r, _ptr(probe_keys), m,
                                          _ptr(ws), ws.numel(), _ptr(raw), _stream()))
    return raw[:n_raw], ws


def index_finish(sig, norm2, probe_sig, probe_norm2, b, probe_ws, raw, K, first_id=None):
    """-> (off int64 [m + 1], idx int32, milli int32, avail int32 [m], keys int64 [n_raw]): the CSR neighbour lists
    and, per raw word, its select key ((1000 - milli) << 32 | id, or -1 for a dropped word).  first_id: probe row q IS
    indexed query first_id + q and stays out of its own list (qrlsh_index_probe_finish_indexed); None: the probe rows
    are strangers to the index."""
    lib = _lib.load()
    n, P = sig.shape
    m = probe_sig.shape[0]
    dev = sig.device
    n_raw = raw.numel()
    code = _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32
    ws = _ws(lib.qrlsh_index_finish_workspace_bytes(m, K, n_raw), dev)
    off = torch.empty((m + 1,), dtype=torch.int64, device=dev)
    idx = torch.empty((max(m * K, 1),), dtype=torch.int32, device=dev)
    milli = torch.empty((max(m * K, 1),), dtype=torch.int32, device=dev)
    avail = torch.empty((m,), dtype=torch.int32, device=dev)
    if first_id is None:
        _lib.check(lib.qrlsh_index_probe_finish(_ptr(sig), _ptr(norm2), n, _ptr(probe_sig), _ptr(probe_norm2), code, P,
                                                b, m, _ptr(probe_ws), _ptr(raw), n_raw, K, _ptr(off), _ptr(idx),
                                                _ptr(milli), _ptr(avail), _ptr(ws), ws.numel(), _stream()))
    else:
        if isinstance(first_id, bool) or not isinstance(first_id, (int, np.integer)) or not 0 <= first_id <= n - m:
            raise ValueError("rows %r .. are not among the %d indexed queries" % (first_id, n))
        _lib.check(lib.qrlsh_index_probe_finish_indexed(_ptr(sig), _ptr(norm2), n, _ptr(probe_sig), _ptr(probe_norm2),
                                                        code, P, b, m, int(first_id), _ptr(probe_ws), _ptr(raw), n_raw,
                                                        K, _ptr(off), _ptr(idx), _ptr(milli), _ptr(avail), _ptr(ws),
                                                        ws.numel(), _stream()))
    cnt = int(off[m].item()) if m else 0
    return off, idx[:cnt], milli[:cnt], avail, ws[:n_raw * 8].view(torch.int64)


def _lists_count_fill(n, dev, count, fill):
    """the tail the list updates share: count(total pointer) leaves the number of entries on the device (~0: the stored
    lists break the contract), fill(cnt, src, dst, val pointers) writes them -> (src, dst, val) new int32 tensors"""
    total = torch.zeros((1,), dtype=torch.int64, device=dev)
    _lib.check(count(_ptr(total)))
    cnt = int(total.item())
    if cnt < 0:     # ~0: the count saw stored lists that break the contract
        raise ValueError("the stored lists are not ordered by src, or hold ids outside [0, %d)" % n)
    out = [torch.empty((max(cnt, 1),), dtype=torch.int32, device=dev) for _ in range(3)]
    _lib.check(fill(cnt, *(_ptr(t) for t in out)))
    return out[0][:cnt], out[1][:cnt], out[2][:cnt]


def lists_update(src, dst, val, n, m, b, K, raw, select_keys, new_off, new_idx, new_milli):
    """The top-K lists (src, dst, val int32 COO: by src, value descending, dst ascending, at most K per src) of a run
    over queries 0 .. n-1, brought up to date with m appended queries n .. n+m-1 (csrc/lists.hip).  raw: index_probe's
    words of the batch probed against the GROWN index; select_keys, new_off, new_idx, new_milli: index_finish's keys
    and lists of that probe with first_id = n and the same K.  -> (src, dst, val): new tensors, element for element the
    lists of a run over all n + m queries with the same K; the arguments are not written.  Raises ValueError for
    K > 256, and for stored lists whose src is not ascending or whose ids lie outside [0, n)."""
    lib = _lib.load()
    for t, name in ((src, "src"), (dst, "dst"), (val, "val"), (new_idx, "new_idx"), (new_milli, "new_milli")):
        _need(t, torch.int32, name, 1)
    for t, name in ((raw, "raw"), (select_keys, "select_keys"), (new_off, "new_off")):
        _need(t, torch.int64, name, 1)
    dev = src.device
    for t in (dst, val, raw, select_keys, new_off, new_idx, new_milli):
        if t.device != dev:
            raise ValueError("every tensor of a list update must live on the lists' device")
    for v, name in ((n, "n"), (m, "m"), (b, "b"), (K, "K")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError("%s must be a non-negative integer, got %r" % (name, v))
    n, m, b, K = int(n), int(m), int(b), int(K)
    if not 1 <= K <= _lib.INDEX_MAX_K:
        raise ValueError("K must lie in 1..%d, got %d" % (_lib.INDEX_MAX_K, K))
    n_edges, n_raw = src.numel(), raw.numel()
    if dst.numel() != n_edges or val.numel() != n_edges:
        raise ValueError("src, dst and val must have one length")
    if select_keys.numel() != n_raw or new_off.numel() != m + 1 or new_idx.numel() != new_milli.numel():
        raise ValueError("select_keys must match raw, new_off hold m + 1 offsets, new_idx match new_milli")
    if b < 1 or n + m >= 2**31 or n_edges >= 2**31 or m * b >= 2**32:
        raise ValueError("a list update needs n + m < 2^31, fewer than 2^31 stored entries and m * b < 2^32")
    if m == 0:
        return src, dst, val
    ws = _ws(lib.qrlsh_lists_update_workspace_bytes(n, m, n_edges, n_raw), dev)
    head = (_ptr(src), _ptr(dst), _ptr(val), n_edges, n, m, b, K)
    return _lists_count_fill(
        n, dev,
        lambda total: lib.qrlsh_lists_update_count(*head, _ptr(raw), _ptr(select_keys), n_raw, _ptr(new_off), _ptr(ws),
                                                   ws.numel(), total, _stream()),
        lambda cnt, *out: lib.qrlsh_lists_update_fill(*head, n_raw, _ptr(new_off), _ptr(new_idx), _ptr(new_milli), _ptr(ws),
                                                      ws.numel(), cnt, *out, _stream()))


# ---------------------------------------------------------------------------
# removing queries from a built index (csrc/remove.hip)
# ---------------------------------------------------------------------------
class IdMap:
    """a set of ids over [0, n) on the device with O(1) membership and rank (qrlsh_idmap_*): .ws its memory, .count its
    members"""

    def __init__(self, ws, n, count):
        self.ws, self.n, self.count = ws, n, count

    def members(self):
        """the members, ascending: int32 [count] (uint32 bit patterns)"""
        out = torch.empty((self.count,), dtype=torch.int32, device=self.ws.device)
        if self.count:
            _lib.check(_lib.load().qrlsh_idmap_list(_ptr(self.ws), self.n, _ptr(out), _stream()))
        return out

    def positions(self):
        """int64 [n]: the rank of every id among the ids outside the set, -1 for a member"""
        out = torch.empty((self.n,), dtype=torch.int64, device=self.ws.device)
        _lib.check(_lib.load().qrlsh_idmap_positions(_ptr(self.ws), self.n, _ptr(out), _stream()))
        return out


def idmap_build(ids, n):
    """ids: int32 device tensor (uint32 bit patterns), any order, duplicates allowed -> IdMap over [0, n); ValueError
    for an id outside [0, n).  One read-back (the member count and the flag word)."""
    lib = _lib.load()
    _need(ids, torch.int32, "ids", 1)
    dev = ids.device
    ws = _ws(lib.qrlsh_idmap_workspace_bytes(n), dev)
    out2 = torch.zeros((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_idmap_build(_ptr(ids), ids.numel(), n, _ptr(ws), ws.numel(), _ptr(out2), _stream()))
    count, flags = out2.tolist()
    if flags & 1:
        raise ValueError("ids must lie in [0, %d)" % n)
    return IdMap(ws, n, count)


def rows_remove(sig, norm2, removed):
    """the rows (and norms) outside the IdMap `removed`, in order: new tensors [n - removed.count]"""
    lib = _lib.load()
    n, P = sig.shape
    row_bytes = P * sig.element_size()
    left = n - removed.count
    sig_out = torch.empty((left, P), dtype=sig.dtype, device=sig.device)
    norm2_out = torch.empty((left,), dtype=torch.int64, device=sig.device)
    if left == 0:
        return sig_out, norm2_out
    _lib.check(lib.qrlsh_rows_remove(_ptr(sig), row_bytes, _ptr(norm2), n, _ptr(removed.ws), _ptr(sig_out),
                                     _ptr(norm2_out), _stream()))
    return sig_out, norm2_out


def index_remove(keys, ids, removed, pick=None):
    """a built index (keys int64 [b, n], ids int32 [b, n]) without the ids of the IdMap `removed`, survivors renumbered
    by rank -> (keys [b, n'], ids [b, n'], directory, pick_keys): byte for byte index_build of the survivors' keys.
    pick: an IdMap over old ids; pick_keys int64 [b, pick.count] then holds the keys those rows are indexed under, in
    pick.members() order (None without pick).  Nothing removed: the arguments come back (directory None)."""
    lib = _lib.load()
    _need(keys, torch.int64, "keys", 2)
    _need(ids, torch.int32, "ids", 2)
    b, n = keys.shape
    if tuple(ids.shape) != (b, n) or removed.n != n or (pick is not None and pick.n != n):
        raise ValueError("ids must be [b, n] and the id maps cover [0, n) = [0, %d)" % n)
    dev = keys.device
    left = n - removed.count
    n_pick = pick.count if pick is not None else 0
    pick_keys = torch.empty((b, n_pick), dtype=torch.int64, device=dev) if pick is not None else None
    if removed.count == 0:
        return keys, ids, None, pick_keys
    if left == 0:
        k0 = torch.empty((b, 0), dtype=torch.int64, device=dev)
        return index_build(k0) + (pick_keys,)
    keys_out = torch.empty((b, left), dtype=torch.int64, device=dev)
    ids_out = torch.empty((b, left), dtype=torch.int32, device=dev)
    dir_out = torch.empty((int(lib.qrlsh_index_dir_words(left, b)),), dtype=torch.int32, device=dev)
    ws = _ws(lib.qrlsh_index_remove_workspace_bytes(n, b), dev)
    _lib.check(lib.qrlsh_index_remove(_ptr(keys), _ptr(ids), n, b, _ptr(removed.ws), removed.count,
                                      _ptr(pick.ws) if n_pick else None, n_pick, _ptr(keys_out), _ptr(ids_out),
                                      _ptr(dir_out), _ptr(pick_keys) if n_pick else None, _ptr(ws), ws.numel(), _stream()))
    return keys_out, ids_out, dir_out, pick_keys


def index_finish_rows(sig, norm2, probe_sig, probe_norm2, b, probe_ws, raw, K, self_ids, want_keys=False):
    """index_finish for probe rows scattered over the index: row q is indexed query self_ids[q] (int32 device tensor
    [m]) and stays out of its own list (qrlsh_index_probe_finish_rows) -> (off, idx, milli, avail); want_keys: and the
    select key of every raw word, as index_finish returns them"""
    lib = _lib.load()
    n, P = sig.shape
    m = probe_sig.shape[0]
    _need(self_ids, torch.int32, "self_ids", 1)
    if self_ids.numel() != m:
        raise ValueError("self_ids must hold one id per probe row")
    dev = sig.device
    n_raw = raw.numel()
    code = _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32
    ws = _ws(lib.qrlsh_index_finish_workspace_bytes(m, K, n_raw), dev)
    off = torch.empty((m + 1,), dtype=torch.int64, device=dev)
    idx = torch.empty((max(m * K, 1),), dtype=torch.int32, device=dev)
    milli = torch.empty((max(m * K, 1),), dtype=torch.int32, device=dev)
    avail = torch.empty((m,), dtype=torch.int32, device=dev)
    _lib.check(lib.qrlsh_index_probe_finish_rows(_ptr(sig), _ptr(norm2), n, _ptr(probe_sig), _ptr(probe_norm2), code, P, b,
                                                 m, _ptr(self_ids), _ptr(probe_ws), _ptr(raw), n_raw, K, _ptr(off),
                                                 _ptr(idx), _ptr(milli), _ptr(avail), _ptr(ws), ws.numel(), _stream()))
    cnt = int(off[m].item()) if m else 0
    if want_keys:
        return off, idx[:cnt], milli[:cnt], avail, ws[:n_raw * 8].view(torch.int64)
    return off, idx[:cnt], milli[:cnt], avail


def _remove_lists_args(src, dst, val, n, K):
    for t, name in ((src, "src"), (dst, "dst"), (val, "val")):
        _need(t, torch.int32, name, 1)
        if t.device != src.device or t.numel() != src.numel():
            raise ValueError("src, dst and val must have one length and one device")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= _lib.INDEX_MAX_K:
        raise ValueError("K must lie in 1..%d, got %r" % (_lib.INDEX_MAX_K, K))
    if n >= 2**31 or src.numel() >= 2**31:
        raise ValueError("lists are kept for fewer than 2^31 queries and entries")


def lists_remove_mark(src, dst, n, K, removed):
    """the rows of the stored lists that a removal has to probe again: surviving rows of exactly K entries with at least
    one removed dst -> IdMap over old ids.  ValueError for stored lists that break the contract."""
    lib = _lib.load()
    _remove_lists_args(src, dst, dst, n, K)
    dev = src.device
    ws = _ws(lib.qrlsh_idmap_workspace_bytes(n), dev)
    out2 = torch.zeros((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_lists_remove_mark(_ptr(src), _ptr(dst), src.numel(), n, int(K), _ptr(removed.ws), _ptr(ws),
                                           _ptr(out2), _stream()))
    count, bad = out2.tolist()
    if bad:
        raise ValueError("the stored lists are not ordered by src, or hold ids outside [0, %d)" % n)
    return IdMap(ws, n, count)


def lists_remove(src, dst, val, n, K, removed, pick, re_off, re_idx, re_milli, re_self):
    """The stored top-K lists without the queries of `removed` (csrc/remove.hip): rows outside `pick` keep their
    surviving entries, renumbered; row pick.members()[j] becomes the re-probed list j (re_off int64 [count + 1], re_idx /
    re_milli int32, re_self int32 [count] = the rows' new ids).  -> (src, dst, val): new tensors ordered by new src."""
    lib = _lib.load()
    _remove_lists_args(src, dst, val, n, K)
    dev = src.device
    n_edges, n_pick = src.numel(), pick.count
    _need(re_off, torch.int64, "re_off", 1)
    for t, name in ((re_idx, "re_idx"), (re_milli, "re_milli"), (re_self, "re_self")):
        _need(t, torch.int32, name, 1)
    if re_off.numel() != n_pick + 1 or re_self.numel() != n_pick or re_idx.numel() != re_milli.numel():
        raise ValueError("re_off must hold count + 1 offsets, re_self count ids, re_idx match re_milli")
    ws = _ws(lib.qrlsh_lists_remove_workspace_bytes(n, n_edges), dev)
    head = (_ptr(src), _ptr(dst), _ptr(val), n_edges, n, int(K), _ptr(removed.ws), _ptr(pick.ws), _ptr(re_off))
    return _lists_count_fill(
        n, dev,
        lambda total: lib.qrlsh_lists_remove_count(*head, n_pick, _ptr(ws), ws.numel(), total, _stream()),
        lambda cnt, *out: lib.qrlsh_lists_remove_fill(*head, _ptr(re_idx), _ptr(re_milli), _ptr(re_self), n_pick, _ptr(ws),
                                                      ws.numel(), cnt, *out, _stream()))


# ---------------------------------------------------------------------------
# changing the list length of stored lists (csrc/listcut.hip)
# ---------------------------------------------------------------------------
def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def lists_cut(src, dst, val, n, K_old, K_new):
    """The stored top-K lists (src, dst, val: by src, value descending, dst ascending, at most K_old per src) cut to
    K_new <= K_old entries per src (csrc/listcut.hip): entry i survives when i < K_new or src[i - K_new] != src[i].
    -> (src, dst, val): new tensors, element for element the lists of a run over the same rows at K_new; the arguments
    are not written.  One read-back (the surviving entries).  ValueError for a K outside 1..256, K_new > K_old, and for
    stored lists whose src is not ascending or outside [0, n) or that hold a row longer than K_old."""
    lib = _lib.load()
    _remove_lists_args(src, dst, val, n, K_old)
    if isinstance(K_new, bool) or not isinstance(K_new, (int, np.integer)) or not 1 <= K_new <= K_old:
        raise ValueError("K_new must lie in 1..K_old = 1..%d, got %r" % (K_old, K_new))
    dev = src.device
    src, dst, val = _aligned16(src), _aligned16(dst), _aligned16(val)
    n_edges = src.numel()
    ws = _ws(lib.qrlsh_lists_cut_workspace_bytes(n_edges), dev)
    total = torch.zeros((1,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_lists_cut_count(_ptr(src), n_edges, int(n), int(K_old), int(K_new), _ptr(ws), ws.numel(),
                                         _ptr(total), _stream()))
    cnt = int(total.item())
    if cnt < 0:     # ~0: the count saw stored lists that break the contract
        raise ValueError("the stored lists are not ordered by src, hold ids outside [0, %d) or a row longer than %d"
                         % (n, K_old))
    out = [torch.empty((max(cnt, 1),), dtype=torch.int32, device=dev) for _ in range(3)]
    _lib.check(lib.qrlsh_lists_cut_fill(_ptr(src), _ptr(dst), _ptr(val), n_edges, int(n), int(K_old), int(K_new), _ptr(ws),
                                        ws.numel(), cnt, *(_ptr(t) for t in out), _stream()))
    return out[0][:cnt], out[1][:cnt], out[2][:cnt]


def lists_regrow_mark(src, n, K_old):
    """the rows of the stored lists that a larger list length has to probe again: those of exactly K_old entries (a
    shorter row was never cut) -> IdMap over [0, n).  One read-back.  ValueError for stored lists that break the
    contract (src not ascending or outside [0, n), a row longer than K_old)."""
    lib = _lib.load()
    _remove_lists_args(src, src, src, n, K_old)
    dev = src.device
    ws = _ws(lib.qrlsh_idmap_workspace_bytes(n), dev)
    out2 = torch.zeros((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_lists_regrow_mark(_ptr(src), src.numel(), int(n), int(K_old), _ptr(ws), _ptr(out2), _stream()))
    count, bad = out2.tolist()
    if bad:
        raise ValueError("the stored lists are not ordered by src, hold ids outside [0, %d) or a row longer than %d"
                         % (n, K_old))
    return IdMap(ws, n, count)


def idmap_empty(n, device):
    """the IdMap over [0, n) without members: zeroed memory is one (no bits, every prefix count 0); no read-back"""
    lib = _lib.load()
    return IdMap(_ws(lib.qrlsh_idmap_workspace_bytes(n), device).zero_(), n, 0)


def index_pick_keys(keys, ids, pick):
    """int64 [b, pick.count]: the keys the rows of the IdMap `pick` are indexed under in a built index (keys int64
    [b, n], ids int32 [b, n]), in pick.members() order -- index_remove's pick_keys without a removal"""
    lib = _lib.load()
    _need(keys, torch.int64, "keys", 2)
    _need(ids, torch.int32, "ids", 2)
    b, n = keys.shape
    if tuple(ids.shape) != (b, n) or pick.n != n:
        raise ValueError("ids must be [b, n] and the id map cover [0, n) = [0, %d)" % n)
    out = torch.empty((b, pick.count), dtype=torch.int64, device=keys.device)
    _lib.check(lib.qrlsh_index_pick_keys(_ptr(keys), _ptr(ids), n, b, _ptr(pick.ws), pick.count, _ptr(out), _stream()))
    return out


# ---------------------------------------------------------------------------
# replacing queries of a built index in place (csrc/replace.hip)
# ---------------------------------------------------------------------------
def rows_replace(sig, norm2, replaced_ids, new_sig, new_norm2):
    """rows (and norms) replaced_ids[x] of sig / norm2 become new_sig[x] / new_norm2[x], IN PLACE (qrlsh_rows_replace);
    replaced_ids: int32 device tensor [m] of distinct ids"""
    lib = _lib.load()
    n, P = sig.shape
    m = new_sig.shape[0]
    _need(replaced_ids, torch.int32, "replaced_ids", 1)
    _need(new_norm2, torch.int64, "new_norm2", 1)
    if new_sig.dtype != sig.dtype or new_sig.shape[1] != P or replaced_ids.numel() != m or new_norm2.numel() != m:
        raise ValueError("the new rows must have the rows' format, with one id and one norm each")
    if not (sig.is_contiguous() and norm2.is_contiguous() and new_sig.is_contiguous()):
        raise ValueError("rows and norms must be contiguous")
    _lib.check(lib.qrlsh_rows_replace(_ptr(sig), P * sig.element_size(), _ptr(norm2), n, _ptr(replaced_ids), _ptr(new_sig),
                                      _ptr(new_norm2), m, _stream()))


def index_replace(keys, ids, dirw, replaced, replaced_ids, new_keys, pick=None):
    """a built index (keys int64 [b, n], ids int32 [b, n], directory) whose queries replaced_ids (int32 [m], ascending;
    `replaced` = their IdMap) take the band keys new_keys int64 [b, m] (consumed) -> (keys [b, n], ids [b, n],
    directory, pick_keys): byte for byte index_build of the key matrix with those columns overwritten.  pick: an IdMap
    of ids outside `replaced`; pick_keys int64 [b, pick.count] = the keys those rows are indexed under (None without)."""
    lib = _lib.load()
    _need(keys, torch.int64, "keys", 2)
    _need(ids, torch.int32, "ids", 2)
    _need(dirw, torch.int32, "dirw", 1)
    _need(new_keys, torch.int64, "new_keys", 2)
    _need(replaced_ids, torch.int32, "replaced_ids", 1)
    b, n = keys.shape
    m = replaced.count
    if tuple(ids.shape) != (b, n) or replaced.n != n or (pick is not None and pick.n != n):
        raise ValueError("ids must be [b, n] and the id maps cover [0, n) = [0, %d)" % n)
    if tuple(new_keys.shape) != (b, m) or replaced_ids.numel() != m or new_keys.device != keys.device:
        raise ValueError("new_keys must be [b, m] = [%d, %d] with one distinct id per column, on the index's device" % (b, m))
    if dirw.numel() < int(lib.qrlsh_index_dir_words(n, b)):
        raise ValueError("the directory is shorter than qrlsh_index_dir_words(n, b)")
    dev = keys.device
    n_pick = pick.count if pick is not None else 0
    pick_keys = torch.empty((b, n_pick), dtype=torch.int64, device=dev) if pick is not None else None
    if m == 0:
        return keys, ids, dirw, pick_keys
    keys_out, ids_out, dir_out = torch.empty_like(keys), torch.empty_like(ids), torch.empty_like(dirw)
    ws = _ws(lib.qrlsh_index_replace_workspace_bytes(n, m, b), dev)
    _lib.check(lib.qrlsh_index_replace(_ptr(keys), _ptr(ids), _ptr(dirw), n, b, _ptr(replaced.ws), _ptr(replaced_ids),
                                       _ptr(new_keys), m, _ptr(pick.ws) if n_pick else None, n_pick, _ptr(keys_out),
                                       _ptr(ids_out), _ptr(dir_out), _ptr(pick_keys) if n_pick else None, _ptr(ws),
                                       ws.numel(), _stream()))
    return keys_out, ids_out, dir_out, pick_keys


def lists_replace(src, dst, val, n, b, K, replaced, replaced_ids, pick, pick_ids, raw, select_keys, r_off, r_idx, r_milli,
                  p_off, p_idx, p_milli):
    """The stored top-K lists after the queries of `replaced` took new rows (csrc/lists.hip).  raw / select_keys /
    r_off / r_idx / r_milli: the probe of the batch against the new index (index_probe, index_finish_rows with
    self_ids = replaced_ids and want_keys); pick / pick_ids: lists_remove_mark's rows over `replaced` and their
    members(); p_off / p_idx / p_milli: their probe.  -> (src, dst, val): new tensors, element for element the lists
    of a run over the new rows at K."""
    lib = _lib.load()
    _remove_lists_args(src, dst, val, n, K)
    dev = src.device
    m, n_pick, n_edges, n_raw = replaced.count, pick.count, src.numel(), raw.numel()
    for t, name in ((raw, "raw"), (select_keys, "select_keys"), (r_off, "r_off"), (p_off, "p_off")):
        _need(t, torch.int64, name, 1)
    for t, name in ((r_idx, "r_idx"), (r_milli, "r_milli"), (p_idx, "p_idx"), (p_milli, "p_milli"),
                    (replaced_ids, "replaced_ids"), (pick_ids, "pick_ids")):
        _need(t, torch.int32, name, 1)
    if (select_keys.numel() != n_raw or r_off.numel() != m + 1 or p_off.numel() != n_pick + 1
            or replaced_ids.numel() != m or pick_ids.numel() != n_pick or r_idx.numel() != r_milli.numel()
            or p_idx.numel() != p_milli.numel()):
        raise ValueError("select_keys must match raw, the offsets hold one more entry than their rows, idx match milli")
    if m * b >= 2**32:
        raise ValueError("a list replacement takes m * b < 2^32 per call")
    ws = _ws(lib.qrlsh_lists_replace_workspace_bytes(n, n_edges, n_raw), dev)
    head = (_ptr(src), _ptr(dst), _ptr(val), n_edges, n, m, int(b), int(K), _ptr(replaced.ws), _ptr(replaced_ids),
            _ptr(pick.ws), _ptr(pick_ids), n_pick)
    return _lists_count_fill(
        n, dev,
        lambda total: lib.qrlsh_lists_replace_count(*head, _ptr(raw), _ptr(select_keys), n_raw, _ptr(r_off), _ptr(p_off),
                                                    _ptr(ws), ws.numel(), total, _stream()),
        lambda cnt, *out: lib.qrlsh_lists_replace_fill(*head, n_raw, _ptr(r_off), _ptr(r_idx), _ptr(r_milli), _ptr(p_off),
                                                       _ptr(p_idx), _ptr(p_milli), _ptr(ws), ws.numel(), cnt, *out,
                                                       _stream()))


def predict_columns(ratings, off, idx, milli, query_weight, user_weight, default_mean, sum_order):
    """int32 [m, nu]: the predicted cells of m new queries for every user (qrlsh_predict_columns); raises ValueError
    when a list is longer than 64 entries or names a query outside the matrix"""
    lib = _lib.load()
    _need(ratings, torch.int32, "ratings", 2)
    nu, nq = ratings.shape
    m = off.numel() - 1
    out = torch.empty((m, nu), dtype=torch.int32, device=ratings.device)
    flags = torch.zeros((1,), dtype=torch.int32, device=ratings.device)
    _lib.check(lib.qrlsh_predict_columns(_ptr(ratings), nu, nq, _ptr(off), _ptr(idx), _ptr(milli), m,
                                         float(query_weight), float(user_weight), float(default_mean), int(sum_order),
                                         _ptr(out), _ptr(flags), _stream()))
    f = int(flags.item())
    if f & 1:
        raise ValueError("a neighbour list is longer than 64 entries; the prediction kernel handles at most 64")
    if f & 2:
        raise ValueError("a neighbour index lies outside the %d columns of the ratings" % nq)
    return out


# ---------------------------------------------------------------------------
# dataset rows come and go under a built index (csrc/tablerows.hip)
# ---------------------------------------------------------------------------
class RowBatch:
    """a batch of dataset rows on the device: .cells int32 [m, nfeat] (the value id = bitmap row of every cell), .slots
    int32 [m] (distinct), with the host's bounds on both -- the kernels gather at them unchecked"""

    def __init__(self, cells, slots, device):
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        slots = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        if cells.ndim != 2 or cells.shape[0] != slots.size or cells.shape[1] < 1:
            raise ValueError("cells must be [m, nfeat] with one slot per row")
        if slots.size and (cells.min() < 0 or slots.min() < 0 or np.unique(slots).size != slots.size):
            raise ValueError("cells and slots must be non-negative, the slots distinct")
        self.m, self.nfeat = cells.shape
        self.cell_hi = int(cells.max()) + 1 if slots.size else 0
        self.slot_hi = int(slots.max()) + 1 if slots.size else 0
        self.cells = torch.from_numpy(cells).to(device)
        self.slots = torch.from_numpy(slots).to(device)


def _table_rows_args(qrows, batch, table, sig):
    _need(qrows, torch.int32, "qrows", 2)
    n, nfeat = qrows.shape
    if sig.dtype not in (torch.int32, torch.int16):
        raise TypeError("sig must be int32 or compact int16 rows")
    _need(sig, sig.dtype, "sig", 2)
    if tuple(sig.shape) != (n, table.P) or nfeat != batch.nfeat:
        raise ValueError("qrows [%d, %d], sig %s and a batch of %d features under a table of %d values do not fit"
                         % (n, nfeat, tuple(sig.shape), batch.nfeat, table.P))
    if batch.slot_hi > table.D:
        raise ValueError("slot %d lies outside the permutation table's %d rows" % (batch.slot_hi - 1, table.D))
    if batch.m > _lib.TABLE_ROWS_MAX_M:
        raise ValueError("at most %d rows per call" % _lib.TABLE_ROWS_MAX_M)
    return n, nfeat, _lib.SIG_U16 if sig.dtype == torch.int16 else _lib.SIG_I32


def table_rows_mark(qrows, batch, table, sig, remove=False):
    """the served queries (qrows int32 [n, nfeat], -1 = unconstrained) that the RowBatch changes under `table`, against
    the index's rows sig: -> (IdMap of the changed queries, matched queries).  remove=False: the batch is added (a
    matched row undercuts a value); True: it leaves (a matched row holds a value) -- call before its bits are cleared.
    One read-back."""
    lib = _lib.load()
    n, nfeat, code = _table_rows_args(qrows, batch, table, sig)
    dev = qrows.device
    ws = _ws(lib.qrlsh_idmap_workspace_bytes(n), dev)
    out2 = torch.zeros((2,), dtype=torch.int64, device=dev)
    _lib.check(lib.qrlsh_table_rows_mark(_ptr(qrows), n, nfeat, _ptr(batch.cells), _ptr(batch.slots), batch.m,
                                         _ptr(table.tab), table.code, table.P, table.P_stride, _ptr(sig), code,
                                         _lib.ROWS_REMOVE if remove else _lib.ROWS_ADD, _ptr(ws), _ptr(out2), _stream()))
    matched, changed = out2.tolist()
    return IdMap(ws, n, changed), matched


def table_rows_fill(qrows, batch, table, sig, changed_ids):
    """the new rows of the changed queries of an added RowBatch (changed_ids: the mark's members, int32 [c] ascending):
    -> (sig [c, P] in sig's format, norm2 int64 [c]); sig itself is not written"""
    lib = _lib.load()
    n, nfeat, code = _table_rows_args(qrows, batch, table, sig)
    _need(changed_ids, torch.int32, "changed_ids", 1)
    c = changed_ids.numel()
    out = torch.empty((c, table.P), dtype=sig.dtype, device=sig.device)
    norm2 = torch.empty((c,), dtype=torch.int64, device=sig.device)
    if c:
        _lib.check(lib.qrlsh_table_rows_fill(_ptr(qrows), n, nfeat, _ptr(batch.cells), _ptr(batch.slots), batch.m,
                                             _ptr(table.tab), table.code, table.P, table.P_stride, _ptr(sig), code,
                                             _ptr(changed_ids), c, _ptr(out), _ptr(norm2), _stream()))
    return out, norm2


def bitmaps_set_rows(bitmaps, batch, live_row, on):
    """set (on=True) or clear the RowBatch's bits in the value rows of bitmaps (int32 [rows, wpr]) and in row live_row"""
    lib = _lib.load()
    _need(bitmaps, torch.int32, "bitmaps", 2)
    rows, wpr = bitmaps.shape
    if batch.cell_hi > rows or not 0 <= live_row < rows or batch.slot_hi > wpr * 32:
        raise ValueError("the batch names a bitmap row or a slot outside the %d x %d-bit bitmaps" % (rows, wpr * 32))
    _lib.check(lib.qrlsh_bitmaps_set_rows(_ptr(bitmaps), wpr, _ptr(batch.cells), _ptr(batch.slots), batch.m, batch.nfeat,
                                          int(live_row), 1 if on else 0, _stream()))
