"""Diversified recommendations: rerank served pools by the stored neighbour lists, and the redundancy of any served
list (qrlsh_diversify, qrlsh_list_redundancy).  The project's own rule; the reference has no counterpart.

sim(a, b) = the largest stored milli value among the list entries a -> b and b -> a, 0 when neither is stored (the
lists are top-K cuts: one direction is often missing, both count).  A pool is a row of top_k / for_users output at
k = N <= 1024: candidates (col, val) in served order.  Greedily, for t = 0 .. k - 1, over the unpicked candidates c:
r_c = max over the picked s of sim(c, s); c is eligible when r_c < max_sim; the eligible c with the largest
1000 * val_c - penalty * r_c (int64) is picked, ties to the smaller pool position; a request ends early when nobody is
eligible.  penalty is rating points x 1000 per unit of similarity, max_sim is in milli (1001: nothing is excluded)."""
import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream

MAX_POOL = _lib.DIVERSIFY_MAX_POOL
MAX_PENALTY = _lib.DIVERSIFY_MAX_PENALTY
WORKSPACE_BUDGET = 1 << 30   # bytes of workspace per library call; more requests are served in row blocks

_FLAG_TEXT = ((1, "a query's neighbour index is outside [0, %(nq)d)"),
              (2, "a candidate column is outside [0, %(nq)d)"),
              (4, "a candidate appears twice in one pool"),
              (8, "a pool's edges do not fit the workspace (a list row names a query twice?)"))


def _int_in(x, lo, hi, name):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError("%s must be an integer in %d..%d, got %r" % (name, lo, hi, x))
    return int(x)


def _check_rule(k, penalty, max_sim):
    return (_int_in(k, 1, MAX_POOL, "k"), _int_in(penalty, 0, MAX_PENALTY, "penalty"),
            _int_in(max_sim, 0, 1001, "max_sim"))


def _int_array(x, ndim, name):
    """an integer tensor / array of `ndim` dimensions (nothing is uploaded)"""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != ndim or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError("%s must be a %d-D integer array, got shape %s %s" % (name, ndim, tuple(t.shape), t.dtype))
    return t


def _coo(q_src, q_dst, q_milli):
    coo = [_int_array(x, 1, n) for n, x in (("q_src", q_src), ("q_dst", q_dst), ("q_milli", q_milli))]
    if not coo[0].numel() == coo[1].numel() == coo[2].numel():
        raise ValueError("q_src, q_dst and q_milli differ in length")
    return coo


def _i32(t, device):
    return t.to(device=device, dtype=torch.int32).contiguous()


def _max_row(q_off):
    """the longest list row (a read-back of one word: it sizes the workspace)"""
    return int((q_off[1:] - q_off[:-1]).max().item()) if q_off.numel() > 1 else 0


def _block(lib, m, n, max_row, device):
    """requests per library call under WORKSPACE_BUDGET, and the workspace for them"""
    blk = m
    while blk > 1 and int(lib.qrlsh_diversify_workspace_bytes(blk, n, max_row)) > WORKSPACE_BUDGET:
        blk = (blk + 1) // 2
    nbytes = max(int(lib.qrlsh_diversify_workspace_bytes(blk, n, max_row)), 16)
    return blk, torch.empty((nbytes,), dtype=torch.uint8, device=device)


def _raise_flags(word, nq):
    for bit, text in _FLAG_TEXT:
        if word & bit:
            raise ValueError(text % {"nq": nq})


def _rerank(ci, cv, av, csr, nq, k, penalty, max_sim, max_row, device):
    """diversify() over device int32 pools and the device CSR of the lists"""
    lib = _lib.load()
    m, n = (int(d) for d in ci.shape)
    idx = torch.empty((m, k), dtype=torch.int32, device=device)
    val = torch.empty((m, k), dtype=torch.int32, device=device)
    red = torch.empty((m, k), dtype=torch.int32, device=device)
    count = torch.empty((m,), dtype=torch.int32, device=device)
    if m == 0:
        return idx, val, red, count
    blk, ws = _block(lib, m, n, max_row, device)
    starts = range(0, m, blk)
    flags = torch.zeros((len(starts),), dtype=torch.int32, device=device)
    st = _stream()
    for b, i0 in enumerate(starts):
        i1 = min(m, i0 + blk)
        _lib.check(lib.qrlsh_diversify(_ptr(ci[i0:i1]), _ptr(cv[i0:i1]), _ptr(av[i0:i1]), i1 - i0, n, nq, _ptr(csr[0]),
                                       _ptr(csr[1]), _ptr(csr[2]), k, penalty, max_sim, _ptr(idx[i0:i1]),
                                       _ptr(val[i0:i1]), _ptr(red[i0:i1]), _ptr(count[i0:i1]), _ptr(flags[b:b + 1]),
                                       _ptr(ws), ws.numel(), st))
    word = 0
    for w in flags.cpu().tolist():   # the one read-back of the call
        word |= int(w)
    _raise_flags(word, nq)
    return idx, val, red, count


def diversify(cand_idx, cand_val, avail, q_src, q_dst, q_milli, nq, k, penalty=0, max_sim=1001, device="cuda"):
    """Rerank pools the caller already has.  cand_idx / cand_val: (m, N) integers, avail: (m,): rows of top_k / for_users
    output at k = N (request x has min(N, avail[x]) candidates, value descending then column ascending).
    q_src / q_dst / q_milli: the query lists in COO form sorted by source, rows of any length; nq: the queries.
    Tensors are used where they are, host data is uploaded.
    -> (idx int32 (m, k), val int32 (m, k), red int32 (m, k), count int32 (m,)) device tensors: the picks' columns and
    values in pick order, the r_c each pick had when it was taken, and the number of picks; idx -1 / val 0 / red 0
    past them.  penalty = 0, max_sim = 1001 returns the first k of every pool with red still filled; max_sim = 1 returns
    sets in which no two entries are stored neighbours.
    Raises ValueError for a bad k, penalty, max_sim, nq or shape, k > N or N > 1024 (before anything is uploaded), and
    for a neighbour index or a candidate column outside [0, nq) and a candidate twice in one pool (through the
    library's flags, read back once; nothing is returned then)."""
    k, penalty, max_sim = _check_rule(k, penalty, max_sim)
    nq = _int_in(nq, 0, 2**31 - 1, "nq")
    ci, cv, av = _int_array(cand_idx, 2, "cand_idx"), _int_array(cand_val, 2, "cand_val"), _int_array(avail, 1, "avail")
    if tuple(ci.shape) != tuple(cv.shape) or av.shape[0] != ci.shape[0]:
        raise ValueError("cand_idx %s, cand_val %s and avail %s do not belong together"
                         % (tuple(ci.shape), tuple(cv.shape), tuple(av.shape)))
    n = int(ci.shape[1])
    if not k <= n <= MAX_POOL:
        raise ValueError("k <= N <= %d is required, got k=%d N=%d" % (MAX_POOL, k, n))
    coo = _coo(q_src, q_dst, q_milli)
    from . import predict
    _lib.load()
    csr = predict.lists_csr(coo, nq, device)
    return _rerank(_i32(ci, device), _i32(cv, device), _i32(av, device), csr, nq, k, penalty, max_sim,
                   _max_row(csr[0]), device)


def default_pool(k):
    return min(MAX_POOL, max(4 * k, 64))


def _check_pool(k, pool):
    pool = default_pool(k) if pool is None else _int_in(pool, 1, MAX_POOL, "pool")
    if pool < k:
        raise ValueError("k <= pool <= %d is required, got k=%d pool=%d" % (MAX_POOL, k, pool))
    return pool


def for_users_diverse(ratings, q_src, q_dst, q_milli, user_sims, users, k, pool=None, penalty=0, max_sim=1001, lo=0,
                      slices=0, sum_order="pairwise", query_weight=None, user_weight=None, default_mean=None,
                      device="cuda"):
    """for_users at k = pool, then diversify over its output: the pools never leave the device, and the lists are
    uploaded once.  pool: candidates per user, default min(1024, max(4 k, 64)); the remaining arguments as for_users
    and diversify take them.
    -> (idx, val, red, count, avail) device tensors: diversify's four, and for_users' avail (the eligible cells).
    Raises what for_users and diversify raise; every check that needs no device precedes any upload."""
    from . import predict, recommend
    k, penalty, max_sim = _check_rule(k, penalty, max_sim)
    pool = _check_pool(k, pool)
    recommend._check_select_args(pool, lo, slices)
    a = predict.ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, users, sum_order)
    _lib.load()
    a.upload(device)
    ci, cv, av = recommend._serve(a, pool, int(lo), int(slices), query_weight, user_weight, default_mean, device)
    idx, val, red, count = _rerank(ci, cv, av, (a.q_off, a.q_idx, a.q_milli), a.nq, k, penalty, max_sim,
                                   _max_row(a.q_off), device)
    return idx, val, red, count, av


class Redundancy:
    """.words int64 (m, 4) per list: entries listed, unordered in-list pairs with sim > 0, the sum of sim (milli) over
    them, the largest sim; .totals int64 (4,): the sums of the first three and the max of the last;
    .pairs_per_list = totals[1] / m; .mean_sim = totals[2] / totals[1] / 1000 (0.0 without pairs)."""

    def __init__(self, words, totals):
        self.words, self.totals = words, totals
        m = int(words.shape[0])
        self.pairs_per_list = float(totals[1]) / m if m else 0.0
        self.mean_sim = float(totals[2]) / float(totals[1]) / 1000.0 if int(totals[1]) else 0.0

    def __repr__(self):
        return "Redundancy(lists=%d, entries=%d, pairs=%d, sim_sum=%d, max_sim=%d)" % (
            (self.words.shape[0],) + tuple(int(x) for x in self.totals))


def list_redundancy(idx, q_src, q_dst, q_milli, nq, device="cuda"):
    """The redundancy of served lists.  idx: (m, k <= 1024) integer columns, -1 = padding (any served idx array);
    the lists and nq as diversify takes them.  -> Redundancy (host arrays; one read-back).
    Raises ValueError for a bad shape or nq (before anything is uploaded), and for a neighbour index or a column
    outside [0, nq) and a column twice in one list (through the library's flags)."""
    nq = _int_in(nq, 0, 2**31 - 1, "nq")
    li = _int_array(idx, 2, "idx")
    m, k = (int(d) for d in li.shape)
    if not 1 <= k <= MAX_POOL:
        raise ValueError("lists of 1..%d entries are served, got k=%d" % (MAX_POOL, k))
    coo = _coo(q_src, q_dst, q_milli)
    from . import predict
    lib = _lib.load()
    csr = predict.lists_csr(coo, nq, device)
    li = _i32(li, device)
    out = torch.zeros((4 * m + 5,), dtype=torch.int64, device=device)   # [words m x 4][totals 4][flag]
    if m:
        blk, ws = _block(lib, m, k, _max_row(csr[0]), device)
        st = _stream()
        for i0 in range(0, m, blk):
            i1 = min(m, i0 + blk)
            _lib.check(lib.qrlsh_list_redundancy(_ptr(li[i0:i1]), i1 - i0, k, nq, _ptr(csr[0]), _ptr(csr[1]),
                                                 _ptr(csr[2]), _ptr(out[4 * i0:]), _ptr(out[4 * m:]),
                                                 _ptr(out[4 * m + 4:]), _ptr(ws), ws.numel(), st))
    host = out.cpu().numpy()
    _raise_flags(int(host[4 * m + 4]), nq)
    return Redundancy(host[:4 * m].reshape(m, 4).copy(), host[4 * m:4 * m + 4].copy())
