"""Top-k unrated queries for every requested user, on the device (qrlsh_recommend_topk).

The batch form of the selection inside the reference's interactive prompt (recommender.py:357-375): for user u the
eligible queries are those it has not rated and that have a non-zero prediction (`just_scored`, :361); the k with the
largest predicted value come first, ties broken by query index ascending (the project's tie rule; the reference's
np.argsort order among equal values is arbitrary)."""
import numpy as np
import torch

from . import _lib
from . import ops
from . import predict
from ._args import _int_in
from ._inputs import WORKSPACE_BUDGET, blocks, ids32, request_blocks, select_ids
from ._inputs import matrix as _matrix, on_device as _on_device
from .ops import _ptr, _stream

MAX_K = _lib.RECOMMEND_MAX_K
MAX_SLICES = 256


def top_k(ratings, predictions, k, users=None, lo=0, slices=0, device="cuda"):
    """ratings: (nu, nq) utility matrix, 0 = unrated; predictions: (nu, nq) completed matrix (fill_predictions'
    output, or compute_scores' DataFrame); tensors are used where they are, host data is uploaded as int32.
    users: row ids to serve (any order, repeats allowed), default all rows in order.  lo: start of the value window
    of the fast path (values outside [lo, lo + 4096) take the radix refinement; same result).  slices: column
    slices per row (1 .. 256), 0 = chosen by the library.
    -> (idx int32 (m, k), val int32 (m, k), avail int32 (m,)) device tensors: per requested user the query columns
    with the largest predictions among its eligible cells (value descending, index ascending), their values, and
    the number of eligible cells; idx -1 / val 0 past min(k, avail).
    Raises ValueError for a bad k, slices or shape and for a user id outside [0, nu) (host ids are checked before
    anything is uploaded; ids given as a device tensor through the library's per-row flag)."""
    k = _check_select_args(k, lo, slices)
    r = _matrix(ratings, "ratings")
    p = _matrix(predictions, "predictions")
    if tuple(r.shape) != tuple(p.shape):
        raise ValueError("ratings %s and predictions %s differ in shape" % (tuple(r.shape), tuple(p.shape)))
    nu, nq = (int(d) for d in r.shape)
    if nq >= 2**31:
        raise ValueError("at most 2^31 - 1 queries per row")
    m, u, check_flag = select_ids(users, nu, "user", "users")

    lib = _lib.load()
    rt, pt = _on_device(r, device), _on_device(p, device)
    idx = torch.empty((m, k), dtype=torch.int32, device=device)
    val = torch.empty((m, k), dtype=torch.int32, device=device)
    avail = torch.empty((m,), dtype=torch.int32, device=device)
    if m == 0:
        return idx, val, avail

    def need(blk):
        return int(lib.qrlsh_recommend_workspace_bytes(blk, nq, k, int(slices)))
    blk, ut = request_blocks(m, need, WORKSPACE_BUDGET, ids=None if u is None else ids32(u, nu, device), full=nu,
                             device=device)
    ws = ops._ws(need(blk), device)
    st = _stream()
    for _, i0, i1 in blocks(m, blk):
        _lib.check(lib.qrlsh_recommend_topk(_ptr(rt), _ptr(pt), nu, nq, None if ut is None else _ptr(ut[i0:i1]),
                                            i1 - i0, k, int(lo), int(slices), _ptr(idx[i0:i1]), _ptr(val[i0:i1]),
                                            _ptr(avail[i0:i1]), _ptr(ws), ws.numel(), st))
    if check_flag and bool((avail < 0).any().item()):
        bad = int(torch.nonzero(avail < 0)[0, 0].item())
        raise ValueError("user id %d (position %d) outside [0, %d)" % (int(u[bad].item()), bad, nu))
    return idx, val, avail


def _check_select_args(k, lo, slices):
    """top_k's and for_users' checks of k, lo and slices -> k as an int"""
    k = _int_in(k, "k", 1, MAX_K)
    _int_in(slices, "slices", 0, MAX_SLICES)
    if isinstance(lo, bool) or not isinstance(lo, (int, np.integer)) or not -2**31 <= int(lo) < 2**31:
        raise ValueError("lo must be an int32, got %r" % (lo,))
    return k


def for_users(ratings, q_src, q_dst, q_milli, user_sims, users, k, lo=0, slices=0, sum_order="pairwise",
              query_weight=None, user_weight=None, default_mean=None, device="cuda"):
    """Top-k unrated queries of chosen users from the live lists, without a prediction matrix
    (qrlsh_recommend_users): what top_k(ratings, fill_predictions(...), k, users=users) returns, output for output.
    ratings, the lists, user_sims and users as predict.predict_users takes them (tensors are used where they are, host
    data is uploaded); k, lo and slices as top_k takes them.  Served in row blocks under WORKSPACE_BUDGET.
    -> (idx int32 (m, k), val int32 (m, k), avail int32 (m,)) device tensors.
    Raises ValueError for a bad k, slices, lo, shape or sum_order, a list longer than 64, a neighbour index outside
    [0, nq) and a user id outside [0, nu) (host ids before anything is uploaded; device ids and the lists through
    the library's flags)."""
    k = _check_select_args(k, lo, slices)
    a = predict.ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, users, sum_order)
    _lib.load()
    a.upload(device)
    return _serve(a, k, int(lo), int(slices), query_weight, user_weight, default_mean, device)


def _serve(a, k, lo, slices, query_weight, user_weight, default_mean, device):
    """for_users over checked and uploaded ServeInputs (for_users_diverse shares them with its rerank)"""
    m, nq = a.m, a.nq
    lib = _lib.load()
    idx = torch.empty((m, k), dtype=torch.int32, device=device)
    val = torch.empty((m, k), dtype=torch.int32, device=device)
    avail = torch.empty((m,), dtype=torch.int32, device=device)
    if m == 0:
        return idx, val, avail

    def need(blk):
        return int(lib.qrlsh_recommend_users_workspace_bytes(blk, nq, k, int(slices)))
    blk, ut = request_blocks(m, need, WORKSPACE_BUDGET, ids=a.ut, full=a.nu, device=device)
    ws = ops._ws(need(blk), device)
    parts = blocks(m, blk)
    flags = torch.zeros((len(parts),), dtype=torch.int32, device=device)
    args = a.lists_args(*predict.weights(query_weight, user_weight, default_mean))
    st = _stream()
    for b, i0, i1 in parts:
        _lib.check(lib.qrlsh_recommend_users(*args, None if ut is None else _ptr(ut[i0:i1]), i1 - i0, k, int(lo),
                                             int(slices), _ptr(idx[i0:i1]), _ptr(val[i0:i1]), _ptr(avail[i0:i1]),
                                             _ptr(flags[b:b + 1]), _ptr(ws), ws.numel(), st))
    a.raise_flags(flags)
    return idx, val, avail
