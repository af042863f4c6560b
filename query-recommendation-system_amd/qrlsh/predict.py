"""N1 -- the hybrid prediction loop on the device (recommender.py:301-331).

fill_predictions() takes the utility matrix, the query top-K lists in the COO form the hot path
returns, and the user top-K lists, and returns the completed matrix (qrlsh_predict).
predict_users() returns the completed rows of chosen users only, straight from the lists (qrlsh_predict_users);
qrlsh.recommend.for_users() selects their top-k from the same sweep."""
import numpy as np
import torch

from . import _lib
from . import ops
from ._inputs import LIST_FLAGS, MAX_NEIGHBOURS, raise_flags, sum_order_code
from ._inputs import ServeInputs, lists_csr, user_lists  # noqa: F401  (re-exported: qrlsh.predict.lists_csr, ...)
from .ops import _ptr, _stream

QUERY_WEIGHT = 0.6   # recommender.py:32-34
USER_WEIGHT = 0.4
DEFAULT_MEAN = 60


def weights(query_weight=None, user_weight=None, default_mean=None):
    """(query_weight, user_weight, default_mean), None = the default above"""
    return (QUERY_WEIGHT if query_weight is None else query_weight, USER_WEIGHT if user_weight is None else user_weight,
            DEFAULT_MEAN if default_mean is None else default_mean)


def fill_predictions(ratings, q_src, q_dst, q_milli, user_sims, query_weight=QUERY_WEIGHT,
                     user_weight=USER_WEIGHT, default_mean=DEFAULT_MEAN, device="cuda", sum_order="pairwise",
                     transpose_lists=True):
    """ratings: (nu, nq) integer array / tensor, 0 = missing.
    q_src/q_dst/q_milli: the hot path's top-K COO (sorted by src; value = milli / 1000).
    user_sims: {u: {'indexes', 'values'}} as compute_userSimilarities returns it.
    sum_order: "pairwise" (numpy's np.sum order: the reference as plain Python, what the fixtures pin) or
    "sequential" (numba's nopython np.sum: the reference where numba is installed; unpinned).
    transpose_lists: give the library a workspace and the longest list (one extra read-back), so that it runs its
    tile form (64 users x 16 queries per workgroup over a byte copy of the matrix) or, for ratings outside 0 .. 255,
    its row form; False: one thread per cell over the CSR lists.  Same results.
    -> int32 device tensor (nu, nq): finalPredictions of recommender.py:301-331.
    Raises ValueError when a neighbour list is longer than 64 (K = round(log_1.5 n) stays below 52 for any
    n < 1e9; only an overridden max_candidates gets there)."""
    sum_order = sum_order_code(sum_order)
    lib = _lib.load()
    r = torch.as_tensor(np.ascontiguousarray(np.asarray(ratings), dtype=np.int32)) if not isinstance(ratings, torch.Tensor) else ratings.to(torch.int32)
    r = r.to(device).contiguous()
    nu, nq = r.shape
    q_src = q_src.to(device)
    counts = torch.bincount(q_src.to(torch.int64), minlength=nq)
    q_off = torch.zeros((nq + 1,), dtype=torch.int64, device=device)
    torch.cumsum(counts, dim=0, out=q_off[1:])
    q_idx = q_dst.to(device).to(torch.int32).contiguous()
    # milli / 1000 correctly rounded, as the reference's np.around values are.  The divisor is a device tensor: with
    # a Python-scalar divisor torch's GPU kernel multiplies by the reciprocal, which is an ulp off for 144 of the
    # 1001 milli values and moves predictions that lie on the edge of a rounding step.
    thousand = torch.full((), 1000.0, dtype=torch.float64, device=device)
    q_val = (q_milli.to(device).to(torch.float64) / thousand).contiguous()
    u_idx, u_val, ku = user_lists(user_sims, nu, device)
    out = torch.empty((nu, nq), dtype=torch.int32, device=device)
    too_long = torch.zeros((1,), dtype=torch.int32, device=device)
    # the longest query list (one read-back): the kernel sweeps the lists transposed to [kq][nq]
    kq = int(counts.max().item()) if (nq and transpose_lists) else 0
    if kq > MAX_NEIGHBOURS:
        raise ValueError("a query has more than %d neighbours (%d; max_candidates overridden?); the prediction kernel "
                         "handles at most %d" % (MAX_NEIGHBOURS, kq, MAX_NEIGHBOURS))
    ws = ops._ws(lib.qrlsh_predict_workspace_bytes(nu, nq, kq), device)
    _lib.check(lib.qrlsh_predict(_ptr(r), nu, nq, _ptr(q_off), _ptr(q_idx), _ptr(q_val), _ptr(u_idx), _ptr(u_val),
                                 u_idx.shape[1] if ku else 0, float(query_weight), float(user_weight),
                                 float(default_mean), sum_order, _ptr(out), _ptr(too_long), kq,
                                 _ptr(ws) if kq else None, ws.numel(), _stream()))
    if int(too_long.item()):
        raise_flags(1, LIST_FLAGS, max=MAX_NEIGHBOURS)
    return out


def predict_users(ratings, q_src, q_dst, q_milli, user_sims, users, query_weight=QUERY_WEIGHT, user_weight=USER_WEIGHT,
                  default_mean=DEFAULT_MEAN, device="cuda", sum_order="pairwise"):
    """The completed rows of chosen users, straight from the lists: rows `users` of fill_predictions' result, cell for
    cell, without the (nu, nq) matrix (qrlsh_predict_users).
    ratings: (nu, nq) utility matrix, a tensor (used where it is) or host data (uploaded as int32).
    q_src / q_dst / q_milli: the query lists in COO form sorted by source, as a run's res.src / dst / val and
    QueryIndex.lists hold them.  user_sims: compute_userSimilarities' dict, or user_lists(...)'s tuple prepared once.
    users: row ids (any order, repeats allowed; a host sequence or a device tensor), None = every row.
    -> int32 device tensor (m, nq).
    Raises ValueError for a bad shape or sum_order, a list longer than 64, a neighbour index outside [0, nq) and a user
    id outside [0, nu) (host ids before anything is uploaded; device ids and the lists through the library's flags)."""
    a = ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, users, sum_order)
    lib = _lib.load()
    a.upload(device)
    out = torch.empty((a.m, a.nq), dtype=torch.int32, device=device)
    if a.m == 0:
        return out
    flags = torch.zeros((1,), dtype=torch.int32, device=device)
    _lib.check(lib.qrlsh_predict_users(*a.lists_args(query_weight, user_weight, default_mean),
                                       None if a.ut is None else _ptr(a.ut), a.m, _ptr(out), _ptr(flags), None, 0,
                                       _stream()))
    a.raise_flags(flags)
    return out
