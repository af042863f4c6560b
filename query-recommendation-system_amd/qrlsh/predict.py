"""N1 -- the hybrid prediction loop on the device (recommender.py:301-331).

fill_predictions() takes the utility matrix, the query top-K lists in the COO form the hot path
returns, and the user top-K lists, and returns the completed matrix (qrlsh_predict).
predict_users() returns the completed rows of chosen users only, straight from the lists (qrlsh_predict_users);
qrlsh.recommend.for_users() selects their top-k from the same sweep."""
import numpy as np
import torch

from . import _lib
from . import ops
from .ops import _ptr, _stream

QUERY_WEIGHT = 0.6   # recommender.py:32-34
USER_WEIGHT = 0.4
DEFAULT_MEAN = 60


MAX_NEIGHBOURS = 64   # PRED_MAXK in csrc/predict.hip


def user_lists(user_sims, nu, device):
    """user_sims: {u: {'indexes', 'values'}} as compute_userSimilarities returns it (users without an entry get an
    empty list).  -> (u_idx int32 (nu, max(ku, 1)) padded with -1, u_val float64 of the same shape padded with 0,
    ku = the longest list): the form the library takes user lists in.  A server prepares it once and passes the
    tuple wherever `user_sims` is taken.  Raises ValueError when a list is longer than 64."""
    ku = max((len(user_sims[u]["indexes"]) for u in user_sims), default=0)
    if ku > MAX_NEIGHBOURS:
        raise ValueError("a user has %d neighbours; the prediction kernel handles at most %d" % (ku, MAX_NEIGHBOURS))
    ui = np.full((nu, max(ku, 1)), -1, dtype=np.int32)
    uv = np.zeros((nu, max(ku, 1)), dtype=np.float64)
    for u in range(nu):
        if u in user_sims:
            n = len(user_sims[u]["indexes"])
            ui[u, :n] = user_sims[u]["indexes"]
            uv[u, :n] = user_sims[u]["values"]
    return torch.from_numpy(ui).to(device), torch.from_numpy(uv).to(device), ku


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
    if sum_order not in ("pairwise", "sequential"):
        raise ValueError("sum_order must be 'pairwise' or 'sequential'")
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
                                 float(default_mean),
                                 _lib.SUM_SEQUENTIAL if sum_order == "sequential" else _lib.SUM_PAIRWISE,
                                 _ptr(out), _ptr(too_long), kq, _ptr(ws) if kq else None, ws.numel(), _stream()))
    if int(too_long.item()):
        raise ValueError("a query has more than %d neighbours (max_candidates overridden?); the prediction kernel "
                         "handles at most %d" % (MAX_NEIGHBOURS, MAX_NEIGHBOURS))
    return out


def lists_csr(coo, nq, device):
    """coo: (q_src, q_dst, q_milli) 1-D integer tensors sorted by source -> the device CSR the serving kernels take:
    (q_off int64 (nq + 1,), q_idx int32, q_milli int32).  ValueError for a source outside [0, nq)."""
    src = coo[0].to(device=device, dtype=torch.int64)
    try:
        counts = torch.bincount(src, minlength=nq)
    except RuntimeError:   # a negative id
        counts = None
    if counts is None or counts.numel() != nq:
        raise ValueError("a list's source query is outside [0, %d)" % nq)
    q_off = torch.zeros((nq + 1,), dtype=torch.int64, device=device)
    torch.cumsum(counts, dim=0, out=q_off[1:])
    return (q_off, coo[1].to(device=device, dtype=torch.int32).contiguous(),
            coo[2].to(device=device, dtype=torch.int32).contiguous())


class ServeInputs:
    """The checked arguments of predict_users / recommend.for_users, and (after upload()) their device form.
    Every check that needs no device runs in the constructor, before anything is uploaded or the library loaded.
    ids = "queries": `users` holds query ids instead (predict_queries / for_queries / query_utility): the same checks
    against nq, None = every column."""

    def __init__(self, ratings, q_src, q_dst, q_milli, user_sims, users, sum_order, ids="users"):
        from .recommend import _matrix
        if sum_order not in ("pairwise", "sequential"):
            raise ValueError("sum_order must be 'pairwise' or 'sequential'")
        self.sum_order = _lib.SUM_SEQUENTIAL if sum_order == "sequential" else _lib.SUM_PAIRWISE
        self.ratings = _matrix(ratings, "ratings")
        self.nu, self.nq = (int(d) for d in self.ratings.shape)
        if self.nq >= 2**31:
            raise ValueError("at most 2^31 - 1 queries per row")
        self.what = "user" if ids == "users" else "query"
        self.bound = self.nu if ids == "users" else self.nq   # the ids lie in [0, bound)
        if ids != "users" and self.nu >= 2**31:
            raise ValueError("at most 2^31 - 1 users per column")
        coo = []
        for name, x in (("q_src", q_src), ("q_dst", q_dst), ("q_milli", q_milli)):
            t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
            if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
                raise ValueError("%s must be a 1-D integer array" % name)
            coo.append(t)
        if not coo[0].numel() == coo[1].numel() == coo[2].numel():
            raise ValueError("q_src, q_dst and q_milli differ in length")
        self.coo = coo
        if isinstance(user_sims, tuple):
            u_idx, u_val, ku = user_sims
            if (u_idx.dim() != 2 or tuple(u_idx.shape) != tuple(u_val.shape) or u_idx.shape[0] != self.nu
                    or u_idx.dtype != torch.int32 or u_val.dtype != torch.float64):
                raise ValueError("prepared user lists must be user_lists(user_sims, %d, device)" % self.nu)
            if not 0 <= int(ku) <= min(MAX_NEIGHBOURS, u_idx.shape[1]):
                raise ValueError("a user has %d neighbours; the prediction kernel handles at most %d"
                                 % (ku, MAX_NEIGHBOURS))
        else:
            ku = max((len(user_sims[u]["indexes"]) for u in user_sims), default=0)
            if ku > MAX_NEIGHBOURS:
                raise ValueError("a user has %d neighbours; the prediction kernel handles at most %d"
                                 % (ku, MAX_NEIGHBOURS))
        self.user_sims = user_sims
        self.device_ids = False
        if users is None:
            self.users, self.m = None, self.bound
        elif isinstance(users, torch.Tensor):
            if users.dim() != 1 or users.dtype.is_floating_point or users.dtype == torch.bool:
                raise ValueError("%s must be a 1-D integer tensor" % ids)
            self.users, self.m, self.device_ids = users, int(users.numel()), True
        else:
            ua = np.asarray(users)
            if ua.ndim != 1 or not (ua.size == 0 or np.issubdtype(ua.dtype, np.integer)):
                raise ValueError("%s must be a 1-D sequence of integer %s ids"
                                 % (ids, "row" if ids == "users" else "column"))
            if ua.size and (ua.min() < 0 or ua.max() >= self.bound):
                raise ValueError("%s id outside [0, %d)" % (self.what, self.bound))
            self.users, self.m = ua, int(ua.size)

    def upload(self, device):
        from .recommend import _on_device
        self.r = _on_device(self.ratings, device)
        self.q_off, self.q_idx, self.q_milli = lists_csr(self.coo, self.nq, device)
        us = self.user_sims
        u_idx, u_val, ku = us if isinstance(us, tuple) else user_lists(us, self.nu, device)
        self.u_idx, self.u_val = u_idx.to(device).contiguous(), u_val.to(device).contiguous()
        self.ku = self.u_idx.shape[1] if ku else 0
        u = self.users
        if u is not None:   # ids past int32 must stay out of range, not wrap into it
            u = u if isinstance(u, torch.Tensor) else torch.from_numpy(u.astype(np.int64))
            u = u.to(device=device, dtype=torch.int64).clamp(-1, self.bound).to(torch.int32).contiguous()
        self.ut = u
        return self

    def lists_args(self, query_weight, user_weight, default_mean):
        """the arguments both entry points share, up to `users`"""
        return (_ptr(self.r), self.nu, self.nq, _ptr(self.q_off), _ptr(self.q_idx), _ptr(self.q_milli),
                _ptr(self.u_idx), _ptr(self.u_val), self.ku, float(query_weight), float(user_weight),
                float(default_mean), self.sum_order)

    def raise_flags(self, flags):
        """flags: the library's flag words of the calls made (one read-back)"""
        f = 0
        for w in flags.cpu().tolist():
            f |= int(w)
        if f & 1:
            raise ValueError("a query has more than %d neighbours (max_candidates overridden?); the prediction kernel "
                             "handles at most %d" % (MAX_NEIGHBOURS, MAX_NEIGHBOURS))
        if f & 2:
            raise ValueError("a query's neighbour index is outside [0, %d)" % self.nq)
        if f & 4:
            bad = torch.nonzero((self.ut < 0) | (self.ut >= self.bound))
            pos = int(bad[0, 0].item()) if bad.numel() else -1
            raise ValueError("%s id %s (position %d) outside [0, %d)"
                             % (self.what, int(self.users[pos].item()) if pos >= 0 else "?", pos, self.bound))


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
