"""What the wrappers above the C ABI share: the checks that turn caller data into library arguments, the request
blocks of a call that does not fit its workspace budget, and the reading of the library's flag words.

One copy of each; depends on _lib, ops, numpy and torch only.  Every check that needs no device runs before anything is
uploaded or the library loaded."""
import numpy as np
import torch

from . import _lib
from .ops import _ptr

WORKSPACE_BUDGET = 1 << 30   # bytes of workspace per library call; larger request sets are served in blocks
MAX_REQUESTS = 1 << 24       # requests per library call of the sweeps over the answer sets (fidelity, exactlists)
MAX_NEIGHBOURS = 64          # PRED_MAXK in csrc/predict.hip
SUM_ORDERS = {"pairwise": _lib.SUM_PAIRWISE, "sequential": _lib.SUM_SEQUENTIAL}
# the tensor dtypes that count as integers: one set lookup per argument instead of three attribute tests (bool is none)
INT_DTYPES = frozenset(getattr(torch, n) for n in ("uint8", "int8", "int16", "int32", "int64", "uint16", "uint32",
                                                   "uint64") if hasattr(torch, n))


# ------------------------------------------------------------------------------------------------ argument checks
def sum_order_code(sum_order):
    """'pairwise' / 'sequential' -> the library's code"""
    if sum_order not in SUM_ORDERS:
        raise ValueError("sum_order must be 'pairwise' or 'sequential'")
    return SUM_ORDERS[sum_order]


def matrix(x, name):
    """2-D int32 view of a tensor / array / DataFrame; host data is checked to fit int32 (nothing is uploaded)"""
    if isinstance(x, torch.Tensor):
        if x.dim() != 2:
            raise ValueError("%s must be 2-D, got shape %s" % (name, tuple(x.shape)))
        if x.dtype not in INT_DTYPES:
            raise ValueError("%s must hold integers, got %s" % (name, x.dtype))
        return x
    a = np.asarray(x.to_numpy() if hasattr(x, "to_numpy") else x)
    if a.ndim != 2:
        raise ValueError("%s must be 2-D, got shape %s" % (name, a.shape))
    if a.dtype != np.int32:
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("%s must hold integers, got %s" % (name, a.dtype))
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
            raise ValueError("%s holds values outside int32" % name)
    return a


def on_device(x, device):
    """matrix()'s result as a contiguous int32 device tensor on a 16-byte-aligned base"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))
    t = t.to(device=device, dtype=torch.int32).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()   # the kernels read rows as 16-byte vectors from a 16-byte-aligned base
    return t


def like_matrix(x, name, shape, other):
    """matrix(x, name), which must have the shape of the matrix `other`"""
    x = matrix(x, name)
    if tuple(int(d) for d in x.shape) != tuple(shape):
        raise ValueError("%s has shape %s, %s %s" % (name, tuple(x.shape), other, tuple(shape)))
    return x


def int_array(x, ndim, name):
    """x (a tensor or host data) as an integer tensor of `ndim` dimensions (None: any); nothing is uploaded.  An empty
    1-D host sequence has no dtype of its own and counts as integer."""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
        if x.ndim == 1 and x.size == 0:
            x = x.astype(np.int64)
        x = torch.as_tensor(x)
    if (ndim is not None and x.dim() != ndim) or x.dtype not in INT_DTYPES:
        raise ValueError("%s must be %s integer array, got shape %s %s"
                         % (name, "an" if ndim is None else "a %d-D" % ndim, tuple(x.shape), x.dtype))
    return x


def coo_triple(q_src, q_dst, q_milli):
    """the query lists in COO form: three 1-D integer arrays of one length -> [src, dst, milli] tensors"""
    coo = [int_array(x, 1, n) for n, x in (("q_src", q_src), ("q_dst", q_dst), ("q_milli", q_milli))]
    if not coo[0].numel() == coo[1].numel() == coo[2].numel():
        raise ValueError("q_src, q_dst and q_milli differ in length")
    return coo


def answer_csr(offsets, rows):
    """the CSR answer sets: 1-D integer (offsets of nq + 1 entries, rows), nq < 2^31 -> the two as tensors"""
    off, r = int_array(offsets, 1, "offsets"), int_array(rows, 1, "rows")
    if off.numel() < 1:
        raise ValueError("offsets must hold nq + 1 entries")
    if off.numel() - 1 >= 2**31:
        raise ValueError("at most 2^31 - 1 queries")
    return off, r


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


def select_ids(ids, bound, what, name, host_tensors=False):
    """The analysis of an id selection (`users=`, `queries=`): None = all `bound` of them, a device tensor, or a host
    sequence, whose ids are held to [0, bound) here, before any upload (host_tensors: a CPU tensor is host data too).
    -> (m, None / the tensor / an int64 host array, whether the library's flag has to vouch for the ids)."""
    if ids is None:
        return bound, None, False
    if isinstance(ids, torch.Tensor) and not (host_tensors and not ids.is_cuda):
        if ids.dim() != 1 or ids.dtype not in INT_DTYPES:
            raise ValueError("%s must be a 1-D integer tensor" % name)
        return int(ids.numel()), ids, True
    a = ids.numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    if a.ndim != 1 or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("%s must be a 1-D sequence of integer %s ids in [0, %d)" % (name, what, bound))
    if a.size and (a.min() < 0 or a.max() >= bound):
        raise ValueError("%s id outside [0, %d)" % (what, bound))
    return int(a.size), a.astype(np.int64), False


def ids32(ids, bound, device):
    """ids (a tensor or a host array) as int32 on the device; ids past int32 stay out of range (-1 or bound) instead of
    wrapping into it"""
    t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(ids)
    return t.to(device=device, dtype=torch.int64).clamp(-1, bound).to(torch.int32).contiguous()


# ------------------------------------------------------------------------------------------------- request blocks
def request_blocks(m, need, budget, ids=None, full=None, device=None, group=1, cap=None):
    """The requests per library call: m (at most `cap`), halved (rounding up) while need(blk) bytes exceed `budget`
    and more than `group` are left, then rounded up to whole groups.  A selection that names nobody
    (ids = None: all `full` ids in order) gets its ids once it is split, since a later block no longer starts at id 0.
    -> (blk, ids)"""
    blk = max(m, 1) if cap is None else min(max(m, 1), cap)
    while blk > group and need(blk) > budget:
        blk = (blk + 1) // 2
    blk = (blk + group - 1) // group * group
    if ids is None and full is not None and blk < m:
        ids = torch.arange(full, dtype=torch.int32, device=device)
    return blk, ids


def blocks(m, blk):
    """(b, i0, i1): block b serves the requests i0 .. i1 - 1"""
    if 0 < m <= blk:     # the usual call: everything at once
        return [(0, 0, m)]
    return [(b, i0, min(m, i0 + blk)) for b, i0 in enumerate(range(0, m, blk))]


# --------------------------------------------------------------------------------------------------------- flags
def or_flags(words, device_bits=0):
    """The or of the calls' flag words.  Host words (a sequence, array or tensor, after the one read-back) -> int;
    device_bits = n: a device tensor of words with bits below 2^n -> their or as a device tensor [1], to go into the
    caller's one read-back."""
    if device_bits:
        bits = torch.tensor([1 << i for i in range(device_bits)], dtype=torch.int64, device=words.device)
        return (words.reshape(-1, 1) & bits).amax(dim=0).sum().reshape(1)
    out = 0
    for w in (words.tolist() if hasattr(words, "tolist") else words):
        out |= int(w)
    return out


def raise_flags(word, table, **fmt):
    """ValueError with the text of the first entry of `table` ((bit, text), ...) whose bit is set in `word`; the texts
    take their numbers from `fmt` by name"""
    for bit, text in table:
        if word & bit:
            raise ValueError(text % fmt)


# ------------------------------------------------------------------------------------------- the serving arguments
def user_lists(user_sims, nu, device):
    """user_sims: {u: {'indexes', 'values'}} as compute_userSimilarities returns it (users without an entry get an
    empty list).  -> (u_idx int32 (nu, max(ku, 1)) padded with -1, u_val float64 of the same shape padded with 0,
    ku = the longest list): the form the library takes user lists in.  A server prepares it once and passes the
    tuple wherever `user_sims` is taken.  Raises ValueError when a list is longer than 64."""
    ku = _longest_user_list(max((len(user_sims[u]["indexes"]) for u in user_sims), default=0))
    ui = np.full((nu, max(ku, 1)), -1, dtype=np.int32)
    uv = np.zeros((nu, max(ku, 1)), dtype=np.float64)
    for u in range(nu):
        if u in user_sims:
            n = len(user_sims[u]["indexes"])
            ui[u, :n] = user_sims[u]["indexes"]
            uv[u, :n] = user_sims[u]["values"]
    return torch.from_numpy(ui).to(device), torch.from_numpy(uv).to(device), ku


def _longest_user_list(ku, room=MAX_NEIGHBOURS):
    if not 0 <= int(ku) <= min(MAX_NEIGHBOURS, room):
        raise ValueError("a user has %d neighbours; the prediction kernel handles at most %d" % (ku, MAX_NEIGHBOURS))
    return ku


LIST_FLAGS = ((1, "a query has more than %(max)d neighbours (max_candidates overridden?); the prediction kernel "
                  "handles at most %(max)d"),
              (2, "a query's neighbour index is outside [0, %(nq)d)"))


class ServeInputs:
    """The checked arguments of predict_users / recommend.for_users, and (after upload()) their device form.
    Every check that needs no device runs in the constructor, before anything is uploaded or the library loaded.
    ids = "queries": `users` holds query ids instead (predict_queries / for_queries / query_utility): the same checks
    against nq, None = every column."""

    def __init__(self, ratings, q_src, q_dst, q_milli, user_sims, users, sum_order, ids="users"):
        self.sum_order = sum_order_code(sum_order)
        self.ratings = matrix(ratings, "ratings")
        self.nu, self.nq = (int(d) for d in self.ratings.shape)
        if self.nq >= 2**31:
            raise ValueError("at most 2^31 - 1 queries per row")
        self.what = "user" if ids == "users" else "query"
        self.bound = self.nu if ids == "users" else self.nq   # the ids lie in [0, bound)
        if ids != "users" and self.nu >= 2**31:
            raise ValueError("at most 2^31 - 1 users per column")
        self.coo = coo_triple(q_src, q_dst, q_milli)
        if isinstance(user_sims, tuple):
            u_idx, u_val, ku = user_sims
            if (u_idx.dim() != 2 or tuple(u_idx.shape) != tuple(u_val.shape) or u_idx.shape[0] != self.nu
                    or u_idx.dtype != torch.int32 or u_val.dtype != torch.float64):
                raise ValueError("prepared user lists must be user_lists(user_sims, %d, device)" % self.nu)
            _longest_user_list(ku, u_idx.shape[1])
        else:
            _longest_user_list(max((len(user_sims[u]["indexes"]) for u in user_sims), default=0))
        self.user_sims = user_sims
        self.m, self.users, self.device_ids = select_ids(users, self.bound, self.what, ids)

    def upload(self, device):
        self.r = on_device(self.ratings, device)
        self.q_off, self.q_idx, self.q_milli = lists_csr(self.coo, self.nq, device)
        us = self.user_sims
        u_idx, u_val, ku = us if isinstance(us, tuple) else user_lists(us, self.nu, device)
        self.u_idx, self.u_val = u_idx.to(device).contiguous(), u_val.to(device).contiguous()
        self.ku = self.u_idx.shape[1] if ku else 0
        self.ut = None if self.users is None else ids32(self.users, self.bound, device)
        return self

    def lists_args(self, query_weight, user_weight, default_mean):
        """the arguments both entry points share, up to `users`"""
        return (_ptr(self.r), self.nu, self.nq, _ptr(self.q_off), _ptr(self.q_idx), _ptr(self.q_milli),
                _ptr(self.u_idx), _ptr(self.u_val), self.ku, float(query_weight), float(user_weight),
                float(default_mean), self.sum_order)

    def raise_flags(self, flags):
        """flags: the library's flag words of the calls made, on the host or (one read-back) still on the device"""
        f = or_flags(flags.cpu() if isinstance(flags, torch.Tensor) else flags)
        if not f:
            return
        raise_flags(f, LIST_FLAGS, max=MAX_NEIGHBOURS, nq=self.nq)
        if f & 4:
            bad = torch.nonzero((self.ut < 0) | (self.ut >= self.bound))
            pos = int(bad[0, 0].item()) if bad.numel() else -1
            raise ValueError("%s id %s (position %d) outside [0, %d)"
                             % (self.what, int(self.users[pos].item()) if pos >= 0 else "?", pos, self.bound))
