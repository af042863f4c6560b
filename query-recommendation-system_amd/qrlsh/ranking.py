"""Is what the user would have liked in the list the user is shown?  Precision, recall and NDCG at k of the served lists
against held-out cells, on the device (qrlsh_evaluate_ranking).

Hold-out only: `train` is the matrix with the test cells zeroed (qrlsh.holdout), `truth` the full matrix.  A test cell of
user u is one with train[u][j] == 0 and truth[u][j] != 0; it is relevant when truth[u][j] >= relevant.  The list of a
user is for_users(train, ...)'s -- a test cell is unrated in `train`, so the serving arithmetic is its hold-out
prediction -- and the sweep, the selection and the score never leave the device: no (nu, nq) prediction matrix.  Every
count is an integer and DCG is an integer sum of the caller's gains, so the totals are exact in any launch order."""
import math

import numpy as np
import torch

from . import _lib
from . import ops
from . import recommend
from ._args import _int_in
from ._inputs import ServeInputs, blocks, like_matrix, on_device, or_flags, request_blocks
from .ops import _ptr, _stream
from .predict import DEFAULT_MEAN, QUERY_WEIGHT, USER_WEIGHT

CANDIDATES = {"all": _lib.RANK_ALL, "heldout": _lib.RANK_HELDOUT}
WORDS = ("listed", "hits", "known", "first_hit", "dcg", "relevant", "test", "avail")   # a line of per_user


def dcg_gains(k):
    """the default DCG gain table: int64 [k], gain of list position p (0-based) = round(2^32 / log2(p + 2)); gains[0] =
    2^32, decreasing"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError("k must be a positive integer, got %r" % (k,))
    return np.array([round(2.0**32 / math.log2(p + 2)) for p in range(int(k))], dtype=np.int64)


def _ratio(a, b):
    return int(a) / int(b) if int(b) else math.nan


class RankingEvaluation:
    """The result of evaluate_ranking().
    idx, val int32 (m, k), avail int32 (m,): the served lists (device), as for_users returns them.
    per_user: device int64 (m, 8), one line per request -- listed = min(k, avail), hits (listed cells that are relevant),
      known (listed cells the truth rates), the 1-based rank of the first hit (0 = none), dcg (sum of the gains at the hit
      positions), relevant test cells, test cells (both include cells without a prediction), avail.
    totals: host int64 [16] -- words 0-7 the column sums of per_user, 8 requests served, 9 requests with >= 1 relevant
      test cell, 10 requests with >= 1 hit, 11 the sum of the ideal DCG (the first min(k, relevant test cells) gains).
    Micro figures, Python floats from the integers (nan on a zero denominator): precision = hits / listed, recall = hits /
    relevant test cells, hit_rate = requests with a hit / requests with a relevant test cell, ndcg = dcg / ideal dcg,
    known_share = known / listed."""

    def __init__(self, totals, idx=None, val=None, avail=None, per_user=None, gain_prefix=None):
        self.totals = np.asarray(totals, dtype=np.int64).reshape(16)
        self.idx, self.val, self.avail, self.per_user = idx, val, avail, per_user
        self._gain_prefix = gain_prefix
        t = [int(x) for x in self.totals]
        self.requests = t[8]
        self.precision = _ratio(t[1], t[0])
        self.recall = _ratio(t[1], t[5])
        self.hit_rate = _ratio(t[10], t[9])
        self.ndcg = _ratio(t[4], t[11])
        self.known_share = _ratio(t[2], t[0])

    def macro(self):
        """{'n', 'precision', 'recall', 'ndcg', 'mrr'}: the means over the n requests with >= 1 relevant test cell of the
        per-request precision (hits / listed; 0 for an empty list), recall, NDCG and reciprocal rank of the first hit (0
        without one), nan when n = 0.  Computed from per_user in float64 (torch): floating point, not exact, unlike the
        micro figures."""
        p = self.per_user.to(torch.float64)
        listed, hits, first, dcg, rel = p[:, 0], p[:, 1], p[:, 3], p[:, 4], p[:, 5]
        on = rel > 0
        n = int(on.sum().item())
        if n == 0:
            return {"n": 0, "precision": math.nan, "recall": math.nan, "ndcg": math.nan, "mrr": math.nan}
        one = torch.ones_like(rel)
        k = self._gain_prefix.numel() - 1
        ideal = self._gain_prefix.to(p.device)[self.per_user[:, 5].clamp(0, k)].to(torch.float64)
        lines = torch.stack([torch.where(listed > 0, hits / torch.maximum(listed, one), 0 * one),
                             hits / torch.maximum(rel, one),
                             torch.where(ideal > 0, dcg / torch.maximum(ideal, one), 0 * one),
                             torch.where(first > 0, 1.0 / torch.maximum(first, one), 0 * one)])
        mean = (lines[:, on].sum(dim=1) / n).cpu().tolist()
        return {"n": n, "precision": mean[0], "recall": mean[1], "ndcg": mean[2], "mrr": mean[3]}

    def __repr__(self):
        return "RankingEvaluation(requests=%d, precision=%.4f, recall=%.4f, ndcg=%.4f, hit_rate=%.4f)" % (
            self.requests, self.precision, self.recall, self.ndcg, self.hit_rate)


def check_arguments(k, relevant, candidates="all", lo=0, slices=0):
    """ValueError for a bad k, relevant, candidates, lo or slices (no device, no library) -> int(k)"""
    k = _int_in(k, "k", 1, recommend.MAX_K)
    if isinstance(relevant, bool) or not isinstance(relevant, (int, np.integer)) or not 1 <= int(relevant) < 2**31:
        raise ValueError("relevant must be an int32 >= 1, got %r" % (relevant,))
    if not isinstance(candidates, str) or candidates not in CANDIDATES:
        raise ValueError("candidates must be 'all' or 'heldout', got %r" % (candidates,))
    _int_in(slices, "slices", 0, recommend.MAX_SLICES)
    if isinstance(lo, bool) or not isinstance(lo, (int, np.integer)) or not -2**31 <= int(lo) < 2**31:
        raise ValueError("lo must be an int32, got %r" % (lo,))
    return k


def _gain_tables(gains, k, m):
    """(gain int64 [k], gain_prefix int64 [k + 1]) host arrays of a checked table"""
    if gains is None:
        g = [int(x) for x in dcg_gains(k)]
    else:
        a = np.asarray(gains.cpu() if isinstance(gains, torch.Tensor) else gains)
        if a.ndim != 1 or a.size != k or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("gains must be %d integers (one per list position)" % k)
        g = [int(x) for x in a.tolist()]
        if min(g) < 0:
            raise ValueError("gains must not be negative")
    prefix = [0]
    for x in g:
        prefix.append(prefix[-1] + x)
    if max(m, 1) * prefix[k] >= 2**63:
        raise ValueError("%d requests x a DCG of up to %d do not fit int64: use smaller gains" % (m, prefix[k]))
    return np.array(g, dtype=np.int64), np.array(prefix, dtype=np.int64)


def evaluate_ranking(train, truth, q_src, q_dst, q_milli, user_sims, k, relevant, users=None, candidates="all",
                     gains=None, lo=0, slices=0, sum_order="pairwise", query_weight=QUERY_WEIGHT,
                     user_weight=USER_WEIGHT, default_mean=DEFAULT_MEAN, device="cuda"):
    """Score the lists for_users(train, ..., users, k) would serve against `truth` (qrlsh_evaluate_ranking).
    train / truth: (nu, nq) integers of one shape, train = truth with the test cells zeroed (qrlsh.holdout); the lists,
    user_sims, users, k, lo, slices and sum_order as for_users takes them (users=None: every user).
    relevant: a test cell counts as relevant when truth >= relevant (an int32 >= 1).
    candidates: "all" ranks every unrated cell of train (the list the user would be shown; cells the truth does not rate
    count as not relevant); "heldout" ranks the test cells only.
    gains: k non-negative integers, the DCG gain per list position (default dcg_gains(k)).
    Served in request blocks under recommend.WORKSPACE_BUDGET; the blocks' totals are added on the device.
    -> RankingEvaluation (lists and per_user on the device; one read-back: the totals and the flags).
    ValueError, for host data before anything is uploaded, for a bad k, relevant, candidates, gains (wrong length,
    negative, or m x their sum >= 2^63), lo, slices or sum_order, a truth of another shape and a user id outside the
    matrix; through the library's flags for a list longer than 64, a neighbour index outside [0, nq) and a device user
    id outside [0, nu)."""
    k = check_arguments(k, relevant, candidates, lo, slices)
    a = ServeInputs(train, q_src, q_dst, q_milli, user_sims, users, sum_order)
    truth = like_matrix(truth, "truth", (a.nu, a.nq), "train")
    gain, prefix = _gain_tables(gains, k, a.m)
    _lib.load()
    a.upload(device)
    return _score(a, on_device(truth, device), k, relevant, candidates, gain, prefix, lo, slices,
                  (query_weight, user_weight, default_mean))


def _score(a, t, k, relevant, candidates, gain, prefix, lo, slices, weights):
    """evaluate_ranking over uploaded ServeInputs `a`, the device truth `t` and checked gain tables (host arrays);
    weights = (query_weight, user_weight, default_mean)"""
    lib = _lib.load()
    m, nq = a.m, a.nq
    dev = a.r.device
    gain_d, prefix_d = torch.from_numpy(gain).to(dev), torch.from_numpy(prefix).to(dev)
    idx = torch.empty((m, k), dtype=torch.int32, device=dev)
    val = torch.empty((m, k), dtype=torch.int32, device=dev)
    avail = torch.empty((m,), dtype=torch.int32, device=dev)
    per_user = torch.empty((m, 8), dtype=torch.int64, device=dev)
    if m == 0:
        return RankingEvaluation(np.zeros(16, dtype=np.int64), idx, val, avail, per_user, prefix_d)
    def need(blk):
        return int(lib.qrlsh_evaluate_ranking_workspace_bytes(blk, nq, k, int(slices)))
    blk, ut = request_blocks(m, need, recommend.WORKSPACE_BUDGET, ids=a.ut, full=a.nu, device=dev)
    ws = ops._ws(need(blk), dev)
    parts = blocks(m, blk)
    back = torch.zeros((len(parts), 17), dtype=torch.int64, device=dev)   # per block [totals: 16][flags: low half]
    args = a.lists_args(*weights)
    st = _stream()
    for b, i0, i1 in parts:
        _lib.check(lib.qrlsh_evaluate_ranking(args[0], _ptr(t), *args[1:], None if ut is None else _ptr(ut[i0:i1]),
                                              i1 - i0, k, int(relevant), CANDIDATES[candidates], int(lo), int(slices),
                                              _ptr(gain_d), _ptr(prefix_d), _ptr(idx[i0:i1]), _ptr(val[i0:i1]),
                                              _ptr(avail[i0:i1]), _ptr(per_user[i0:i1]), _ptr(back[b]),
                                              _ptr(back[b, 16:]), _ptr(ws), ws.numel(), st))
    flag = or_flags(back[:, 16:], device_bits=4)
    host = torch.cat([back[:, :16].sum(dim=0), flag]).cpu().numpy()     # the one read-back
    if int(host[16]) & 8:
        raise ValueError("gains must not be negative")
    a.raise_flags(host[16:] & 7)
    return RankingEvaluation(host[:16], idx, val, avail, per_user, prefix_d)
