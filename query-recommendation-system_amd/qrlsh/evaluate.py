"""How good is the served model?  The prediction error on rated cells, on the device.

The blend of cell (i, j) (recommender.py:313-331) never reads ratings[i][j], so a rated cell can be predicted as if it
were unrated and compared with its rating.  evaluate() does that for a seeded sample of the rated cells
(qrlsh_evaluate), evaluate_cells() for an explicit test set (qrlsh_evaluate_cells), and holdout() makes the train
matrix of a hold-out split with the same sample rule (qrlsh_ratings_holdout).  Predictions and ratings are integers:
every statistic is an exact integer sum.

LEAVE-ONE-OUT HOLDS THE LISTS FIXED.  evaluate(ratings, ...) with truth=None predicts each rated cell without its own
rating, but from user similarities that were computed with the cell present; that leak flatters the user side.  The
protocol without it is the hold-out: train, n = holdout(truth, fraction, seed); user similarities over `train`;
evaluate(train, ..., truth=truth, fraction=fraction, seed=seed)."""
import math

import numpy as np
import torch

from . import _lib
from . import ops
from ._inputs import ServeInputs, ids32, int_array, like_matrix, matrix, on_device
from .ops import _ptr, _stream
from .predict import DEFAULT_MEAN, QUERY_WEIGHT, USER_WEIGHT

BRANCHES = (("query", 0), ("user", 4), ("both", 8))   # the three non-zero branches of the blend -> first word


def mix64(x):
    """qr_mix64 of csrc/common.h (the splitmix64 finaliser) on a Python integer"""
    m = (1 << 64) - 1
    z = x & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def keep_word(fraction):
    """the sample rule's `keep` of a fraction in [0, 1]: round(fraction * 2^32)"""
    if isinstance(fraction, bool) or not isinstance(fraction, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(fraction) <= 1.0:      # (nan fails the comparison)
        raise ValueError("fraction must be a number in [0, 1], got %r" % (fraction,))
    return int(round(float(fraction) * 2.0**32))


def is_kept(seed, keep, i, j):
    """the sample rule: cell (i, j) is kept iff mix64(seed ^ (i << 32 | j)) >> 32 < keep"""
    return (mix64(int(seed) ^ (int(i) << 32 | (int(j) & 0xFFFFFFFF))) >> 32) < keep


def _seed_word(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2**64:
        raise ValueError("seed must be an integer in [0, 2^64), got %r" % (seed,))
    return int(seed)


def _figures(n, se, sa, ss):
    n, se, sa, ss = int(n), int(se), int(sa), int(ss)
    if n == 0:
        return {"n": 0, "mae": math.nan, "rmse": math.nan, "bias": math.nan}
    return {"n": n, "mae": sa / n, "rmse": math.sqrt(ss / n), "bias": se / n}


class Evaluation:
    """The result of evaluate() / evaluate_cells().
    totals: host int64 [16] -- words 0-3, 4-7, 8-11 = n, sum err, sum |err|, sum err^2 (err = prediction - rating) of the
      cells predicted from the query side only, the user side only and both; word 12 = evaluated cells without a
      prediction (missed: in no sum); word 13 = evaluated cells.
    per_user: device int64 [nu][16], the same line per user (evaluate only, else None).
    predictions: device int32, evaluate(want_predictions=True): [nu][nq], the prediction at evaluated cells (0 = missed)
      and -1 elsewhere; evaluate_cells: [m], one per triplet.  None unless asked for.
    n = evaluated cells, covered = those with a prediction, coverage = covered / n; mae, rmse, bias: Python floats from
    the integer sums over the covered cells (nan when nothing is covered); by_branch: {'query' / 'user' / 'both': {'n',
    'mae', 'rmse', 'bias'}}."""

    def __init__(self, totals, per_user=None, predictions=None):
        self.totals = np.asarray(totals, dtype=np.int64).reshape(16)
        self.per_user = per_user
        self.predictions = predictions
        t = [int(x) for x in self.totals]
        self.n = t[13]
        self.covered = t[13] - t[12]
        self.coverage = self.covered / self.n if self.n else math.nan
        self.by_branch = {name: _figures(*t[o:o + 4]) for name, o in BRANCHES}
        whole = _figures(*(sum(t[o + w] for _, o in BRANCHES) for w in range(4)))
        self.mae, self.rmse, self.bias = whole["mae"], whole["rmse"], whole["bias"]

    def __repr__(self):
        return "Evaluation(n=%d, covered=%d, mae=%.4f, rmse=%.4f, bias=%+.4f)" % (self.n, self.covered, self.mae,
                                                                                    self.rmse, self.bias)


def holdout(ratings, fraction, seed=0, device="cuda"):
    """The train matrix of a hold-out split: `ratings` ((nu, nq) integers, a tensor or host data) with the kept rated
    cells set to 0 -- about `fraction` of them, chosen by the sample rule (is_kept) under `seed`.  Out of place: the
    input is not modified.  -> (int32 device tensor (nu, nq), the number of cells held out).
    ValueError for a fraction outside [0, 1]."""
    keep, seed = keep_word(fraction), _seed_word(seed)
    a = matrix(ratings, "ratings")
    nu, nq = (int(d) for d in a.shape)
    if nu >= 2**31 or nq >= 2**31:
        raise ValueError("at most 2^31 - 1 rows and columns")
    lib = _lib.load()
    r = on_device(a, device)
    out = torch.empty_like(r)
    count = torch.zeros((1,), dtype=torch.int64, device=r.device)
    _lib.check(lib.qrlsh_ratings_holdout(_ptr(r), nu, nq, seed, keep, _ptr(out), _ptr(count), _stream()))
    return out, int(count.item())


def evaluate(ratings, q_src, q_dst, q_milli, user_sims, truth=None, fraction=1.0, seed=0, sum_order="pairwise",
             want_predictions=False, query_weight=QUERY_WEIGHT, user_weight=USER_WEIGHT, default_mean=DEFAULT_MEAN,
             device="cuda"):
    """The prediction error over the kept cells that `truth` rates (qrlsh_evaluate): each is predicted from `ratings`
    exactly as if ratings[i][j] were 0, from the lists as predict_users takes them (q_src / q_dst / q_milli: COO sorted
    by source; user_sims: compute_userSimilarities' dict or user_lists' tuple).
    truth=None: truth = ratings, leave-one-out WITH THE LISTS HELD FIXED (see the module text).  truth=the full matrix
    and ratings=holdout(truth, fraction, seed)[0] with the same fraction and seed: the cells held out.
    fraction / seed: the sample (is_kept); fraction 1 keeps every rated cell.
    -> Evaluation (per_user on the device; one read-back: the totals and the flags).
    ValueError for a fraction outside [0, 1], a truth of another shape, a bad sum_order, a list longer than 64 and a
    neighbour index outside [0, nq)."""
    keep, seed = keep_word(fraction), _seed_word(seed)
    a = ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, None, sum_order)
    if truth is not None:
        truth = like_matrix(truth, "truth", (a.nu, a.nq), "ratings")
    if a.nu >= 2**31:
        raise ValueError("at most 2^31 - 1 users")
    lib = _lib.load()
    a.upload(device)
    t = a.r if truth is None else on_device(truth, device)
    dev = a.r.device
    per_user = torch.empty((a.nu, 16), dtype=torch.int64, device=dev)
    back = torch.zeros((17,), dtype=torch.int64, device=dev)    # [totals: 16][flags: the low half of word 16]
    pred = torch.empty((a.nu, a.nq), dtype=torch.int32, device=dev) if want_predictions else None
    ws = ops._ws(lib.qrlsh_evaluate_workspace_bytes(a.nu, a.nq), dev)
    _lib.check(lib.qrlsh_evaluate(_ptr(a.r), _ptr(t), a.nu, a.nq, _ptr(a.q_off), _ptr(a.q_idx), _ptr(a.q_milli),
                                  _ptr(a.u_idx), _ptr(a.u_val), a.ku, float(query_weight), float(user_weight),
                                  float(default_mean), a.sum_order, seed, keep, _ptr(per_user), _ptr(back), _ptr(pred),
                                  _ptr(back[16:]), _ptr(ws), ws.numel(), _stream()))
    host = back.cpu().numpy()
    a.raise_flags(host[16:])
    return Evaluation(host[:16], per_user=per_user, predictions=pred)


def evaluate_cells(ratings, q_src, q_dst, q_milli, user_sims, users, queries, values, sum_order="pairwise",
                   want_predictions=False, query_weight=QUERY_WEIGHT, user_weight=USER_WEIGHT,
                   default_mean=DEFAULT_MEAN, device="cuda"):
    """The prediction error on an explicit test set (qrlsh_evaluate_cells): triplets (users[c], queries[c], values[c]),
    host sequences or device tensors of one length; every triplet is evaluated -- repeats once each -- as if
    ratings[user][query] were 0, whatever `ratings` holds there.  Other arguments as evaluate takes them.
    -> Evaluation without per_user; predictions (want_predictions=True): int32 [m], one per triplet.
    ValueError as evaluate raises it, and for a user or query id outside the matrix (host ids before anything is
    uploaded; device ids through the library's flag)."""
    a = ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, users if users is not None else [], sum_order)
    cols = [int_array(queries, 1, "queries"), int_array(values, 1, "values")]
    if not cols[0].numel() == cols[1].numel() == a.m:
        raise ValueError("users, queries and values differ in length")
    if not cols[0].is_cuda and cols[0].numel() and (int(cols[0].min()) < 0 or int(cols[0].max()) >= a.nq):
        raise ValueError("query id outside [0, %d)" % a.nq)
    if a.nu >= 2**31:
        raise ValueError("at most 2^31 - 1 users")
    lib = _lib.load()
    a.upload(device)
    dev = a.r.device
    cq = ids32(cols[0], a.nq, dev)
    cv = cols[1].to(device=dev, dtype=torch.int32).contiguous()
    back = torch.zeros((17,), dtype=torch.int64, device=dev)
    pred = torch.empty((a.m,), dtype=torch.int32, device=dev) if want_predictions else None
    _lib.check(lib.qrlsh_evaluate_cells(_ptr(a.r), a.nu, a.nq, _ptr(a.q_off), _ptr(a.q_idx), _ptr(a.q_milli),
                                        _ptr(a.u_idx), _ptr(a.u_val), a.ku, float(query_weight), float(user_weight),
                                        float(default_mean), a.sum_order, _ptr(a.ut), _ptr(cq), _ptr(cv), a.m,
                                        _ptr(pred), _ptr(back), _ptr(back[16:]), _stream()))
    host = back.cpu().numpy()
    if int(host[16]) & 4 and a.m and bool(((cq < 0) | (cq >= a.nq)).any().item()):
        raise ValueError("query id outside [0, %d)" % a.nq)
    a.raise_flags(host[16:])
    return Evaluation(host[:16], predictions=pred)
