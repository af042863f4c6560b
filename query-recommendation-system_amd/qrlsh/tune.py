"""Which blend serves best?  evaluate()'s figures for a whole grid of settings from one sweep of the device.

A setting is (query-list cut, user-list cut, weight triple).  Two facts make one sweep exact for all of them
(qrlsh_evaluate_grid): the two sides of a cell do not depend on the weights, and every stored list is ordered score
descending with ties by id ascending, so its first c entries are the list a run with K = c would have stored.  A cut of 0
switches a side off (the ablation), a cut at or past the length is the whole list.

evaluate_grid() takes evaluate()'s arguments and the grid, and returns a GridEvaluation: the exact integer sums per
setting, the figures derived from them on the host after one read-back, and best().  Cuts are reported here, never applied:
applying one is QueryIndex.set_list_length / UserLists.set_list_length (Recommender.tune(apply_cuts=True))."""
import numpy as np
import torch

from . import _lib
from . import ops
from ._inputs import ServeInputs, like_matrix, on_device, or_flags
from .evaluate import keep_word, _seed_word
from .ops import _ptr, _stream

MAX_CUTS = 4          # QRLSH_GRID_MAX_CUTS
MAX_SETTINGS = 128    # QRLSH_GRID_MAX_SETTINGS
WHOLE = 64            # the default cut: no stored list is longer
METRICS = ("rmse", "mae", "bias")   # best(): the lowest rmse, mae or |bias|


def _cuts(cuts, name):
    if cuts is None:
        return [WHOLE]
    try:
        seq = list(cuts)
    except TypeError:
        raise ValueError("%s must be a sequence of integers >= 0" % name) from None
    if not 1 <= len(seq) <= MAX_CUTS:
        raise ValueError("%s needs 1 to %d cuts, got %d" % (name, MAX_CUTS, len(seq)))
    for c in seq:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0:
            raise ValueError("%s must hold integers >= 0, got %r" % (name, c))
    return [min(int(c), 2**31 - 1) for c in seq]


def _weights(weights):
    w = np.array(weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != 3 or w.shape[0] < 1 or not np.isfinite(w).all():
        raise ValueError("weights must be (W, 3) finite numbers (query_weight, user_weight, default_mean), W >= 1")
    return w


def chunks_of(nw, ncq, ncu, limit=MAX_SETTINGS):
    """the runs [lo, hi) of weight triples that fit one library call each: ncq * ncu * (hi - lo) <= limit"""
    step = limit // (ncq * ncu)
    if step < 1:
        raise ValueError("%d x %d cuts exceed the %d settings of a call" % (ncq, ncu, limit))
    return [(lo, min(nw, lo + step)) for lo in range(0, nw, step)]


def sweep(nw, ncq, ncu, launch, limit=MAX_SETTINGS):
    """Run launch(lo, hi) for every run of chunks_of() and stitch the results along the weights.
    launch -> (totals int64 tensor [ncq][ncu][hi - lo][8], per_user int64 tensor [nu][ncq][ncu][hi - lo][8] or None,
    flags int64 tensor [1]), all on one device.
    -> (totals [ncq][ncu][nw][8], per_user or None, flags [calls]) on that device: nothing is read back here."""
    parts = [launch(lo, hi) for lo, hi in chunks_of(nw, ncq, ncu, limit)]
    totals = torch.cat([p[0] for p in parts], dim=2) if len(parts) > 1 else parts[0][0]
    per_user = None
    if parts[0][1] is not None:
        per_user = torch.cat([p[1] for p in parts], dim=3) if len(parts) > 1 else parts[0][1]
    return totals, per_user, torch.cat([p[2].reshape(1) for p in parts])


class GridEvaluation:
    """The result of evaluate_grid().
    q_cuts, u_cuts: the lists of cuts; weights: float64 [W][3] = (query_weight, user_weight, default_mean).
    totals: host int64 [CQ][CU][W][8] -- word 0 = n (cells with a non-zero prediction), 1 = sum err, 2 = sum |err|,
      3 = sum err^2 (err = prediction - rating), 4 = missed (prediction 0), 5 = cells evaluated, 6 / 7 = n predicted from
      the query side only / the user side only.
    per_user: device int64 [nu][CQ][CU][W][8], the same line per user (want_per_user=True, else None).
    n, mae, rmse, bias, coverage: float64 [CQ][CU][W] from the integers (mae, rmse, bias: nan where n == 0; coverage =
      n / cells evaluated, nan where nothing was evaluated)."""

    def __init__(self, q_cuts, u_cuts, weights, totals, per_user=None):
        self.q_cuts = [int(c) for c in q_cuts]
        self.u_cuts = [int(c) for c in u_cuts]
        self.weights = np.array(weights, dtype=np.float64).reshape(-1, 3)
        shape = (len(self.q_cuts), len(self.u_cuts), len(self.weights))
        self.totals = np.asarray(totals, dtype=np.int64).reshape(shape + (8,))
        self.per_user = per_user
        t = self.totals.astype(np.float64)
        n, cells = t[..., 0], t[..., 5]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.n = n.copy()
            self.mae = np.where(n > 0, t[..., 2] / n, np.nan)
            self.rmse = np.where(n > 0, np.sqrt(t[..., 3] / n), np.nan)
            self.bias = np.where(n > 0, t[..., 1] / n, np.nan)
            self.coverage = np.where(cells > 0, n / cells, np.nan)

    def setting(self, index):
        """(q_cut, u_cut, (qw, uw, dm)) of setting `index` = (cq * CU + cu) * W + w"""
        cq, cu, w = np.unravel_index(int(index), self.n.shape)
        return self.q_cuts[cq], self.u_cuts[cu], tuple(float(x) for x in self.weights[w])

    def best(self, metric="rmse", min_coverage=0.0):
        """The setting with the lowest `metric` ('rmse', 'mae', or 'bias' = the lowest |bias|) among those with
        coverage >= min_coverage; ties go to the lowest setting index; a setting without a figure (nan) never wins.
        -> (q_cut, u_cut, (query_weight, user_weight, default_mean), index).  ValueError when no setting qualifies."""
        if metric not in METRICS:
            raise ValueError("metric must be one of %s" % (METRICS,))
        value = np.abs(self.bias) if metric == "bias" else getattr(self, metric)
        value = value.reshape(-1)
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(value) & (self.coverage.reshape(-1) >= float(min_coverage))
        if not ok.any():
            raise ValueError("no setting has a %s at coverage >= %r" % (metric, min_coverage))
        index = int(np.argmin(np.where(ok, value, np.inf)))   # argmin: the first of equal values
        return self.setting(index) + (index,)

    def __repr__(self):
        return "GridEvaluation(%d x %d cuts x %d weights)" % self.n.shape


def evaluate_grid(ratings, q_src, q_dst, q_milli, user_sims, weights, q_cuts=None, u_cuts=None, truth=None,
                  fraction=1.0, seed=0, sum_order="pairwise", want_per_user=False, device="cuda"):
    """evaluate()'s cells under every setting of a grid, in one sweep per 128 settings (qrlsh_evaluate_grid).
    ratings, q_src / q_dst / q_milli, user_sims, truth, fraction, seed, sum_order: as evaluate() takes them.
    weights: (W, 3) rows (query_weight, user_weight, default_mean).  q_cuts / u_cuts: 1 to 4 list lengths >= 0 each
    (default [64], the whole lists); a cut keeps the first min(len, cut) entries of a list as stored, 0 switches the
    side off.  More than 128 settings run as successive calls along the weights and are stitched together.
    -> GridEvaluation (one read-back: the totals and the flags).
    ValueError for empty or negative cuts or more than 4 per side, weights of another shape, a fraction outside [0, 1],
    a bad sum_order, a truth of another shape, and the lists' flags as evaluate() raises them."""
    qc, uc, w = _cuts(q_cuts, "q_cuts"), _cuts(u_cuts, "u_cuts"), _weights(weights)
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
    ncq, ncu = len(qc), len(uc)
    d_qc = torch.tensor(qc, dtype=torch.int32, device=dev)
    d_uc = torch.tensor(uc, dtype=torch.int32, device=dev)
    d_w = torch.from_numpy(w).to(dev)

    def launch(lo, hi):
        nw = hi - lo
        s = ncq * ncu * nw
        per_user = torch.empty((a.nu, ncq, ncu, nw, 8), dtype=torch.int64, device=dev) if want_per_user else None
        back = torch.zeros((s * 8 + 1,), dtype=torch.int64, device=dev)   # [totals][flags: the low half of a word]
        ws = ops._ws(lib.qrlsh_evaluate_grid_workspace_bytes(a.nu, a.nq, s), dev)
        _lib.check(lib.qrlsh_evaluate_grid(_ptr(a.r), _ptr(t), a.nu, a.nq, _ptr(a.q_off), _ptr(a.q_idx),
                                           _ptr(a.q_milli), _ptr(a.u_idx), _ptr(a.u_val), a.ku, _ptr(d_qc), ncq,
                                           _ptr(d_uc), ncu, _ptr(d_w[lo:hi]), nw, a.sum_order, seed, keep,
                                           _ptr(per_user), _ptr(back), _ptr(back[s * 8:]), _ptr(ws), ws.numel(),
                                           _stream()))
        return back[:s * 8].view(ncq, ncu, nw, 8), per_user, back[s * 8:]

    totals, per_user, flags = sweep(len(w), ncq, ncu, launch)
    host = torch.cat([totals.reshape(-1), flags]).cpu().numpy()
    n = totals.numel()
    if or_flags(host[n:]) & 8:
        raise ValueError("a cut is negative")   # (checked above: the library's own check)
    a.raise_flags(host[n:] & 7)
    return GridEvaluation(qc, uc, w, host[:n], per_user=per_user)
