"""Which blend serves the best LISTS?  evaluate_ranking(candidates="heldout")'s figures for a whole grid of settings
from one sweep of the device (qrlsh_evaluate_ranking_grid).

RMSE moves with the default-mean term of the blend, not with the order of the list; precision, recall and NDCG at k are
the figures for the order.  A setting is tune's: (query-list cut, user-list cut, weight triple).  The two sides of a test
cell do not depend on the weights and depend on the cuts only through a list prefix, so the device computes them once per
cut and keeps one record per test cell; per setting it blends, selects the k best test cells exactly (ties to the lowest
column) and scores them.  Every figure is an integer: the result is the one evaluate_ranking returns for that setting
over lists cut on the host, word for word.

evaluate_ranking_grid() returns a RankingGridEvaluation: the totals per setting, the figures derived from them on the
host, and best().  Cuts are reported here, never applied (Recommender.tune_ranking(apply_cuts=True) applies them)."""
import numpy as np
import torch

from . import _lib
from . import ops
from . import recommend
from . import tune
from ._inputs import ServeInputs, blocks, like_matrix, on_device, or_flags, request_blocks
from .ops import _ptr, _stream
from .ranking import check_arguments, _gain_tables

METRICS = ("ndcg", "precision", "recall", "hit_rate")   # best(): the highest


def _ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b != 0, a.astype(np.float64) / np.where(b != 0, b, 1).astype(np.float64), np.nan)


class RankingGridEvaluation:
    """The result of evaluate_ranking_grid().
    q_cuts, u_cuts: the lists of cuts; weights: float64 [W][3] = (query_weight, user_weight, default_mean).
    totals: host int64 [CQ][CU][W][16], RankingEvaluation.totals per setting -- words 0-7 the column sums of the
      per-request lines (listed, hits, known, first_hit, dcg, relevant, test, avail), 8 requests served, 9 requests with
      >= 1 relevant test cell, 10 requests with >= 1 hit, 11 the sum of the ideal DCG.
    per_request: device int64 [m][CQ][CU][W][8], the line of every request (want_per_request=True, else None).
    precision, recall, ndcg, hit_rate: float64 [CQ][CU][W] with RankingEvaluation's divisions (hits / listed, hits /
      relevant test cells, dcg / ideal dcg, requests with a hit / requests with a relevant test cell), nan on a zero
      denominator."""

    def __init__(self, q_cuts, u_cuts, weights, totals, per_request=None):
        self.q_cuts = [int(c) for c in q_cuts]
        self.u_cuts = [int(c) for c in u_cuts]
        self.weights = np.array(weights, dtype=np.float64).reshape(-1, 3)
        shape = (len(self.q_cuts), len(self.u_cuts), len(self.weights))
        self.totals = np.asarray(totals, dtype=np.int64).reshape(shape + (16,))
        self.per_request = per_request
        t = self.totals
        self.precision = _ratio(t[..., 1], t[..., 0])
        self.recall = _ratio(t[..., 1], t[..., 5])
        self.hit_rate = _ratio(t[..., 10], t[..., 9])
        self.ndcg = _ratio(t[..., 4], t[..., 11])

    def setting(self, index):
        """(q_cut, u_cut, (qw, uw, dm)) of setting `index` = (cq * CU + cu) * W + w"""
        cq, cu, w = np.unravel_index(int(index), self.ndcg.shape)
        return self.q_cuts[cq], self.u_cuts[cu], tuple(float(x) for x in self.weights[w])

    def best(self, metric="ndcg", min_recall=0.0):
        """The setting with the highest `metric` ('ndcg', 'precision', 'recall' or 'hit_rate') among those with recall >=
        min_recall; ties go to the lowest setting index; a setting without a figure (nan) never wins.
        -> (q_cut, u_cut, (query_weight, user_weight, default_mean), index).  ValueError when no setting qualifies."""
        if metric not in METRICS:
            raise ValueError("metric must be one of %s" % (METRICS,))
        value = getattr(self, metric).reshape(-1)
        ok = ~np.isnan(value)
        if float(min_recall) > 0.0:   # a recall of nan (no relevant test cell) passes only a bar of 0
            with np.errstate(invalid="ignore"):
                ok &= self.recall.reshape(-1) >= float(min_recall)
        if not ok.any():
            raise ValueError("no setting has a %s at recall >= %r" % (metric, min_recall))
        index = int(np.argmax(np.where(ok, value, -np.inf)))   # argmax: the first of equal values
        return self.setting(index) + (index,)

    def __repr__(self):
        return "RankingGridEvaluation(%d x %d cuts x %d weights)" % self.ndcg.shape


def _test_cells_per_request(a, truth, train_dev, truth_dev):
    """int64 host array [m]: the test cells (train == 0 and truth != 0) of every request's row -- the size of the
    record workspace.  Host matrices are counted on the host before the upload; device ones on the device, in row
    blocks, with one small read-back."""
    if not isinstance(a.ratings, torch.Tensor) and not isinstance(truth, torch.Tensor):
        rows = ((np.asarray(a.ratings) == 0) & (np.asarray(truth) != 0)).sum(axis=1).astype(np.int64)
        if a.users is None:
            return rows
        ids = a.ut.cpu().numpy().astype(np.int64) if a.device_ids else np.asarray(a.users, dtype=np.int64)
        inside = (ids >= 0) & (ids < a.nu)
        out = np.zeros(len(ids), dtype=np.int64)
        out[inside] = rows[ids[inside]]
        return out
    if a.nu == 0 or a.m == 0:
        return np.zeros(a.m, dtype=np.int64)
    # the rows of the requests only (a request list of 16 reads 16 rows), at most 2^26 cells at a time
    ids = None if a.ut is None else a.ut.to(torch.int64)
    step = max(1, (1 << 26) // max(a.nq, 1))
    parts = []
    for i in range(0, a.m, step):
        if ids is None:
            tr, tt = train_dev[i:i + step], truth_dev[i:i + step]
        else:
            sel = ids[i:i + step]
            inside = (sel >= 0) & (sel < a.nu)      # an id outside the matrix has no row: the library flags it
            sel = sel.clamp(0, a.nu - 1)
            tr, tt = train_dev[sel], truth_dev[sel]
        n = ((tr == 0) & (tt != 0)).sum(dim=1)
        parts.append(n if ids is None else n * inside)
    return torch.cat(parts).cpu().numpy().astype(np.int64)


def evaluate_ranking_grid(train, truth, q_src, q_dst, q_milli, user_sims, k, relevant, weights, q_cuts=None,
                          u_cuts=None, users=None, gains=None, sum_order="pairwise", want_per_request=False,
                          device="cuda"):
    """evaluate_ranking(candidates="heldout")'s totals under every setting of a grid (qrlsh_evaluate_ranking_grid).
    train / truth, the lists, user_sims, k, relevant, users, gains and sum_order: as evaluate_ranking takes them.
    weights: (W, 3) rows (query_weight, user_weight, default_mean).  q_cuts / u_cuts: 1 to 4 list lengths >= 0 each
    (default [64], the whole lists); a cut keeps the first min(len, cut) entries of a list as stored, 0 switches the
    side off.  More than 128 settings run as successive calls along the weights and are stitched together; requests run
    in blocks under recommend.WORKSPACE_BUDGET and the blocks' totals are added on the device.
    -> RankingGridEvaluation (one read-back of results: the totals and the flags; sizing the record workspace reads the
    number of test cells per request first when the matrices are already on the device).
    ValueError, before anything is uploaded, for a bad k, relevant, gains, sum_order, cuts or weights, a truth of another
    shape and a host user id outside the matrix; through the library's flags for a list longer than 64, a neighbour index
    outside [0, nq) and a device user id outside [0, nu)."""
    k = check_arguments(k, relevant, "heldout")
    qc, uc, w = tune._cuts(q_cuts, "q_cuts"), tune._cuts(u_cuts, "u_cuts"), tune._weights(weights)
    a = ServeInputs(train, q_src, q_dst, q_milli, user_sims, users, sum_order)
    truth = like_matrix(truth, "truth", (a.nu, a.nq), "train")
    m, nq = a.m, a.nq
    gain, prefix = _gain_tables(gains, k, m)
    ncq, ncu = len(qc), len(uc)
    tune.chunks_of(len(w), ncq, ncu)

    lib = _lib.load()
    a.upload(device)
    dev = a.r.device
    t = on_device(truth, device)
    if m == 0:
        per = torch.empty((0, ncq, ncu, len(w), 8), dtype=torch.int64, device=dev) if want_per_request else None
        return RankingGridEvaluation(qc, uc, w, np.zeros((ncq, ncu, len(w), 16), dtype=np.int64), per)
    gain_d, prefix_d = torch.from_numpy(gain).to(dev), torch.from_numpy(prefix).to(dev)
    d_qc = torch.tensor(qc, dtype=torch.int32, device=dev)
    d_uc = torch.tensor(uc, dtype=torch.int32, device=dev)
    d_w = torch.from_numpy(w).to(dev)
    cells = _test_cells_per_request(a, truth, a.r, t)
    size = lib.qrlsh_evaluate_ranking_grid_workspace_bytes
    widest = min(tune.MAX_SETTINGS // (ncq * ncu), len(w)) * ncq * ncu   # the settings of the largest call

    def need(blk):
        return max(int(size(i1 - i0, nq, ncq, ncu, widest, int(cells[i0:i1].sum()))) for _, i0, i1 in blocks(m, blk))

    blk, ut = request_blocks(m, need, recommend.WORKSPACE_BUDGET, ids=a.ut, full=a.nu, device=dev)
    ws = ops._ws(need(blk), dev)
    st = _stream()

    def launch(lo, hi):
        nw = hi - lo
        s = ncq * ncu * nw
        per = torch.empty((m, ncq, ncu, nw, 8), dtype=torch.int64, device=dev) if want_per_request else None
        parts = blocks(m, blk)
        back = torch.zeros((len(parts), s * 16 + 1), dtype=torch.int64, device=dev)   # per block [totals][flags]
        for b, i0, i1 in parts:
            _lib.check(lib.qrlsh_evaluate_ranking_grid(
                _ptr(a.r), _ptr(t), a.nu, nq, _ptr(a.q_off), _ptr(a.q_idx), _ptr(a.q_milli), _ptr(a.u_idx),
                _ptr(a.u_val), a.ku, _ptr(d_qc), ncq, _ptr(d_uc), ncu, _ptr(d_w[lo:hi]), nw, a.sum_order,
                None if ut is None else _ptr(ut[i0:i1]), i1 - i0, k, int(relevant), _ptr(gain_d), _ptr(prefix_d),
                int(cells[i0:i1].sum()), None if per is None else _ptr(per[i0:i1]), _ptr(back[b]), None,
                _ptr(back[b, s * 16:]), _ptr(ws), ws.numel(), st))
        return back[:, :s * 16].sum(dim=0).view(ncq, ncu, nw, 16), per, or_flags(back[:, s * 16:], device_bits=5)

    totals, per, flags = tune.sweep(len(w), ncq, ncu, launch)
    host = torch.cat([totals.reshape(-1), flags]).cpu().numpy()     # the one read-back
    n = totals.numel()
    f = or_flags(host[n:])
    if f & 16:
        raise RuntimeError("the matrices changed while they were evaluated: more test cells than were counted")
    if f & 8:
        raise ValueError("gains and cuts must not be negative")
    a.raise_flags(host[n:] & 7)
    return RankingGridEvaluation(qc, uc, w, host[:n], per_request=per)
