"""Diversified recommendations: rerank served pools by the stored neighbour lists, and the redundancy of any served
list (qrlsh_diversify, qrlsh_list_redundancy).  The project's own rule; the reference has no counterpart.

sim(a, b) = the largest stored milli value among the list entries a -> b and b -> a, 0 when neither is stored (the
lists are top-K cuts: one direction is often missing, both count).  A pool is a row of top_k / for_users output at
k = N <= 1024: candidates (col, val) in served order.  Greedily, for t = 0 .. k - 1, over the unpicked candidates c:
r_c = max over the picked s of sim(c, s); c is eligible when r_c < max_sim; the eligible c with the largest
1000 * val_c - penalty * r_c (int64) is picked, ties to the smaller pool position; a request ends early when nobody is
eligible.  penalty is rating points x 1000 per unit of similarity, max_sim is in milli (1001: nothing is excluded).

Which penalty, which max_sim?  diversify_grid / evaluate_diversity (qrlsh_diversify_grid) run the rule under a list of
settings over one adjacency per request and score every setting's lists on the device: evaluate_ranking's words against
a held-out truth and list_redundancy's words, 24 exact integer totals per setting -> DiversityGrid."""
import numpy as np
import torch

from . import _lib
from . import ops
from . import predict, ranking, recommend
from ._args import _int_in
from ._inputs import WORKSPACE_BUDGET, blocks, coo_triple, ids32, int_array, like_matrix, lists_csr, on_device
from ._inputs import or_flags, raise_flags, request_blocks, select_ids
from .ops import _ptr, _stream

MAX_POOL = _lib.DIVERSIFY_MAX_POOL
MAX_PENALTY = _lib.DIVERSIFY_MAX_PENALTY

_FLAG_TEXT = ((1, "a query's neighbour index is outside [0, %(nq)d)"),
              (2, "a candidate column is outside [0, %(nq)d)"),
              (4, "a candidate appears twice in one pool"),
              (8, "a pool's edges do not fit the workspace (a list row names a query twice?)"),
              (16, "a setting's penalty or max_sim is outside its range"),
              (32, "a user id is outside the truth's rows"),
              (64, "gains must not be negative"))
MAX_SETTINGS = 128    # QRLSH_GRID_MAX_SETTINGS: settings per library call
GRID_LINE, GRID_TOTALS = 12, 24
GRID_METRICS = ("ndcg", "precision", "recall", "hit_rate")


def _check_rule(k, penalty, max_sim):
    return (_int_in(k, "k", 1, MAX_POOL), _int_in(penalty, "penalty", 0, MAX_PENALTY),
            _int_in(max_sim, "max_sim", 0, 1001))


def _i32(t, device):
    return t.to(device=device, dtype=torch.int32).contiguous()


def _max_row(q_off):
    """the longest list row (a read-back of one word: it sizes the workspace)"""
    return int((q_off[1:] - q_off[:-1]).max().item()) if q_off.numel() > 1 else 0


def _block(lib, m, n, max_row, device, ids=None, full=None):
    """requests per library call under WORKSPACE_BUDGET, the workspace for them, and request_blocks' ids"""
    def need(blk):
        return int(lib.qrlsh_diversify_workspace_bytes(blk, n, max_row))
    blk, ids = request_blocks(m, need, WORKSPACE_BUDGET, ids=ids, full=full, device=device)
    return blk, ops._ws(need(blk), device), ids


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
    blk, ws, _ = _block(lib, m, n, max_row, device)
    parts = blocks(m, blk)
    flags = torch.zeros((len(parts),), dtype=torch.int32, device=device)
    st = _stream()
    for b, i0, i1 in parts:
        _lib.check(lib.qrlsh_diversify(_ptr(ci[i0:i1]), _ptr(cv[i0:i1]), _ptr(av[i0:i1]), i1 - i0, n, nq, _ptr(csr[0]),
                                       _ptr(csr[1]), _ptr(csr[2]), k, penalty, max_sim, _ptr(idx[i0:i1]),
                                       _ptr(val[i0:i1]), _ptr(red[i0:i1]), _ptr(count[i0:i1]), _ptr(flags[b:b + 1]),
                                       _ptr(ws), ws.numel(), st))
    raise_flags(or_flags(flags.cpu()), _FLAG_TEXT, nq=nq)   # the one read-back of the call
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
    nq = _int_in(nq, "nq", 0, 2**31 - 1)
    ci, cv, av = int_array(cand_idx, 2, "cand_idx"), int_array(cand_val, 2, "cand_val"), int_array(avail, 1, "avail")
    if tuple(ci.shape) != tuple(cv.shape) or av.shape[0] != ci.shape[0]:
        raise ValueError("cand_idx %s, cand_val %s and avail %s do not belong together"
                         % (tuple(ci.shape), tuple(cv.shape), tuple(av.shape)))
    n = int(ci.shape[1])
    if not k <= n <= MAX_POOL:
        raise ValueError("k <= N <= %d is required, got k=%d N=%d" % (MAX_POOL, k, n))
    coo = coo_triple(q_src, q_dst, q_milli)
    _lib.load()
    csr = lists_csr(coo, nq, device)
    return _rerank(_i32(ci, device), _i32(cv, device), _i32(av, device), csr, nq, k, penalty, max_sim,
                   _max_row(csr[0]), device)


def default_pool(k):
    return min(MAX_POOL, max(4 * k, 64))


def _check_pool(k, pool):
    pool = default_pool(k) if pool is None else _int_in(pool, "pool", 1, MAX_POOL)
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
    nq = _int_in(nq, "nq", 0, 2**31 - 1)
    li = int_array(idx, 2, "idx")
    m, k = (int(d) for d in li.shape)
    if not 1 <= k <= MAX_POOL:
        raise ValueError("lists of 1..%d entries are served, got k=%d" % (MAX_POOL, k))
    coo = coo_triple(q_src, q_dst, q_milli)
    lib = _lib.load()
    csr = lists_csr(coo, nq, device)
    li = _i32(li, device)
    out = torch.zeros((4 * m + 5,), dtype=torch.int64, device=device)   # [words m x 4][totals 4][flag]
    if m:
        blk, ws, _ = _block(lib, m, k, _max_row(csr[0]), device)
        st = _stream()
        for _, i0, i1 in blocks(m, blk):
            _lib.check(lib.qrlsh_list_redundancy(_ptr(li[i0:i1]), i1 - i0, k, nq, _ptr(csr[0]), _ptr(csr[1]),
                                                 _ptr(csr[2]), _ptr(out[4 * i0:]), _ptr(out[4 * m:]),
                                                 _ptr(out[4 * m + 4:]), _ptr(ws), ws.numel(), st))
    host = out.cpu().numpy()
    raise_flags(int(host[4 * m + 4]), _FLAG_TEXT, nq=nq)
    return Redundancy(host[:4 * m].reshape(m, 4).copy(), host[4 * m:4 * m + 4].copy())


# ------------------------------------------------------------------- the rerank under a grid of settings, scored
def _check_settings(settings):
    try:
        rows = [tuple(x) for x in settings]
    except TypeError:
        rows = []
    if not rows or any(len(r) != 2 for r in rows):
        raise ValueError("settings must be a non-empty sequence of (penalty, max_sim) pairs")
    return [(_int_in(p, "penalty", 0, MAX_PENALTY), _int_in(ms, "max_sim", 0, 1001)) for p, ms in rows]


def _ratios(a, b):
    return [int(x) / int(y) if int(y) else float("nan") for x, y in zip(a, b)]


class DiversityGrid:
    """The result of diversify_grid() / evaluate_diversity() / Recommender.tune_diversity().
    settings: the S (penalty, max_sim) pairs.  totals: host int64 (S, 24) per setting -- words 0-7 the column sums of the
      per-request words 0-7 (listed, hits, known, first_hit, dcg, relevant test cells, test cells, avail), 8 requests
      served, 9 requests with >= 1 relevant test cell, 10 requests with >= 1 hit, 11 the sum of the ideal DCG (0-11 are
      RankingEvaluation.totals over the diversified lists), 12 in-list pairs of stored neighbours, 13 the sum of their
      similarities (milli), 14 the largest, 15 the sum of the picks' red, 16 requests whose list differs from the plain
      prefix of their pool, 17 requests that ended before min(k, pool).
    per_request: device int64 (S, m, 12) (want_per_request) -- the eight words above, then the list's pairs, their
      similarity sum, the largest similarity and the sum of red.  idx, val, red (S, m, k), count (S, m): device int32,
      diversify()'s output per setting (want_lists).
    Per setting, lists of Python floats: precision, recall, ndcg, hit_rate with RankingEvaluation's divisions (nan on a
    zero denominator, as without a truth); pairs_per_list and mean_sim as Redundancy computes them (over the requests
    served); changed_share = word 16 / requests served; ended_early = word 17 (a count)."""

    def __init__(self, settings, totals, per_request=None, idx=None, val=None, red=None, count=None):
        self.settings = [(int(p), int(ms)) for p, ms in settings]
        self.totals = np.asarray(totals, dtype=np.int64).reshape(len(self.settings), GRID_TOTALS)
        self.per_request, self.idx, self.val, self.red, self.count = per_request, idx, val, red, count
        t = self.totals
        self.precision = _ratios(t[:, 1], t[:, 0])
        self.recall = _ratios(t[:, 1], t[:, 5])
        self.hit_rate = _ratios(t[:, 10], t[:, 9])
        self.ndcg = _ratios(t[:, 4], t[:, 11])
        self.pairs_per_list = [int(x) / int(y) if int(y) else 0.0 for x, y in zip(t[:, 12], t[:, 8])]
        self.mean_sim = [int(x) / int(y) / 1000.0 if int(y) else 0.0 for x, y in zip(t[:, 13], t[:, 12])]
        self.changed_share = [int(x) / int(y) if int(y) else 0.0 for x, y in zip(t[:, 16], t[:, 8])]
        self.ended_early = [int(x) for x in t[:, 17]]

    def setting(self, index):
        """(penalty, max_sim) of setting `index`"""
        return self.settings[int(index)]

    def _metric(self, metric):
        if metric not in GRID_METRICS:
            raise ValueError("metric must be one of %s" % (GRID_METRICS,))
        return getattr(self, metric)

    def best(self, metric="ndcg", max_pairs_per_list=None):
        """The setting with the highest `metric` ('ndcg', 'precision', 'recall' or 'hit_rate') among those with
        pairs_per_list <= max_pairs_per_list (None: all of them); ties go to the lowest index; a setting without a figure
        (nan) never wins.  -> (penalty, max_sim, index).  ValueError when no setting is within the bound."""
        value = self._metric(metric)
        ok = [v == v and (max_pairs_per_list is None or p <= float(max_pairs_per_list))
              for v, p in zip(value, self.pairs_per_list)]
        if not any(ok):
            raise ValueError("no setting has a %s at pairs_per_list <= %r" % (metric, max_pairs_per_list))
        index = max((i for i in range(len(value)) if ok[i]), key=lambda i: (value[i], -i))
        return self.settings[index] + (index,)

    def least_redundant(self, metric="ndcg", keep=0.98):
        """Among the settings whose `metric` is at least `keep` times the grid's largest: the one with the fewest pairs
        per list, then the smallest similarity sum, then the lowest index.  -> (penalty, max_sim, index).  ValueError
        when no setting has a figure."""
        value = self._metric(metric)
        known = [v for v in value if v == v]
        if not known:
            raise ValueError("no setting has a %s" % metric)
        bar = float(keep) * max(known)
        index = min((i for i in range(len(value)) if value[i] == value[i] and value[i] >= bar),
                    key=lambda i: (self.pairs_per_list[i], int(self.totals[i, 13]), i))
        return self.settings[index] + (index,)

    def __repr__(self):
        return "DiversityGrid(%d settings, %d requests)" % (len(self.settings), int(self.totals[0, 8]))


def _grid(ci, cv, av, csr, nq, k, settings, max_row, device, scoring=None, want_per_request=False, want_lists=False):
    """diversify_grid() over device int32 pools and the device CSR of the lists.  scoring: None or (truth int32 (nu, nq),
    users int32 (m,) or None, relevant, gain int64 (k,), gain_prefix int64 (k + 1,), request_counts int64 (m, 2) or
    None), device tensors."""
    lib = _lib.load()
    m, n = (int(d) for d in ci.shape)
    S = len(settings)
    pen = torch.tensor([p for p, _ in settings], dtype=torch.int64, device=device)
    cut = torch.tensor([ms for _, ms in settings], dtype=torch.int32, device=device)
    per = torch.zeros((S, m, GRID_LINE), dtype=torch.int64, device=device) if want_per_request else None
    lists = None
    if want_lists:
        lists = [torch.empty((S, m, k), dtype=torch.int32, device=device) for _ in range(3)]
        lists.append(torch.empty((S, m), dtype=torch.int32, device=device))
    back = torch.zeros((S * GRID_TOTALS + 1,), dtype=torch.int64, device=device)   # [totals S x 24][flag: low half]
    if m:
        if scoring is None:
            truth, users, relevant, gain, prefix, counts, nu = None, None, 1, None, None, None, 0
        else:
            truth, users, relevant, gain, prefix, counts = scoring
            nu = int(truth.shape[0])
        # without users request x is row x: of a later block still row i0 + x
        blk, ws, users = _block(lib, m, n, max_row, device, users, None if scoring is None else m)
        widest = min(S, MAX_SETTINGS)
        whole = blk >= m
        tmp = None
        if not whole:   # a row block's [settings][rows] outputs, copied into place after each call
            tmp = [torch.empty((widest * blk * w,), dtype=dt, device=device) if on else None
                   for w, dt, on in ((k, torch.int32, want_lists), (k, torch.int32, want_lists),
                                     (k, torch.int32, want_lists), (1, torch.int32, want_lists),
                                     (GRID_LINE, torch.int64, want_per_request))]
        st = _stream()
        for c0 in range(0, S, MAX_SETTINGS):
            c1 = min(S, c0 + MAX_SETTINGS)
            for _, i0, i1 in blocks(m, blk):
                if whole:
                    outs = [t[c0:c1] for t in lists] if want_lists else [None] * 4
                    outs.append(per[c0:c1] if want_per_request else None)
                else:
                    outs = tmp
                _lib.check(lib.qrlsh_diversify_grid(
                    _ptr(ci[i0:i1]), _ptr(cv[i0:i1]), _ptr(av[i0:i1]), i1 - i0, n, nq, _ptr(csr[0]), _ptr(csr[1]),
                    _ptr(csr[2]), k, _ptr(pen[c0:c1]), _ptr(cut[c0:c1]), c1 - c0,
                    None if truth is None else _ptr(truth), nu, None if users is None else _ptr(users[i0:i1]),
                    int(relevant), None if gain is None else _ptr(gain), None if prefix is None else _ptr(prefix),
                    None if counts is None else _ptr(counts[i0:i1]), *(None if t is None else _ptr(t) for t in outs),
                    _ptr(back[c0 * GRID_TOTALS:]), _ptr(back[S * GRID_TOTALS:]), _ptr(ws), ws.numel(), st))
                if not whole:
                    full = (lists if want_lists else [None] * 4) + [per]
                    for dst, src in zip(full, tmp):
                        if dst is not None:
                            shape = (c1 - c0, i1 - i0) + tuple(dst.shape[2:])
                            dst[c0:c1, i0:i1] = src[:int(np.prod(shape))].view(shape)
    host = back.cpu().numpy()   # the flags together with the totals
    raise_flags(int(host[S * GRID_TOTALS]), _FLAG_TEXT, nq=nq)
    return DiversityGrid(settings, host[:S * GRID_TOTALS].copy(), per, *(lists or [None] * 4))


def _scoring_checks(k, m, relevant, gains):
    """the scoring arguments that need no device -> (relevant, gain, gain_prefix) host values"""
    if isinstance(relevant, bool) or not isinstance(relevant, (int, np.integer)) or not 1 <= int(relevant) < 2**31:
        raise ValueError("relevant must be an int32 >= 1, got %r" % (relevant,))
    gain, prefix = ranking._gain_tables(gains, k, m)
    return int(relevant), gain, prefix


def diversify_grid(cand_idx, cand_val, avail, q_src, q_dst, q_milli, nq, k, settings, truth=None, users=None,
                   relevant=None, gains=None, request_counts=None, want_per_request=False, want_lists=False,
                   device="cuda"):
    """diversify() under every (penalty, max_sim) of `settings` at once, each setting's lists scored on the device
    (qrlsh_diversify_grid): the adjacency of a pool does not depend on the setting and is built once per request; per
    setting there is the greedy selection, the truth at the picks and the redundancy of the list, folded out of the
    pool's adjacency.  Pools, lists, nq and k as diversify takes them.
    truth: None, or (nu, nq) integers -- the held-out matrix the picks are held to; then users: (m,) row ids (None:
    request x is row x, m <= nu), relevant: a pick with truth >= relevant is a hit (an int32 >= 1, required), gains: k
    non-negative integers (default dcg_gains(k)), request_counts: None or (m, 2) integers, the relevant test cells and
    the test cells of each request (words 5 and 6 of evaluate_ranking's per_user lines; None: zeros, so recall, hit_rate
    and ndcg have no denominator).
    More than 128 settings run as successive library calls over the same pools and are stitched together; requests run
    in row blocks under WORKSPACE_BUDGET and the blocks' totals are added on the device.
    -> DiversityGrid (two read-backs: the longest list row, then the flags together with the totals).
    Raises ValueError before anything is uploaded for a bad k, setting, nq, shape, relevant, gains or host user id, and
    through the library's flags as diversify does, and for a device user id outside the truth's rows."""
    k = _check_rule(k, 0, 1001)[0]
    settings = _check_settings(settings)
    nq = _int_in(nq, "nq", 0, 2**31 - 1)
    ci, cv, av = int_array(cand_idx, 2, "cand_idx"), int_array(cand_val, 2, "cand_val"), int_array(avail, 1, "avail")
    if tuple(ci.shape) != tuple(cv.shape) or av.shape[0] != ci.shape[0]:
        raise ValueError("cand_idx %s, cand_val %s and avail %s do not belong together"
                         % (tuple(ci.shape), tuple(cv.shape), tuple(av.shape)))
    m, n = (int(d) for d in ci.shape)
    if not k <= n <= MAX_POOL:
        raise ValueError("k <= N <= %d is required, got k=%d N=%d" % (MAX_POOL, k, n))
    coo = coo_triple(q_src, q_dst, q_milli)
    scoring = None
    if truth is None:
        if users is not None or request_counts is not None or gains is not None or relevant is not None:
            raise ValueError("users, relevant, gains and request_counts need a truth")
    else:
        tt = int_array(truth, 2, "truth")
        nu = int(tt.shape[0])
        if int(tt.shape[1]) != nq:
            raise ValueError("truth has %d columns, nq = %d" % (int(tt.shape[1]), nq))
        relevant, gain, prefix = _scoring_checks(k, m, relevant, gains)
        if users is None:
            if m > nu:
                raise ValueError("%d requests but %d rows of truth: pass users" % (m, nu))
            ut = None
        else:
            named, ut, _ = select_ids(users, nu, "user", "users", host_tensors=True)
            if named != m:
                raise ValueError("users must name one row per request (%d), got %d" % (m, named))
        rc = None
        if request_counts is not None:
            rc = int_array(request_counts, 2, "request_counts")
            if tuple(rc.shape) != (m, 2):
                raise ValueError("request_counts must have shape (%d, 2), got %s" % (m, tuple(rc.shape)))
        scoring = (tt, ut, relevant, gain, prefix, rc)
    _lib.load()
    csr = lists_csr(coo, nq, device)
    if scoring is not None:
        tt, ut, relevant, gain, prefix, rc = scoring
        scoring = (_i32(tt, device), None if ut is None else ids32(ut, nu, device), relevant,
                   torch.from_numpy(gain).to(device), torch.from_numpy(prefix).to(device),
                   None if rc is None else rc.to(device=device, dtype=torch.int64).contiguous())
    return _grid(_i32(ci, device), _i32(cv, device), _i32(av, device), csr, nq, k, settings, _max_row(csr[0]), device,
                 scoring, want_per_request, want_lists)


def evaluate_diversity(train, truth, q_src, q_dst, q_milli, user_sims, k, relevant, settings, pool=None, users=None,
                       gains=None, lo=0, slices=0, sum_order="pairwise", want_per_request=False, want_lists=False,
                       query_weight=None, user_weight=None, default_mean=None, device="cuda"):
    """What does each (penalty, max_sim) cost in NDCG, and what redundancy does it remove?  evaluate_ranking(train, ...,
    candidates="all") at k = pool serves every request its pool and counts its test cells; diversify_grid then reranks
    those pools to k under every setting and holds each list to `truth`.  The pools never leave the device.
    train / truth, the lists, user_sims, users, relevant, lo, slices, sum_order and the weights: as evaluate_ranking
    takes them; pool: candidates per request, default min(1024, max(4 k, 64)); gains: k integers, default dcg_gains(k);
    settings, want_per_request, want_lists: as diversify_grid takes them.  Setting (0, 1001) gives evaluate_ranking(...,
    k)'s figures.  -> DiversityGrid.  Raises what evaluate_ranking and diversify_grid raise; every check that needs no
    device precedes any upload."""
    k = _check_rule(k, 0, 1001)[0]
    pool = _check_pool(k, pool)
    settings = _check_settings(settings)
    ranking.check_arguments(pool, relevant, "all", lo, slices)
    a = predict.ServeInputs(train, q_src, q_dst, q_milli, user_sims, users, sum_order)
    truth = like_matrix(truth, "truth", (a.nu, a.nq), "train")
    relevant, gain, prefix = _scoring_checks(k, a.m, relevant, gains)
    pool_gains = ranking._gain_tables(None, pool, a.m)
    weights = predict.weights(query_weight, user_weight, default_mean)
    _lib.load()
    a.upload(device)
    t = on_device(truth, device)
    ev = ranking._score(a, t, pool, relevant, "all", pool_gains[0], pool_gains[1], lo, slices, weights)
    dev = a.r.device
    scoring = (t, a.ut, relevant, torch.from_numpy(gain).to(dev), torch.from_numpy(prefix).to(dev),
               ev.per_user[:, 5:7].contiguous())
    return _grid(ev.idx, ev.val, ev.avail, (a.q_off, a.q_idx, a.q_milli), a.nq, k, settings, _max_row(a.q_off), dev,
                 scoring, want_per_request, want_lists)
