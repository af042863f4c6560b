"""Serving chosen queries from the live lists (qrlsh_predict_queries / qrlsh_recommend_queries): the question the other
way round.  predict_queries() returns the completed columns of queries that are columns of the matrix, for_queries()
their top-k users ("whom do I show query j?"), query_utility() eight exact words per query ("how useful is query j to
the user base?") -- all without the (nu, nq) prediction matrix, so the answers are as current as the lists."""
import numpy as np
import torch

from . import _lib
from . import ops
from . import predict
from ._inputs import blocks, request_blocks
from .ops import _ptr, _stream
from .recommend import WORKSPACE_BUDGET, _check_select_args


class QueryUtility:
    """.words int64 (m, 8), host, per requested query: [0] users who rated it, [1] the sum of their ratings, [2] unrated
    users with a non-zero prediction, [3] the sum of those predictions, [4] unrated users with prediction 0 (missed),
    and the unrated users by the non-zero sides of their blend: [5] the query side alone, [6] the user side alone, [7]
    both.  .rated / .predicted / .missed = words 0 / 2 / 4.  float64 (m,), nan where the denominator is 0:
    .utility = (w1 + w3) / (w0 + w2), the mean value of the query over everyone who has one; .mean_rating = w1 / w0;
    .mean_prediction = w3 / w2; .coverage = 1 - missed / unrated.  .by_branch = {'query' / 'user' / 'both': int64 (m,)}."""

    def __init__(self, words):
        w = self.words = np.ascontiguousarray(words, dtype=np.int64).reshape(-1, 8)
        self.rated, self.predicted, self.missed = w[:, 0], w[:, 2], w[:, 4]
        self.utility = _ratio(w[:, 1] + w[:, 3], w[:, 0] + w[:, 2])
        self.mean_rating = _ratio(w[:, 1], w[:, 0])
        self.mean_prediction = _ratio(w[:, 3], w[:, 2])
        self.coverage = 1.0 - _ratio(w[:, 4], w[:, 2] + w[:, 4])
        self.by_branch = {"query": w[:, 5], "user": w[:, 6], "both": w[:, 7]}

    def __repr__(self):
        t = self.words.sum(axis=0)
        return "QueryUtility(queries=%d, rated=%d, predicted=%d, missed=%d)" % (len(self.words), t[0], t[2], t[4])


def _ratio(num, den):
    """num / den as float64, nan where den == 0"""
    out = np.full(len(den), np.nan, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def _run(a, weights, device, k=None, lo=0, slices=0, want_columns=False, want_words=False):
    """The requests of checked and uploaded ServeInputs(ids="queries") in blocks under WORKSPACE_BUDGET, counting the
    raw columns (cols_tmp) plus the workspace.  k = None: qrlsh_predict_queries (columns when asked for, else the words
    alone); else qrlsh_recommend_queries.  -> (columns or None, (users, val, avail) or None, QueryUtility or None); the
    flags come back with the words in one read-back."""
    lib = _lib.load()
    m, nu = a.m, a.nu
    out = torch.empty((m, nu), dtype=torch.int32, device=device) if want_columns else None
    sel = None
    if k is not None:
        sel = (torch.empty((m, k), dtype=torch.int32, device=device), torch.empty((m, k), dtype=torch.int32, device=device),
               torch.empty((m,), dtype=torch.int32, device=device))
    if m == 0:
        return out, sel, QueryUtility(np.zeros((0, 8), dtype=np.int64)) if want_words else None

    def ws_bytes(blk):
        return int(lib.qrlsh_recommend_users_workspace_bytes(blk, nu, k, slices)) if k is not None else 0

    blk, ids = request_blocks(m, lambda blk: blk * nu * 4 + ws_bytes(blk), WORKSPACE_BUDGET, ids=a.ut, full=a.nq,
                              device=device)
    cols = ops._ws(blk * nu * 4, device)
    ws = ops._ws(ws_bytes(blk), device)
    parts = blocks(m, blk)
    # the words and, behind them, one 8-byte slot per block whose low half is that block's flag word
    back = torch.zeros((m * 8 + len(parts),), dtype=torch.int64, device=device)
    args = a.lists_args(*weights)
    st = _stream()
    for b, i0, i1 in parts:
        q = None if ids is None else _ptr(ids[i0:i1])
        words = _ptr(back[i0 * 8:i1 * 8]) if want_words else None
        flags = _ptr(back[m * 8 + b:m * 8 + b + 1])
        if k is None:
            _lib.check(lib.qrlsh_predict_queries(*args, q, i1 - i0, None if out is None else _ptr(out[i0:i1]),
                                                 _ptr(cols), words, flags, st))
        else:
            _lib.check(lib.qrlsh_recommend_queries(*args, q, i1 - i0, k, lo, slices, _ptr(sel[0][i0:i1]),
                                                   _ptr(sel[1][i0:i1]), _ptr(sel[2][i0:i1]), words, flags, _ptr(cols),
                                                   _ptr(ws), ws.numel(), st))
    host = back.cpu()
    a.raise_flags(host[m * 8:])
    return out, sel, QueryUtility(host[:m * 8].numpy()) if want_words else None


def predict_queries(ratings, q_src, q_dst, q_milli, user_sims, queries, query_weight=None, user_weight=None,
                    default_mean=None, device="cuda", sum_order="pairwise", utility=False):
    """The completed columns of chosen queries, straight from the lists: columns `queries` of fill_predictions' result,
    transposed, cell for cell, without the (nu, nq) matrix (qrlsh_predict_queries).
    ratings, the lists and user_sims as predict_users takes them.  queries: column ids (any order, repeats allowed; a
    host sequence or a device tensor), None = every column.
    -> int32 device tensor (m, nu); with utility=True (columns, QueryUtility).
    Raises ValueError for a bad shape or sum_order, a list longer than 64, a neighbour index outside [0, nq) and a query
    id outside [0, nq) (host ids before anything is uploaded; device ids and the lists through the library's flags)."""
    a = predict.ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, queries, sum_order, ids="queries")
    _lib.load()
    a.upload(device)
    out, _, words = _run(a, predict.weights(query_weight, user_weight, default_mean), device, want_columns=True,
                         want_words=bool(utility))
    return (out, words) if utility else out


def for_queries(ratings, q_src, q_dst, q_milli, user_sims, queries, k, lo=0, slices=0, sum_order="pairwise",
                query_weight=None, user_weight=None, default_mean=None, device="cuda", utility=False):
    """Top-k users of chosen queries from the live lists (qrlsh_recommend_queries): what top_k returns for the transposed
    columns -- top_k(ratings[:, queries].T, fill_predictions(...)[:, queries].T, k) -- output for output.  A user is
    eligible when it has not rated the query and its prediction is not 0; value descending, then user ascending.
    Arguments as predict_queries takes them; k, lo and slices as top_k takes them.
    -> (users int32 (m, k), val int32 (m, k), avail int32 (m,)) device tensors, -1 / 0 past min(k, avail); with
    utility=True the QueryUtility as a fourth.  Raises ValueError as predict_queries does, and for a bad k, lo or slices."""
    k = _check_select_args(k, lo, slices)
    a = predict.ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, queries, sum_order, ids="queries")
    _lib.load()
    a.upload(device)
    _, sel, words = _run(a, predict.weights(query_weight, user_weight, default_mean), device, k=k, lo=int(lo),
                         slices=int(slices), want_words=bool(utility))
    return sel + (words,) if utility else sel


def query_utility(ratings, q_src, q_dst, q_milli, user_sims, queries=None, query_weight=None, user_weight=None,
                  default_mean=None, device="cuda", sum_order="pairwise"):
    """How useful each chosen query (default: every column) is to the whole user base -> QueryUtility.  No column is
    written (qrlsh_predict_queries with out = NULL); one read-back, the flags with the words.  Arguments and errors as
    predict_queries."""
    a = predict.ServeInputs(ratings, q_src, q_dst, q_milli, user_sims, queries, sum_order, ids="queries")
    _lib.load()
    a.upload(device)
    return _run(a, predict.weights(query_weight, user_weight, default_mean), device, want_words=True)[2]
