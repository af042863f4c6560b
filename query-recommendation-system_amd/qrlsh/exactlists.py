"""The exact neighbour lists (qrlsh_exact_neighbours): what list_fidelity() holds the served lists to, produced.

For chosen queries, or all of them, the top K by Jaccard over the CSR answer sets, J(s, j) = |A(s) & A(j)| / |A(s) | A(j)|:
the j != s that share a row with s, by J descending, ties by j ascending, cut at K -- a total order, so the lists are
unique.  ExactLists.coo() gives them in the (src, dst, milli) form every serving and evaluation call takes, so evaluate,
evaluate_ranking, for_users and list_fidelity run over the exact lists beside the LSH lists.  Integer arithmetic on the
device throughout; nothing of size requests x queries is written."""
import numpy as np
import torch

from . import _lib
from . import ops
from . import postings as _postings
from ._args import _int_in
from ._inputs import MAX_REQUESTS, WORKSPACE_BUDGET, answer_csr, blocks, ids32, or_flags, raise_flags
from ._inputs import request_blocks, select_ids
from .ops import _ptr, _stream
MAX_K = _lib.FIDELITY_MAX_K
MAX_D = _lib.FIDELITY_MAX_D

_FLAG_TEXT = ((4, "a chosen query is outside [0, %(nq)d)"),
              (8, "an answer-set row id is outside [0, %(D)d)"))


def jaccard_milli(inter, union):
    """round-half-up of 1000 J in integers: (2000 inter + union) // (2 union); 0 where union is 0.  int64 tensors or
    arrays of any integer type."""
    if isinstance(inter, torch.Tensor):
        i, u = inter.to(torch.int64), union.to(torch.int64)
        return torch.where(u > 0, (2000 * i + u) // (2 * u).clamp(min=1), torch.zeros_like(u))
    i, u = np.asarray(inter, dtype=np.int64), np.asarray(union, dtype=np.int64)
    return np.where(u > 0, (2000 * i + u) // np.maximum(2 * u, 1), 0)


class ExactLists:
    """The result of exact_neighbours() / Recommender.exact_query_lists(); device tensors.
    K: the list length.  queries int32 (m,): the chosen queries.
    dst int32 (m, K): request x's neighbours by J descending, ties by id ascending, -1 past listed[x];
    inter, union int32 (m, K): |A(s) & A(dst)| and |A(s) | A(dst)|, 0 past listed[x], so J = inter / union exactly;
    listed int32 (m,) = min(K, positives); positives int32 (m,): the j != s that share a row with s."""

    def __init__(self, K, queries, dst, inter, union, listed, positives):
        self.K = int(K)
        self.queries, self.dst, self.inter, self.union = queries, dst, inter, union
        self.listed, self.positives = listed, positives

    def __repr__(self):
        return "ExactLists(K=%d, requests=%d)" % (self.K, int(self.queries.numel()))

    def coo(self):
        """-> (src, dst, milli) int32 device tensors sorted by source: the lists in the form predict.lists_csr,
        predict_users, for_users, evaluate, evaluate_ranking, diversify and list_fidelity take.  src is the chosen
        query's id; milli = (2000 inter + union) // (2 union), round-half-up of 1000 J in integers.  Entries whose
        milli is 0 are left out: J descends along a row, so they are its tail -- a truncation, and a prefix of a row
        stays the exact list at that shorter length.  WITHIN EQUAL milli THE ORDER IS THAT OF THE EXACT J (then id),
        NOT OF THE ID: milli is a rounding of the key the rows are sorted by.
        ValueError when a query was requested more than once (a source has one row)."""
        q = self.queries.to(torch.int64)
        order = torch.argsort(q, stable=True)
        qs = q[order]
        if qs.numel() > 1 and bool((qs[1:] == qs[:-1]).any().item()):
            raise ValueError("a query was requested more than once: a list row per source")
        milli = jaccard_milli(self.inter, self.union)[order]
        keep = (self.dst[order] >= 0) & (milli > 0)
        src = qs[:, None].expand(-1, self.K)[keep].to(torch.int32).contiguous()
        return src, self.dst[order][keep].contiguous(), milli[keep].to(torch.int32).contiguous()


def slice_count(nq, m, D, slices=0):
    """the slices of the ids a call over m requests runs (qrlsh_exact_neighbours_slices; 0 for arguments out of range):
    its scratch is m * slices * K * 3 int32 words"""
    return int(_lib.load().qrlsh_exact_neighbours_slices(int(nq), int(m), int(D), int(slices)))


def exact_neighbours(offsets, rows, D, K, queries=None, slices=0, device="cuda", postings=None):
    """The exact top K by Jaccard of chosen queries over all nq queries -> ExactLists (one read-back, for the flags).
    offsets (nq + 1,) / rows: the CSR answer sets over D table rows (row ids in [0, D), ascending per query, as
    answer_sets gives them); K in 1..64; queries: ids of the chosen queries (any order, repeats allowed; a host sequence
    or a device tensor), None = all; slices: 0 = automatic, else 1..256 slices of the ids (the result depends on
    neither).  Tensors are used where they are, host data is uploaded.  Requests run in blocks of whole workgroups whose
    partial lists stay within WORKSPACE_BUDGET.
    postings: None = the sweep over all queries; an AnswerPostings (answer_postings() of the same answer sets) = the same
    lists, word for word, from the posting lists of each request's own rows: the cost follows the request's matches, not
    nq ("Exact lists from postings").  slices must stay 0 with it; postings built from another
    shape (nq, entries, D) are refused before any device work.  Postings of another CSR of the same shape are refused by
    the library's flag only where a request meets a bound or an id out of range; otherwise they are NOT refused and the
    numbers are wrong (qrlsh/postings.py).
    Raises ValueError before anything is uploaded for a bad K, D (at most 2^20), slices or shape and a host query id
    outside [0, nq); through the library's flags for a device query id outside [0, nq) and an answer-set row id outside
    [0, D) (nothing is returned then)."""
    K = _int_in(K, "K", 1, MAX_K)
    D = _int_in(D, "D", 0, MAX_D)
    slices = _int_in(slices, "slices", 0, 256)
    off, r = answer_csr(offsets, rows)
    nq = int(off.numel()) - 1
    m, ids, _ = select_ids(queries, nq, "query", "queries", host_tensors=True)
    if m and not nq:
        raise ValueError("query id outside [0, 0)")
    if postings is not None:
        _postings.check_postings(postings, nq, int(r.numel()), D, slices)
    lib = _lib.load()
    off = off.to(device=device, dtype=torch.int64).contiguous()
    r = r.to(device=device, dtype=torch.int32).contiguous()
    ids = torch.arange(nq, dtype=torch.int32, device=device) if ids is None else ids32(ids, nq, device)
    if postings is not None:
        dst, inter, union, counts = _postings.exact_lists(off, r, nq, D, K, ids, m, postings, device)
        return ExactLists(K, ids, dst, inter, union, counts[:, 0].contiguous(), counts[:, 1].contiguous())
    dst = torch.full((m, K), -1, dtype=torch.int32, device=device)       # the library writes nothing when nq is 0
    inter = torch.zeros((2, m, K), dtype=torch.int32, device=device)
    counts = torch.zeros((m, 2), dtype=torch.int32, device=device)
    G = max(1, int(lib.qrlsh_list_fidelity_group(D)))

    def scratch_bytes(n):
        return n * int(lib.qrlsh_exact_neighbours_slices(nq, n, D, slices)) * K * 3 * 4
    blk, _ = request_blocks(m, scratch_bytes, WORKSPACE_BUDGET, group=G, cap=MAX_REQUESTS)
    parts = blocks(m, blk)
    flags = torch.zeros((max(len(parts), 1),), dtype=torch.int32, device=device)
    # a shorter last block can run more slices than the full ones
    scratch = ops._ws(max(scratch_bytes(i1 - i0) for _, i0, i1 in parts), device) if m else None
    st = _stream()
    for b, i0, i1 in parts:
        _lib.check(lib.qrlsh_exact_neighbours(_ptr(off), _ptr(r), nq, D, _ptr(ids[i0:i1]), i1 - i0, K, slices,
                                              _ptr(dst[i0:i1]), _ptr(inter[0, i0:i1]), _ptr(inter[1, i0:i1]),
                                              _ptr(counts[i0:i1]), _ptr(flags[b:]), _ptr(scratch),
                                              scratch_bytes(i1 - i0), st))
    raise_flags(or_flags(flags.cpu()), _FLAG_TEXT, nq=nq, D=D)
    return ExactLists(K, ids, dst, inter[0], inter[1], counts[:, 0].contiguous(), counts[:, 1].contiguous())
