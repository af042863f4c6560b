"""How much of the exact neighbourhoods the served lists hold (qrlsh_edge_overlaps, qrlsh_list_fidelity).

The lists come from MinHash + banding, ranked by a cosine over raw signature values and cut at K.  "True" neighbours are
those by Jaccard over the answer sets, J(s, j) = |A(s) & A(j)| / |A(s) | A(j)| (0 when both are empty): the quantity
MinHash estimates.  edge_overlaps() gives the exact intersection of any edges; list_fidelity() holds the first
min(len, K) entries of chosen queries' lists to the exact Jaccard over ALL queries -> ListFidelity: recall against the
exact top K, the share of listed entries that share no row at all, and how often the stored order disagrees with the
exact one.  Integer arithmetic on the device throughout; nothing of size requests x queries is written."""
import numpy as np
import torch

from . import _lib
from ._args import _int_in
from ._inputs import MAX_REQUESTS, WORKSPACE_BUDGET, answer_csr, blocks, coo_triple, ids32, int_array, lists_csr
from ._inputs import or_flags, raise_flags, request_blocks, select_ids
from .ops import _ptr, _stream

MAX_K = _lib.FIDELITY_MAX_K
MAX_D = _lib.FIDELITY_MAX_D
_REQUEST_BYTES = 4 * MAX_K * 4 + 8 * 8

_FLAG_TEXT = ((1, "a chosen query's list row is longer than %d entries" % MAX_K),
              (2, "a query's neighbour index is outside [0, %(nq)d)"),
              (4, "a chosen query is outside [0, %(nq)d)"),
              (8, "an answer-set row id is outside [0, %(D)d)"))


def group_size(D):
    """requests a workgroup of the sweep serves at D table rows (qrlsh_list_fidelity_group; 0 for a D out of range)"""
    return int(_lib.load().qrlsh_list_fidelity_group(int(D)))


def mix64_array(x):
    """evaluate.mix64 over a uint64 numpy array"""
    z = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_positions(nq, sample, seed=0):
    """The seeded sample of Recommender.list_fidelity: the min(sample, nq) positions p of 0 .. nq - 1 with the smallest
    mix64(seed ^ p) (ties to the smaller p), ascending.  A position's key depends on nothing but seed and p, so the samples
    of a growing nq are nested in the sense that a position leaves only when one with a smaller key arrives."""
    nq = _int_in(nq, "nq", 0, 2**31 - 1)
    sample = _int_in(sample, "sample", 0, 2**31 - 1)
    seed = _int_in(seed, "seed", 0, 2**64 - 1)
    keys = mix64_array(np.arange(nq, dtype=np.uint64) ^ np.uint64(seed))
    order = np.argsort(keys, kind="stable")[:min(sample, nq)]
    return np.sort(order).astype(np.int64)


def _ratio(num, den):
    return float(int(num)) / float(int(den)) if int(den) else float("nan")


class ListFidelity:
    """The result of list_fidelity() / Recommender.list_fidelity(); host arrays.
    K: the list length the lists were held to.  queries: int64 (m,) the chosen queries.
    per_request int64 (m, 8): 0 listed = min(row length, K); 1 |A(s)|; 2 positives = the j != s that share a row with s;
      3 hits = listed entries with fewer than K queries strictly better (in the exact top K under some tie-break); 4 sure =
      listed entries with better + equal < K (under every tie-break); 5 reachable = min(K, positives); 6 disjoint = listed
      entries that share no row with s; 7 inversions = pairs of listed entries e before f with J_e < J_f.
    totals int64 (8,): the column sums.
    entries {'inter', 'union', 'better', 'equal'}: int32 (m, 64) per stored entry, 0 past listed.
    recall = hits / reachable, sure_recall = sure / reachable, disjoint_share = disjoint / listed, inversion_share =
    inversions / the in-list pairs (sum of listed (listed - 1) / 2): floats over the totals, nan on a zero denominator."""

    def __init__(self, K, queries, per_request, totals, entries):
        self.K = int(K)
        self.queries = np.asarray(queries, dtype=np.int64).reshape(-1)
        self.per_request = np.ascontiguousarray(per_request, dtype=np.int64).reshape(-1, 8)
        self.totals = np.ascontiguousarray(totals, dtype=np.int64).reshape(8)
        self.entries = entries
        t = self.totals
        listed = self.per_request[:, 0]
        self.pairs = int((listed * (listed - 1) // 2).sum())
        self.recall = _ratio(t[3], t[5])
        self.sure_recall = _ratio(t[4], t[5])
        self.disjoint_share = _ratio(t[6], t[0])
        self.inversion_share = _ratio(t[7], self.pairs)

    def __repr__(self):
        return "ListFidelity(K=%d, requests=%d, listed=%d, reachable=%d, hits=%d, sure=%d, disjoint=%d, inversions=%d)" % (
            self.K, len(self.per_request), self.totals[0], self.totals[5], self.totals[3], self.totals[4],
            self.totals[6], self.totals[7])


def edge_overlaps(offsets, rows, src, dst, device="cuda"):
    """inter int32 device tensor (n,): inter[e] = |A(src[e]) & A(dst[e])|, exact, from the CSR answer sets (offsets
    (nq + 1,), rows: ascending per query, as answer_sets gives them).  With the sizes from offsets the caller has Jaccard =
    inter / (|A| + |B| - inter).  src == dst gives |A|; two empty sets give 0.  Tensors are used where they are.
    Raises ValueError for a bad shape (before anything is uploaded) and for an edge end outside [0, nq) (through the
    library's flag, read back once; nothing is returned then)."""
    off, r = answer_csr(offsets, rows)
    s, d = int_array(src, 1, "src"), int_array(dst, 1, "dst")
    if s.numel() != d.numel():
        raise ValueError("src and dst differ in length")
    nq, n = int(off.numel()) - 1, int(s.numel())
    lib = _lib.load()
    off = off.to(device=device, dtype=torch.int64).contiguous()
    r = r.to(device=device, dtype=torch.int32).contiguous()
    s, d = ids32(s, nq, device), ids32(d, nq, device)
    out = torch.empty((n,), dtype=torch.int32, device=device)
    flag = torch.zeros((1,), dtype=torch.int32, device=device)
    _lib.check(lib.qrlsh_edge_overlaps(_ptr(off), _ptr(r), nq, _ptr(s), _ptr(d), n, _ptr(out), _ptr(flag), _stream()))
    if n and int(flag.item()) & 1:
        raise ValueError("an edge end is outside [0, %d)" % nq)
    return out


def list_fidelity(offsets, rows, D, q_src, q_dst, q_milli, nq, K, queries=None, slices=0, device="cuda"):
    """Hold the stored lists of chosen queries to the exact Jaccard over all nq queries -> ListFidelity (one read-back).
    offsets (nq + 1,) / rows: the CSR answer sets over D table rows (row ids in [0, D), ascending per query); q_src /
    q_dst / q_milli: the query lists in COO form sorted by source, as diversify takes them (the stored order is the order
    that is judged; the values are not read); K in 1..64: the first min(len, K) entries of a row are scored -- a prefix is
    the list a run with that K would have stored; queries: ids of the chosen queries (any order, repeats allowed; a host
    sequence or a device tensor), None = all; slices: 0 = automatic, else 1..256 slices of the ids (the result depends on
    neither).  Tensors are used where they are, host data is uploaded.
    Raises ValueError before anything is uploaded for a bad K, nq, D (at most 2^20), slices or shape and a host query id
    outside [0, nq); through the library's flags for a list row longer than 64, a neighbour index or a device query id
    outside [0, nq) and an answer-set row id outside [0, D) (nothing is returned then)."""
    K = _int_in(K, "K", 1, MAX_K)
    nq = _int_in(nq, "nq", 0, 2**31 - 1)
    D = _int_in(D, "D", 0, MAX_D)
    slices = _int_in(slices, "slices", 0, 256)
    off, r = answer_csr(offsets, rows)
    if off.numel() != nq + 1:
        raise ValueError("offsets holds %d entries, nq + 1 = %d" % (off.numel(), nq + 1))
    coo = coo_triple(q_src, q_dst, q_milli)
    m, chosen, vouched = select_ids(queries, nq, "query", "queries", host_tensors=True)
    lib = _lib.load()
    off = off.to(device=device, dtype=torch.int64).contiguous()
    r = r.to(device=device, dtype=torch.int32).contiguous()
    q_off, q_idx, _ = lists_csr(coo, nq, device)
    G = max(1, int(lib.qrlsh_list_fidelity_group(D)))
    blk, ids = request_blocks(m, lambda blk: blk * _REQUEST_BYTES, WORKSPACE_BUDGET,
                              ids=None if chosen is None else ids32(chosen, nq, device), full=nq, device=device,
                              group=G, cap=MAX_REQUESTS)
    parts = blocks(m, blk)
    # one buffer, one read-back: [words m x 8][totals 8][one flag slot per call] int64, then the four entry arrays int32
    head = m * 8 + 8 + len(parts)
    back = torch.zeros((head + 4 * m * (MAX_K // 2),), dtype=torch.int64, device=device)
    ent = back[head:].view(torch.int32).view(4, m, MAX_K)
    st = _stream()
    for b, i0, i1 in parts:
        _lib.check(lib.qrlsh_list_fidelity(_ptr(off), _ptr(r), nq, D, _ptr(q_off), _ptr(q_idx),
                                           None if ids is None else _ptr(ids[i0:i1]), i1 - i0, K, slices,
                                           _ptr(ent[0, i0:i1]), _ptr(ent[1, i0:i1]), _ptr(ent[2, i0:i1]),
                                           _ptr(ent[3, i0:i1]), _ptr(back[i0 * 8:i1 * 8]), _ptr(back[m * 8:]),
                                           _ptr(back[m * 8 + 8 + b:]), st))
    host = back.cpu().numpy()
    raise_flags(or_flags(host[m * 8 + 8:head]), _FLAG_TEXT, nq=nq, D=D)
    e = host[head:].view(np.int32).reshape(4, m, MAX_K)
    if chosen is None:
        chosen = np.arange(m, dtype=np.int64)
    elif vouched:   # device ids: the flags have vouched for them
        chosen = ids.cpu().numpy().astype(np.int64)
    return ListFidelity(K, chosen, host[:m * 8].reshape(m, 8).copy(), host[m * 8:m * 8 + 8].copy(),
                        {"inter": e[0].copy(), "union": e[1].copy(), "better": e[2].copy(), "equal": e[3].copy()})
