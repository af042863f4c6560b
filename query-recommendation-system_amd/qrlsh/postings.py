"""The postings of the answer sets (qrlsh_answer_postings) and the exact neighbour lists served from them
(qrlsh_exact_neighbours_postings): the second, opt-in route of exact_neighbours().

The postings are the transpose of the CSR answer sets: row d of the table -> the queries whose answer set holds d,
ascending.  A request reads the posting lists of its own rows, so its cost follows its matches instead of a sweep over all
queries; the result is word for word that of the sweep route.  Built on the device on demand and never kept current:
an AnswerPostings carries the shape it was built from, and a call refuses one whose shape is not the CSR's.

A stale index of the SAME shape (nq, entries and D unchanged: two queries of equal size swapped, a replace_queries whose new
sets have the same total size) passes that check, and the library's flag bit 4 ("do not belong") sees only bounds and
ids out of range: such postings are NOT refused, neither for a request whose own answer set changed nor for one whose
neighbours' sets changed.  The result then has intersections from the old lists and unions from the new offsets, and no
flag.  Postings held across any change of the answer sets are the caller's responsibility."""
import torch

from . import _lib
from . import ops
from ._args import _int_in
from ._inputs import MAX_REQUESTS, WORKSPACE_BUDGET, answer_csr, blocks, or_flags, raise_flags, request_blocks
from .ops import _ptr, _stream

MAX_D = _lib.FIDELITY_MAX_D

_FLAG_TEXT = ((4, "a chosen query is outside [0, %(nq)d)"),
              (8, "an answer-set row id is outside [0, %(D)d)"),
              (16, "the postings do not belong to these answer sets"),
              (32, "offsets is not a CSR over the %(nnz)d rows given"))


class AnswerPostings:
    """The result of answer_postings() / Recommender.answer_postings(); device tensors.
    p_off int64 (D + 1,), p_qry int32 (nnz,): the queries of table row d are p_qry[p_off[d]:p_off[d + 1]], ascending.
    D, nq, nnz: the shape of the answer sets they were built from."""

    def __init__(self, p_off, p_qry, D, nq, nnz):
        self.p_off, self.p_qry = p_off, p_qry
        self.D, self.nq, self.nnz = int(D), int(nq), int(nnz)

    def __repr__(self):
        return "AnswerPostings(D=%d, nq=%d, nnz=%d)" % (self.D, self.nq, self.nnz)


def answer_postings(offsets, rows, D, device="cuda"):
    """The row -> queries index of the CSR answer sets -> AnswerPostings (one read-back, for the flags).
    offsets (nq + 1,) / rows: the answer sets over D table rows, as exact_neighbours takes them.  Tensors are used where
    they are, host data is uploaded.
    Raises ValueError before the library is loaded for a bad D (at most 2^20) or shape; through the library's flags for a
    row id outside [0, D) and for offsets that are no CSR over rows (nothing is returned then)."""
    D = _int_in(D, "D", 0, MAX_D)
    off, r = answer_csr(offsets, rows)
    nq, nnz = int(off.numel()) - 1, int(r.numel())
    if nnz >= 2**32:
        raise ValueError("at most 2^32 - 1 answer-set entries")
    lib = _lib.load()
    off = off.to(device=device, dtype=torch.int64).contiguous()
    r = r.to(device=device, dtype=torch.int32).contiguous()
    p_off = torch.empty((D + 1,), dtype=torch.int64, device=device)
    p_qry = torch.empty((nnz,), dtype=torch.int32, device=device)
    flags = torch.zeros((1,), dtype=torch.int32, device=device)
    need = int(lib.qrlsh_answer_postings_scratch_bytes(nnz, D))
    scratch = ops._ws(need, device)
    _lib.check(lib.qrlsh_answer_postings(_ptr(off), _ptr(r), nq, nnz, D, _ptr(p_off), _ptr(p_qry), _ptr(flags),
                                         _ptr(scratch), need, _stream()))
    raise_flags(or_flags(flags.cpu()), _FLAG_TEXT, nq=nq, D=D, nnz=nnz)
    return AnswerPostings(p_off, p_qry, D, nq, nnz)


def check_postings(postings, nq, nnz, D, slices=0):
    """the checks of exact_neighbours(postings=...) that need no device: the type, slices, and the shape the postings were
    built from against the CSR's"""
    if not isinstance(postings, AnswerPostings):
        raise ValueError("postings must be an AnswerPostings (answer_postings()), got %r" % type(postings).__name__)
    if slices != 0:
        raise ValueError("slices belongs to the sweep: leave it 0 with postings")
    if (postings.nq, postings.nnz, postings.D) != (nq, nnz, D):
        raise ValueError("the postings were built from %d queries, %d entries, %d rows; the answer sets hold %d, %d, %d"
                         % (postings.nq, postings.nnz, postings.D, nq, nnz, D))
    if int(postings.p_off.numel()) != D + 1 or int(postings.p_qry.numel()) != nnz:
        raise ValueError("postings of shape (%d,), (%d,): (%d,), (%d,) expected"
                         % (int(postings.p_off.numel()), int(postings.p_qry.numel()), D + 1, nnz))


def exact_lists(off, r, nq, D, K, ids, m, postings, device):
    """exact_neighbours' device work over the postings: off / r / ids already on the device -> (dst, inter, union,
    counts), after the one read-back (the flags).  Requests run in blocks under WORKSPACE_BUDGET / MAX_REQUESTS."""
    lib = _lib.load()
    p_off = postings.p_off.to(device=device, dtype=torch.int64).contiguous()
    p_qry = postings.p_qry.to(device=device, dtype=torch.int32).contiguous()
    dst = torch.full((m, K), -1, dtype=torch.int32, device=device)       # the library writes nothing when nq is 0
    inter = torch.zeros((2, m, K), dtype=torch.int32, device=device)
    counts = torch.zeros((m, 2), dtype=torch.int32, device=device)

    def scratch_bytes(n):
        return int(lib.qrlsh_exact_postings_scratch_bytes(nq, n, K))

    def call_bytes(n):   # the scratch is 0 today: a block is held to the budget by what it writes, (3 K + 2) words a request
        return scratch_bytes(n) + n * (3 * K + 2) * 4
    blk, _ = request_blocks(m, call_bytes, WORKSPACE_BUDGET, cap=MAX_REQUESTS)
    parts = blocks(m, blk)
    flags = torch.zeros((max(len(parts), 1),), dtype=torch.int32, device=device)
    scratch = ops._ws(max(scratch_bytes(i1 - i0) for _, i0, i1 in parts), device) if m else None
    st = _stream()
    for b, i0, i1 in parts:
        _lib.check(lib.qrlsh_exact_neighbours_postings(_ptr(off), _ptr(r), nq, D, _ptr(p_off), _ptr(p_qry),
                                                       _ptr(ids[i0:i1]), i1 - i0, K, _ptr(dst[i0:i1]),
                                                       _ptr(inter[0, i0:i1]), _ptr(inter[1, i0:i1]), _ptr(counts[i0:i1]),
                                                       _ptr(flags[b:]), _ptr(scratch), scratch_bytes(i1 - i0), st))
    raise_flags(or_flags(flags.cpu()), _FLAG_TEXT, nq=nq, D=D, nnz=int(r.numel()))
    return dst, inter[0], inter[1], counts
