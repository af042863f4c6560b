"""The probe contract of qrlsh.QueryIndex restated in numpy (test infrastructure only), and the hold-out cases built
from the golden fixtures.

A new query x gets as candidates the indexed ids that share with it a band whose r values are equal after the int16
cast and not all -1 (lsh.py:28-49); each once.  Its score is milli = rint(1000 * dot / (sqrt(na) * sqrt(nb))) (the
C oracle's and qrlsh_score_pairs' expression); its list the K best by milli descending, then id ascending."""
import numpy as np

from helpers import FULL, PIECES, load

HOLDOUT_SETS = FULL + PIECES + ["lsh_edge"]


def low16(sig):
    return np.asarray(sig).astype(np.int64) & 0xFFFF


def restate_candidates(index_sig, b, x):
    """ascending indexed ids that share a non-empty band with signature x"""
    n, P = index_sig.shape
    r = P // b
    I = low16(index_sig).reshape(n, b, r)
    X = low16(x).reshape(b, r)
    live = ~(X == 0xFFFF).all(axis=1)
    return np.nonzero(((I == X[None]).all(axis=2) & live[None]).any(axis=1))[0]


def restate_scores(index_sig, ids, x):
    a = np.asarray(index_sig, dtype=np.int64)[ids]
    xv = np.asarray(x, dtype=np.int64)
    dot = a @ xv
    na = (a * a).sum(axis=1)
    nb = int((xv * xv).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        cs = dot.astype(np.float64) / (np.sqrt(na.astype(np.float64)) * np.sqrt(np.float64(nb)))
    cs = np.where((na == 0) | (nb == 0), 0.0, cs)
    return np.rint(cs * 1000.0).astype(np.int64)


def restate_probe(index_sig, b, xs, K):
    """-> list of (ids int64, milli int64, avail) per new signature"""
    out = []
    for x in np.atleast_2d(xs):
        ids = restate_candidates(index_sig, b, x)
        mi = restate_scores(index_sig, ids, x)
        order = np.lexsort((ids, -mi))[:K]
        out.append((ids[order], mi[order], len(ids)))
    return out


def holdout_queries(sig, pairs):
    """first, last, the query with the most candidates, and one without candidates (when there is one)"""
    n = sig.shape[0]
    deg = np.zeros(n, dtype=np.int64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    np.add.at(deg, p[:, 0], 1)
    np.add.at(deg, p[:, 1], 1)
    hs = [0, n - 1, int(np.argmax(deg))]
    lonely = np.nonzero(deg == 0)[0]
    if len(lonely):
        hs.append(int(lonely[0]))
    return sorted(set(hs))


def holdout(sig, h):
    """(index signatures without row h, signature of h, id remap old -> new for the others)"""
    keep = np.arange(sig.shape[0]) != h
    remap = np.cumsum(keep) - 1
    return sig[keep], sig[h], remap


def golden_candidates(pairs, h, remap):
    """the golden candidates of query h as index ids (ascending)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    other = np.concatenate((p[p[:, 0] == h, 1], p[p[:, 1] == h, 0]))
    return np.sort(remap[other])


def golden_list(g, h, remap):
    """(ids, values) of the reference's own top-K list of h, ids remapped; None when h has no list"""
    qs = [int(q) for q in g["qs_q"]]
    if h not in qs:
        return None
    n = qs.index(h)
    lo, hi = int(g["qs_off"][n]), int(g["qs_off"][n + 1])
    return remap[np.asarray(g["qs_idx"][lo:hi], dtype=np.int64)], np.asarray(g["qs_val"][lo:hi])


def check_list_tie_aware(ids, milli, ref_ids, ref_vals):
    """same value sequence, every reference neighbour present with its value unless tied at the cut"""
    mv = np.asarray(milli, dtype=np.float64) / 1000.0
    assert np.array_equal(mv, np.asarray(ref_vals)), (mv, ref_vals)
    cut = ref_vals[-1] if len(ref_vals) else None
    mine = dict(zip(np.asarray(ids).tolist(), mv.tolist()))
    for j, v in zip(np.asarray(ref_ids).tolist(), np.asarray(ref_vals).tolist()):
        if v > cut:
            assert mine.get(j) == v, (j, v)


def golden_sets():
    """(name, g, sig int32, b, K) of every hold-out fixture"""
    for name in HOLDOUT_SETS:
        g = load(name)
        sig = (np.asarray(g["sig"]).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        K = int(g["K"]) if "K" in g else 16
        yield name, g, sig, int(g["b"]), K
