"""The layout contract of qrlsh.QueryIndex's band arrays restated in numpy (test infrastructure only), and the claim
qrlsh_index_append rests on.

A built index holds, per band, the (key, id) records sorted stably by the top 32 bits of mix64(key) -- ids ascending
among equal bits -- and a directory over the top d bits: dir[t][h] = first position of band t whose bits are >= h,
h = 0 .. 2^d, with d = ceil(log2 n) - 3 clamped to 1 .. 26 (qrlsh_index_dir_bits).

Appended queries get ids above every indexed id, so the grown index is the stable merge of the old band and the sorted
batch with the old records first among equal bits: restate_merge writes that merge down through positions
q_j = (old records with bits <= the batch record's) + j, the form the device uses."""
import numpy as np

from bucket_cases import np_mix64


def dir_bits(n):
    lg = 0
    while lg < 62 and (1 << lg) < n:
        lg += 1
    return min(max(lg - 3, 1), 26)


def np_band_keys(sig, b):
    """band keys [b][n] uint64 of a signature matrix, as qr_make_key (csrc/common.h): r <= 4 the packed low-16 values,
    r > 4 a 64-bit hash of them; the all -1 band maps to ~0 (r >= 4) or 2^(16 r) - 1"""
    s = (np.asarray(sig).astype(np.int64) & 0xFFFF).astype(np.uint64)
    n, P = s.shape
    r = P // b
    s = s.reshape(n, b, r)
    with np.errstate(over="ignore"):
        if r <= 4:
            k = np.zeros((n, b), dtype=np.uint64)
            for j in range(r):
                k |= s[:, :, j] << np.uint64(16 * j)
            return np.ascontiguousarray(k.T)
        h = np.full((n, b), 0x243F6A8885A308D3, dtype=np.uint64)
        for j in range(r):
            h = (h ^ s[:, :, j]) * np.uint64(0x9E3779B97F4A7C15)
            h ^= h >> np.uint64(29)
        h = np_mix64(h)
        full = np.uint64(0xFFFFFFFFFFFFFFFF)
        h = np.where(h == full, h - np.uint64(1), h)
        h = np.where((s == 0xFFFF).all(axis=2), full, h)
    return np.ascontiguousarray(h.T)


def _directory(sorted_keys, d):
    h = (np_mix64(sorted_keys) >> np.uint64(64 - d)).astype(np.int64)
    return np.searchsorted(h, np.arange((1 << d) + 1), side="left").astype(np.uint32)


def restate_layout(keys):
    """keys [b][n] (uint64, or int64 bit patterns) -> (sorted keys uint64 [b][n], ids uint32 [b][n],
    directory uint32 [b * (2^d + 1)])"""
    keys = np.ascontiguousarray(keys).view(np.uint64)
    b, n = keys.shape
    d = dir_bits(n)
    sk = np.empty((b, n), dtype=np.uint64)
    ids = np.empty((b, n), dtype=np.uint32)
    dirw = np.empty((b, (1 << d) + 1), dtype=np.uint32)
    for t in range(b):
        order = np.argsort(np_mix64(keys[t]) >> np.uint64(32), kind="stable")
        sk[t], ids[t] = keys[t][order], order
        dirw[t] = _directory(sk[t], d)
    return sk, ids, dirw.reshape(-1)


def restate_merge(old, batch):
    """stable merge, old first on ties, of two layouts (restate_layout's triples) of the same band count; the batch's
    ids are offset by the old n.  -> the merged triple"""
    ok, oi, _ = old
    bk, bi, _ = batch
    b, n = ok.shape
    m = bk.shape[1]
    N = n + m
    d = dir_bits(N)
    sk = np.empty((b, N), dtype=np.uint64)
    ids = np.empty((b, N), dtype=np.uint32)
    dirw = np.empty((b, (1 << d) + 1), dtype=np.uint32)
    for t in range(b):
        otop = np_mix64(ok[t]) >> np.uint64(32)
        btop = np_mix64(bk[t]) >> np.uint64(32)
        q = np.searchsorted(otop, btop, side="right") + np.arange(m)      # strictly increasing
        new = np.zeros(N, dtype=bool)
        new[q] = True
        sk[t][new], ids[t][new] = bk[t], bi[t].astype(np.int64) + n
        sk[t][~new], ids[t][~new] = ok[t], oi[t]
        dirw[t] = _directory(sk[t], d)
    return sk, ids, dirw.reshape(-1)


def device_restate_probe(index_sig, b, x, K):
    """restate_probe for ONE probe row over a large index held on the device: the candidates by band equality in
    torch, scores and order in numpy (query_index_cases.restate_scores).  index_sig: int32 [n, P] device tensor;
    x: int32 [P] device tensor.  -> (ids int64, milli int64, avail)"""
    import torch
    import query_index_cases as QC
    n, P = index_sig.shape
    r = P // b
    I16 = index_sig.bitwise_and(0xFFFF).view(n, b, r)
    X = x.bitwise_and(0xFFFF).view(b, r)
    live = ~(X == 0xFFFF).all(dim=1)
    ids = torch.nonzero(((I16 == X[None]).all(dim=2) & live[None]).any(dim=1)).flatten()
    rows = index_sig[ids].cpu().numpy()
    ids = ids.cpu().numpy()
    mi = QC.restate_scores(rows, np.arange(len(ids)), x.cpu().numpy())
    order = np.lexsort((ids, -mi))[:K]
    return ids[order].astype(np.int64), mi[order], len(ids)
