"""Numpy references, inputs and checkers for the user-similarity step (csrc/users.hip, qrlsh/users.py): the column
statistics of StandardScaler, the Gram matrix of the standardized ratings, the PCA features, and the pairs, scores and
lists of the clusters under every kind of label.  Used by tests/test_users_host.py (the references against
scikit-learn, the oracle and planted defects, no GPU) and tests/test_gpu_users.py (the kernels against the references).
Nothing here imports the library."""
import functools
import math

import numpy as np

EPS = 2.220446049250313e-16      # float64 machine epsilon, as scikit-learn's rules use it
U = 2.0 ** -53                   # float64 unit roundoff

# the Gram kernel's own sizes (users.hip): tile side, columns per step, the slice thresholds
GR_T, GR_K = 128, 32


def slices_of(nq):
    return 16 if nq >= 65536 else 4 if nq >= 4096 else 1


def slice_cols_of(nq):
    per_slice = -(-nq // slices_of(nq))
    return -(-per_slice // GR_K) * GR_K


# --------------------------------------------------------------------------------------------- 1. column statistics
def stats_ref(r):
    """(mean, scale) float64 [nq] of an integer matrix [nu][nq] as StandardScaler().fit gives them, restated:
    T = sum / n with the rows added in order, d = x - T, var = (sum d^2 - (sum d)^2 / n) / n; a column is constant
    when var <= n eps var + (n T eps)^2 and keeps scale 1; a scale below 10 eps becomes 1 too"""
    x = np.asarray(r).astype(np.float64)
    nu, nq = x.shape
    n = float(nu)
    s = np.zeros(nq)
    for row in x:
        s = s + row
    T = s / n
    corr, ss = np.zeros(nq), np.zeros(nq)
    for row in x:
        d = row - T
        corr = corr + d
        ss = ss + d * d
    var = (ss - corr * corr / n) / n
    ub = n * EPS * var + (n * T * EPS) * (n * T * EPS)
    scale = np.where(var <= ub, 1.0, np.sqrt(var))
    scale[scale < 10.0 * EPS] = 1.0
    return T, scale


def planted_columns(nq):
    """the columns that hold the four planted patterns (all 7, all 0, a single non-zero entry, alternating 0 / 100);
    none in a matrix of fewer than four columns"""
    return tuple(k * nq // 5 for k in (1, 2, 3, 4)) if nq >= 4 else ()


def ratings_matrix(nu, nq, big=False):
    """integers 0..100 at about 40 % fill with the planted columns; big: values up to 10^6 and a few negative ones
    (legal int32 input outside the reference's domain)"""
    rng = np.random.default_rng(100_003 * nu + nq + (7 if big else 0))
    r = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < 0.4)).astype(np.int32)
    if big:
        r = r * rng.integers(1, 10_001, size=(nu, nq)).astype(np.int32)
        neg = rng.random((nu, nq)) < 0.002
        r[neg] = -r[neg] - 3
    cols = planted_columns(nq)
    if cols:
        r[:, cols[0]] = 7
        r[:, cols[1]] = 0
        r[:, cols[2]] = 0
        r[nu // 2, cols[2]] = 83
        r[:, cols[3]] = (np.arange(nu) % 2) * 100
    return r


# every nq at nu = 129, every nu at nq = 33 and 4097, 257 x 65 537 once, and one matrix of large and negative values
GRAM_NU = (1, 2, 127, 128, 129, 257)
GRAM_NQ = (1, 31, 32, 33, 4095, 4096, 4097, 65535, 65536, 65537)
GRAM_SHAPES = sorted({(129, nq) for nq in GRAM_NQ} | {(nu, nq) for nu in GRAM_NU for nq in (33, 4097)} | {(257, 65537)})
GRAM_CASES = [(nu, nq, False) for nu, nq in GRAM_SHAPES] + [(129, 4097, True)]


def case_id(c):
    return "%dx%d%s" % (c[0], c[1], "-big" if c[2] else "")


@functools.lru_cache(maxsize=None)
def gram_case(nu, nq, big=False):
    """-> (ratings int32 [nu][nq], (mean, scale) of stats_ref); built once, not to be written"""
    r = ratings_matrix(nu, nq, big)
    r.setflags(write=False)
    return r, stats_ref(r)


def check_stats(mean, inv_scale, ref):
    """the device's statistics against stats_ref: the mean exactly, 1 / inv_scale within rtol = 1e-15"""
    mean, inv_scale = np.asarray(mean), np.asarray(inv_scale)
    assert mean.shape == ref[0].shape and inv_scale.shape == ref[1].shape
    assert np.array_equal(mean, ref[0]), "mean differs in columns %s" % np.flatnonzero(mean != ref[0])[:8].tolist()
    ok = np.isclose(1.0 / inv_scale, ref[1], rtol=1e-15, atol=0)
    assert ok.all(), "scale differs in columns %s" % np.flatnonzero(~ok)[:8].tolist()


# ------------------------------------------------------------------------------------------------------ 2. the Gram
def standardized(r, mean, inv_scale):
    """z = (float64(x) - mean) * inv: the kernel's own two roundings (no fused operation exists in this expression)"""
    return (np.asarray(r).astype(np.float64) - mean) * inv_scale


def sampled_rows(nu):
    return sorted({i for i in (0, 1, 63, 64, 127, 128, nu - 1) if 0 <= i < nu})


def gram_gamma(nq):
    """g = n u / (1 - n u), n = nq + 16: the terms of an entry plus the sum over at most 16 slices.  For ANY order of
    the additions, fused or not, |G_dev[i][j] - G_exact[i][j]| <= g * sum_c |z_ic| |z_jc|"""
    n = nq + 16
    return n * U / (1.0 - n * U)


def _longdouble_rows(z, rows, step=8192):
    zr = z[rows].astype(np.longdouble)
    acc = np.zeros((len(rows), z.shape[0]), dtype=np.longdouble)
    for c in range(0, z.shape[1], step):
        acc += zr[:, c:c + step] @ z[:, c:c + step].astype(np.longdouble).T
    return acc


def check_gram(gram, z):
    """gram [nu][nu] against the standardized matrix z [nu][nq]: exactly symmetric; every entry within 2 g S of
    numpy's float64 product (which carries the bound g S itself), the sampled rows within g S of a longdouble product,
    S = sum_c |z_ic| |z_jc|; exactly 0 where S is 0.  AssertionError otherwise (a NaN never passes).
    -> (largest |G - float64 product| / (2 g S), largest |G - longdouble rows| / (g S))"""
    gram = np.asarray(gram)
    nu, nq = z.shape
    assert gram.shape == (nu, nu) and gram.dtype == np.float64
    assert np.isfinite(gram).all(), "an entry is not finite (unwritten?)"
    assert np.array_equal(gram, gram.T), "not symmetric"
    g = gram_gamma(nq)
    a = np.abs(z)
    S = a @ a.T
    zero = S == 0
    assert (gram[zero] == 0).all(), "a non-zero entry between rows that share no non-zero column"
    Sd = np.where(zero, 1.0, S)
    q64 = np.abs(gram - z @ z.T) / (2.0 * g * Sd)
    rows = sampled_rows(nu)
    qld = (np.abs(gram[rows].astype(np.longdouble) - _longdouble_rows(z, rows)) / (g * Sd[rows])).astype(np.float64)
    worst64, worstld = float(q64.max()), float(qld.max())
    if not (q64 <= 1.0).all():
        i, j = np.unravel_index(np.argmax(q64), q64.shape)
        raise AssertionError("G[%d][%d] is %.3g bounds from the float64 product" % (i, j, worst64))
    if not (qld <= 1.0).all():
        i, j = np.unravel_index(np.argmax(qld), qld.shape)
        raise AssertionError("G[%d][%d] is %.3g bounds from the longdouble product" % (rows[i], j, worstld))
    return worst64, worstld


def gram_by_slices(z):
    """G the way the kernels build it, in numpy: one product per column slice, summed in slice order"""
    nu, nq = z.shape
    sc = slice_cols_of(nq)
    G = np.zeros((nu, nu))
    for c0 in range(0, nq, sc):
        G = G + z[:, c0:c0 + sc] @ z[:, c0:c0 + sc].T
    return np.triu(G) + np.triu(G, 1).T               # one stored orientation, as the reduce kernel reads it


DEFECTS = ("slice 0 loses its last column", "the last slice counts its first column twice",
           "row 128 staged as a rated zero", "tile pair (0, 1) transposed")


def defect_case(kind):
    """-> (z, G with the one defect `kind` of DEFECTS planted into a reference-built G); three at 129 x 4097 (one row in
    the second tile, four slices with a short last one), the transposed tile pair at 257 x 33 (it needs a square block)"""
    nu, nq = (257, 33) if kind == DEFECTS[3] else (129, 4097)
    r, (mean, scale) = gram_case(nu, nq)
    inv = 1.0 / scale
    z = standardized(r, mean, inv)
    G = gram_by_slices(z)
    sc, ns = slice_cols_of(nq), slices_of(nq)
    if kind == DEFECTS[0]:
        c = sc - 1
        assert c not in planted_columns(nq)[:2]
        G = G - np.outer(z[:, c], z[:, c])
    elif kind == DEFECTS[1]:
        c = (ns - 1) * sc
        assert c < nq and nq - c < sc and c not in planted_columns(nq)[:2]      # a short last slice
        G = G + np.outer(z[:, c], z[:, c])
    elif kind == DEFECTS[2]:
        # the load leaves the row out (reads 0 for it) but the staging standardizes it like a row inside the matrix:
        # row 128 enters as (0 - mean) * inv in every column instead of with its ratings
        z2 = z.copy()
        z2[128] = (0.0 - mean) * inv
        G = gram_by_slices(z2)
    else:
        blk = G[0:GR_T, GR_T:2 * GR_T].copy()
        G[0:GR_T, GR_T:2 * GR_T] = blk.T
        G[GR_T:2 * GR_T, 0:GR_T] = blk                   # (stays symmetric: only the values give it away)
    return z, G


# ------------------------------------------------------------------------------------------------- 3. PCA features
PCA_SHAPES = [(2, 5), (50, 7), (129, 33), (300, 250), (250, 4097)]


def pca_reference(r):
    """StandardScaler + PCA(n_components = min(nu, nq, 200), svd_solver="full") -> float64 [nu][k].  The solver is
    named: "auto" takes scikit-learn's randomized solver on the larger shapes, whose own two runs disagree"""
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    x = StandardScaler().fit_transform(np.asarray(r))
    return PCA(n_components=min(x.shape[0], x.shape[1], 200), svd_solver="full").fit(x).transform(x)


def pca_from_gram(r):
    """the Gram route in numpy: eigh of the float64 Gram of the standardized matrix, scores U_k sqrt(lambda_k)"""
    mean, scale = stats_ref(r)
    z = standardized(r, mean, 1.0 / scale)
    nu, nq = z.shape
    k = min(nu, nq, 200)
    lam, vec = np.linalg.eigh(z @ z.T)
    return vec[:, nu - k:][:, ::-1] * np.sqrt(np.maximum(lam[nu - k:][::-1], 0.0))


def distances(f):
    d2 = ((f[:, None, :] - f[None, :, :]) ** 2).sum(axis=2)
    return np.sqrt(d2)


def check_pca(f, r, ref):
    """f: features of the integer matrix r, ref = pca_reference(r): the shape, the columns by descending variance, all
    pairwise distances between users within rtol = 1e-7, atol = 1e-6 (what BIRCH reads; single components of close
    eigenvalues are ill-conditioned and are not compared).  -> the largest distance error"""
    nu, nq = r.shape
    assert f.shape == ref.shape == (nu, min(nu, nq, 200)) and f.dtype == np.float64
    v = f.var(axis=0)
    # eigh returns the eigenvalues ascending to within its backward error, O(nu eps lambda_max) < 1e-13 lambda_max
    # here; 1e-10 of the leading variance is a thousand times that and far below any gap that orders components
    assert (np.diff(v) <= 1e-10 * v[0]).all(), "components are not ordered by descending variance"
    d, dr = distances(f), distances(ref)
    assert np.allclose(d, dr, rtol=1e-7, atol=1e-6), "largest distance error %.3g" % np.abs(d - dr).max()
    return float(np.abs(d - dr).max())


# ------------------------------------------------------------------ 4. cluster pairs, scores and lists by any label
LABEL_NU, LABEL_NQ = 700, 37            # a row stride of 40: three padding columns
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
# label value -> members.  -1 is the bucket machinery's all-ones key; 1000 / 1001 differ only in bit 0, 5 / 5 + 2^62
# only in bit 62; clusters of 1, 2, 17 (K + 1 at 700 users) and 300 users
LABEL_SIZES = ((-1, 40), (I64_MIN, 17), (I64_MAX, 2), (0, 300), (1000, 1), (1001, 60), (5, 100), (5 + 2 ** 62, 180))


@functools.lru_cache(maxsize=None)
def label_case():
    """-> (ratings int64 [700][37], labels int64 [700]); rows 0 / 1 / 2: unrated, a single rating, [1, 2, 2, 0, ...]
    (mean 5/3: truncation toward zero centres it to all zeros, floor would not)"""
    rng = np.random.default_rng(4)
    nu, nq = LABEL_NU, LABEL_NQ
    r = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < 0.4)).astype(np.int64)
    r[0] = 0
    r[1] = 0
    r[1, 20] = 55
    r[2] = 0
    r[2, :3] = (1, 2, 2)
    labels = np.concatenate([np.full(n, v, dtype=np.int64) for v, n in LABEL_SIZES])
    assert labels.size == nu
    labels = labels[rng.permutation(nu)]
    for row, want in ((0, -1), (1, 0), (2, -1)):     # the three special rows sit in clusters that have pairs
        if labels[row] != want:
            j = 3 + int(np.flatnonzero(labels[3:] == want)[0])
            labels[row], labels[j] = labels[j], labels[row]
    r.setflags(write=False)
    return r, labels


def max_candidates(nu):
    return round(math.log(nu, 1.5))


def pairs_ref(labels):
    """every u < v with labels[u] == labels[v] as u << 32 | v, sorted -> int64 [n]"""
    labels = np.asarray(labels)
    out = []
    for lab in np.unique(labels):
        mem = np.flatnonzero(labels == lab).astype(np.int64)
        a, b = np.triu_indices(mem.size, k=1)
        out.append((mem[a] << 32) | mem[b])
    return np.sort(np.concatenate(out)) if out else np.zeros(0, dtype=np.int64)


def centred(ratings):
    """x == 0 ? 0 : trunc(float64(x) - sum / count) over a row's non-zero ratings -> int64"""
    r = np.asarray(ratings).astype(np.int64)
    cnt = (r != 0).sum(axis=1)
    mean = np.where(cnt > 0, r.sum(axis=1).astype(np.float64) / np.maximum(cnt, 1).astype(np.float64), 0.0)
    return np.where(r != 0, np.trunc(r.astype(np.float64) - mean[:, None]), 0.0).astype(np.int64)


def scores_ref(ratings, pairs, product_last=False):
    """milli int32 [n] of pairs: exact integer dot and norms of the truncated centred rows,
    rint(1000 * dot / (sqrt(na) * sqrt(nb))) in float64, 0 where a norm is 0.  product_last: (dot / (...)) * 1000, the
    order the scoring kernel writes -- the host test shows the two agree on the case"""
    c = centred(ratings)
    u, v = pairs >> 32, pairs & 0xFFFFFFFF
    dot = (c[u] * c[v]).sum(axis=1)
    n2 = (c * c).sum(axis=1)
    na, nb = n2[u], n2[v]
    ok = (na != 0) & (nb != 0)
    den = np.where(ok, np.sqrt(na.astype(np.float64)) * np.sqrt(nb.astype(np.float64)), 1.0)
    cs = (dot.astype(np.float64) / den) * 1000.0 if product_last else (1000.0 * dot.astype(np.float64)) / den
    return np.where(ok, np.rint(cs), 0.0).astype(np.int32)


def lists_ref(ratings, labels, K):
    """dense lists (idx int32 [nu][K], -1 past the end; milli int32 [nu][K], 0 past the end; len int32 [nu]): per user
    the positive scores of its cluster by value descending, then id ascending, cut at K"""
    nu = np.asarray(ratings).shape[0]
    pairs = pairs_ref(labels)
    m = scores_ref(ratings, pairs)
    u, v = pairs >> 32, pairs & 0xFFFFFFFF
    src, dst, val = np.concatenate((u, v)), np.concatenate((v, u)), np.concatenate((m, m)).astype(np.int64)
    keep = val > 0
    src, dst, val = src[keep], dst[keep], val[keep]
    order = np.lexsort((dst, -val, src))
    src, dst, val = src[order], dst[order], val[order]
    idx = np.full((nu, K), -1, dtype=np.int32)
    mil = np.zeros((nu, K), dtype=np.int32)
    cnt = np.bincount(src, minlength=nu)
    rank = np.arange(src.size) - (np.cumsum(cnt) - cnt)[src]
    cut = rank < K
    idx[src[cut], rank[cut]] = dst[cut]
    mil[src[cut], rank[cut]] = val[cut]
    return idx, mil, np.minimum(cnt, K).astype(np.int32)


def dense_from_coo(src, dst, val, nu, K):
    """(src, dst, val) sorted by user, in list order -> the dense form of lists_ref"""
    src, dst, val = (np.asarray(a).astype(np.int64) for a in (src, dst, val))
    idx = np.full((nu, K), -1, dtype=np.int32)
    mil = np.zeros((nu, K), dtype=np.int32)
    cnt = np.bincount(src, minlength=nu)
    assert cnt.max(initial=0) <= K and (np.diff(src) >= 0).all()
    rank = np.arange(src.size) - (np.cumsum(cnt) - cnt)[src]
    idx[src, rank] = dst
    mil[src, rank] = val
    return idx, mil, cnt.astype(np.int32)


def lists_to_dict(lists):
    """dense lists -> {u: {'indexes', 'values'}}, the oracle's form"""
    idx, mil, ln = lists
    return {u: {"indexes": idx[u, :ln[u]].astype(np.int64), "values": mil[u, :ln[u]].astype(np.float64) / 1000.0}
            for u in range(len(ln))}


def assert_lists(got, want, what):
    for name, g, w in zip(("idx", "milli", "len"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            raise AssertionError("%s: %s differs in rows %s" % (what, name, np.unique(np.argwhere(g != w)[:, 0])[:8].tolist()))


def check_user_sims_tie_aware(mine, ref, K):
    """mine / ref: {u: {'indexes', 'values'}}.  The reference keeps zero-valued entries (the user itself, negative
    cosines) when a cluster has fewer than K positive neighbours and orders ties arbitrarily (np.argsort); the
    device lists hold the positive entries only, ties by ascending id.  Equal means: same positive value
    multiset per user, every device neighbour strictly above the cut-off value is a reference neighbour and
    vice versa."""
    assert sorted(mine.keys()) == sorted(ref.keys())
    for u in ref:
        rv = np.asarray(ref[u]["values"], dtype=np.float64)
        ri = np.asarray(ref[u]["indexes"])
        pos = rv > 0
        mv, mi = np.asarray(mine[u]["values"]), np.asarray(mine[u]["indexes"])
        assert len(mv) <= K and np.all(mv > 0) and np.all(np.diff(mv) <= 0)
        assert np.array_equal(np.sort(mv), np.sort(rv[pos])), u
        if len(mv):
            cut = mv.min()
            assert set(mi[mv > cut].tolist()) == set(ri[pos & (rv > cut)].tolist()), u
        for a, b, x, y in zip(mi[:-1], mi[1:], mv[:-1], mv[1:]):
            assert x > y or a < b


def add_users_case():
    """the label case split for add_users: -> (base ratings, base labels, added rows, added labels): the users
    labelled -1 and 2^63 - 1 leave the matrix and come back as new users, in their old order"""
    r, labels = label_case()
    out = (labels == -1) | (labels == I64_MAX)
    return r[~out], labels[~out], r[out], labels[out]
