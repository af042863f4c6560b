"""Reference and case builders for the answer sets (csrc/answers.hip, qrlsh/answers.py).  Shared by
tests/test_answers_host.py (no GPU) and tests/test_gpu_answers.py.  Pure numpy.

The kernel ANDs one bitmap row per constrained feature over the D table rows, 32 rows to a word.  A lane takes one
word per step (2048 rows per wave step) or, when words_per_row % 4 == 0, four consecutive words (a lane's 128 rows,
8192 rows per wave step).  The one-sweep form parks the first 64 row ids of a query (SLOT).  The planted tables below
put values into EXACTLY k rows at chosen places, so that answer-set sizes and positions are exact, not left to chance.
"""
import numpy as np

SLOT = 64
PLANT_SIZES = (64, 65, 63, 1)
D_EDGES = (1, 31, 32, 33, 2047, 2048, 2049, 8065, 8191, 8192, 8193,
           8320)      # the last: words_per_row = 260, two wave steps at 16-byte loads
NFEATS = (1, 2, 63, 64)
NQS = (1, 3, 4, 5, 131)
ABSENT = ("0-before-every-value", "c-between-the-values", "zz-after-every-value")


def words_per_row(D):
    return (D + 31) // 32


def step_rows(D):
    """table rows one wave step covers: 16-byte loads need words_per_row % 4 == 0"""
    return 8192 if words_per_row(D) % 4 == 0 else 2048


# ---------------------------------------------------------------------------- reference
def ref_answer_sets(columns, queries):
    """per query the AND of (column == value) over its constrained features ("" = unconstrained), the indices of the
    surviving rows ascending.  -> CSR (offsets int64, rows int32)"""
    columns = [np.asarray(c, dtype=object) for c in columns]
    D = len(columns[0])
    sets = []
    for q in queries:
        mask = np.ones(D, dtype=bool)
        for f, value in enumerate(q):
            if value != "":
                mask &= np.asarray(columns[f] == value, dtype=bool)
        sets.append(np.flatnonzero(mask).astype(np.int32))
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in sets])
    rows = np.concatenate(sets + [np.zeros(0, np.int32)]).astype(np.int32)
    return offsets, rows


# ---------------------------------------------------------------------------- planted tables
def plants_for(D, variant=0):
    """[(value, k, first row)]: disjoint runs of k consecutive rows for the first column.  The places: the first rows,
    the last rows, across the last wave-step boundary below D (both load widths), across a lane's four words (row 128)
    and across a second step boundary; the sizes 64, 65, 63 and 1 rotate through the places with `variant`.  A size
    that found no place is put into the first gap that holds it, so every size that fits D occurs."""
    steps = [B for B in (8192, 6144, 4096, 2048) if B < D]
    places = [("head", lambda k: 0)]
    if steps:       # (before the tail: when D lies just past the boundary, this run is the one that ends at the last row)
        places.append(("step%d" % steps[0], lambda k, B=steps[0]: min(B - k // 2, D - k)))
    places.append(("tail", lambda k: D - k))
    places.append(("lane128", lambda k: 128 - k // 2))
    if len(steps) > 1:
        places.append(("step%d" % steps[-1], lambda k, B=steps[-1]: B - k // 2))
    taken = np.zeros(D, dtype=bool)
    out = []

    def put(name, k, start):
        if start < 0 or start + k > D or taken[start:start + k].any():
            return False
        taken[start:start + k] = True
        out.append(("k%d-%s" % (k, name), k, start))
        return True

    for i, (name, where) in enumerate(places):
        # the single row goes to the first or the last rows only: it cannot lie across a boundary
        k = PLANT_SIZES[(i + variant) % 4] if name in ("head", "tail") else PLANT_SIZES[(i + variant) % 3]
        put(name, k, where(k))
    for k in PLANT_SIZES:
        if not any(kk == k for _, kk, _ in out):
            for start in range(0, D - k + 1):
                if put("gap", k, start):
                    break
    return out


def planted_columns(D, nfeat, variant=0):
    """-> (columns, plants).  Column 0: the planted values of plants_for over a background of three common values.
    Last column (nfeat >= 2): one value in all D rows (a CONSTRAINED query of size D; with nfeat = 64 it is the last
    lane's bitmap row).  Column 1 (nfeat >= 3): the parity of the row.  The others: a few values in runs."""
    plants = plants_for(D, variant)
    rows = np.arange(D)
    col0 = np.array(["bg%d" % (d * 7 % 3) for d in rows], dtype=object)
    for value, k, start in plants:
        col0[start:start + k] = value
    columns = [col0]
    for f in range(1, nfeat):
        if f == nfeat - 1:
            columns.append(np.array(["all"] * D, dtype=object))
        elif f == 1:
            columns.append(np.array(["even" if d % 2 == 0 else "odd" for d in rows], dtype=object))
        else:
            columns.append(np.array(["m%d" % ((d // (f + 1)) % 3) for d in rows], dtype=object))
    return columns, plants


def query_pool(D, nfeat, plants, n=131):
    """n queries cycling through: each planted value alone; with the last column's all-rows value; with the parity
    column; an absent value (alone: the empty set between non-empty neighbours); a planted value AND an absent one;
    the unconstrained query; the all-rows value alone; a background value.  -> object array [n][nfeat]"""
    kinds = []
    for value, _, _ in plants:
        kinds.append({0: value})
        if nfeat >= 2:
            kinds.append({0: value, nfeat - 1: "all"})
        if nfeat >= 3:
            kinds.append({0: value, 1: "odd"})
        kinds.append({0: ABSENT[len(kinds) % 3]})
    kinds.append({})
    kinds.append({0: "bg1"})
    if nfeat >= 2:
        kinds.append({nfeat - 1: "all"})
        kinds.append({0: plants[0][0] if plants else "bg0", nfeat - 1: ABSENT[2]})
        kinds.append({0: "bg2", nfeat - 1: "all"})
    if nfeat >= 4:
        kinds.append({1: "even", 2: "m0", nfeat - 2: "m1"})
    q = np.full((n, nfeat), "", dtype=object)
    for i in range(n):
        for f, value in kinds[i % len(kinds)].items():
            q[i, f] = value
    return q


def sizes_of(offsets):
    return np.diff(np.asarray(offsets))


def route_batches(queries, sizes):
    """-> (compact, refill): the queries whose sets hold at most SLOT rows (the one-sweep form's compact route; their
    largest is exactly SLOT when D allows), and the same batch with ONE set of SLOT + 1 rows in its middle (the refill
    route), or None when no set of that size exists"""
    small = np.flatnonzero(sizes <= SLOT)
    compact = queries[small]
    big = np.flatnonzero(sizes == SLOT + 1)
    if len(big) == 0:
        return compact, None
    mid = len(small) // 2
    return compact, np.concatenate([compact[:mid], queries[big[:1]], compact[mid:]])
