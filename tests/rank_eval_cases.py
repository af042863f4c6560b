"""The numpy restatement of the ranking evaluation (qrlsh_evaluate_ranking) and seeded cases for it (test infrastructure
only).  Built on the oracle's predict_cells -- the restated predictions the serving tests use, in either sum order --
never on the code under test.

`train` = the matrix with the test cells zeroed, `truth` = the full one.  A test cell of user u: train[u][j] == 0 and
truth[u][j] != 0; relevant when truth[u][j] >= relevant.  The list of a request: the candidates (train == 0, a non-zero
prediction, and for "heldout" a test cell) in a stable sort by (-value, column), cut at k.  Per request 8 int64 words:
listed, hits, known, 1-based rank of the first hit (0 = none), dcg, relevant test cells, test cells, avail; totals: 16
words, 0-7 their sums, 8 requests, 9 requests with a relevant test cell, 10 requests with a hit, 11 the ideal DCG."""
import numpy as np

from oracle import oracle as O
import evaluate_cases as EC

NOBODY = {"indexes": np.zeros(0, dtype=np.int64), "values": np.zeros(0)}


def dcg_gains_ref(k):
    """round(2^32 / log2(p + 2)), p = 0 .. k - 1, as Python integers"""
    import math
    return [round(2.0**32 / math.log2(p + 2)) for p in range(k)]


def candidate_predictions(train, qs, us, users, summation=O.np_sum_order, only=None):
    """int64 [m][nq]: the restated prediction at every unrated cell of `train` in the row of each request's user (those
    where `only` [nu][nq] is set, when given), 0 elsewhere.  The expensive part of the reference: computed once per case
    and sum order and handed to rank_eval_ref as `pred`."""
    train = np.asarray(train)
    nu, nq = train.shape
    rows = np.arange(nu) if users is None else np.asarray(users, dtype=np.int64)
    every = {u: us.get(u, NOBODY) for u in range(nu)}
    done = {}
    out = np.zeros((len(rows), nq), dtype=np.int64)
    for x, u in enumerate(rows.tolist()):
        if u not in done:
            want = train[u] == 0
            if only is not None:
                want &= np.asarray(only)[u]
            cols = np.nonzero(want)[0]
            line = np.zeros(nq, dtype=np.int64)
            if len(cols):
                cells = np.stack([np.full(len(cols), u), cols], axis=1)
                line[cols] = O.predict_cells(train, qs, every, cells, summation=summation)
            done[u] = line
        out[x] = done[u]
    return out


def rank_eval_ref(train, truth, qs, us, users, k, relevant, candidates, gains, summation=O.np_sum_order, pred=None):
    """-> (idx int64 [m][k], val int64 [m][k], avail int64 [m], per_user int64 [m][8], totals int64 [16]).
    users: row ids (repeats allowed) or None = every row; gains: k integers; pred: candidate_predictions(...) of the
    same train, lists, users and summation (computed here when not given)."""
    train, truth = np.asarray(train), np.asarray(truth)
    nu, nq = train.shape
    rows = list(range(nu)) if users is None else [int(u) for u in users]
    if pred is None:
        pred = candidate_predictions(train, qs, us, rows, summation)
    gains = [int(g) for g in gains]
    assert len(gains) == k and candidates in ("all", "heldout")
    idx = np.full((len(rows), k), -1, dtype=np.int64)
    val = np.zeros((len(rows), k), dtype=np.int64)
    avail = np.zeros(len(rows), dtype=np.int64)
    per = np.zeros((len(rows), 8), dtype=np.int64)
    totals = [0] * 16
    for x, u in enumerate(rows):
        tr, tt, pr = train[u].tolist(), truth[u].tolist(), pred[x].tolist()
        test = relevant_cells = 0
        cand = []
        for j in range(nq):
            is_test = tr[j] == 0 and tt[j] != 0
            if is_test:
                test += 1
                if tt[j] >= relevant:
                    relevant_cells += 1
            if tr[j] == 0 and pr[j] != 0 and (candidates == "all" or is_test):
                cand.append(j)
        cand.sort(key=lambda j: (-pr[j], j))          # stable: value descending, then column ascending
        shown = cand[:k]
        hits = known = first = dcg = 0
        for p, j in enumerate(shown):
            idx[x, p], val[x, p] = j, pr[j]
            if tt[j] != 0:
                known += 1
            if tt[j] >= relevant:
                hits += 1
                dcg += gains[p]
                if first == 0:
                    first = p + 1
        avail[x] = len(cand)
        line = [len(shown), hits, known, first, dcg, relevant_cells, test, len(cand)]
        per[x] = line
        for w in range(8):
            totals[w] += line[w]
        totals[8] += 1
        totals[9] += 1 if relevant_cells > 0 else 0
        totals[10] += 1 if hits > 0 else 0
        totals[11] += sum(gains[:min(k, relevant_cells)])
    return idx, val, avail, per, np.array(totals, dtype=np.int64)


def macro_ref(per, gains):
    """the macro figures in float64 numpy from the expected per-request words"""
    per = np.asarray(per, dtype=np.int64)
    prefix = np.concatenate(([0], np.cumsum(np.asarray(gains, dtype=np.int64))))
    on = per[:, 5] > 0
    n = int(on.sum())
    if n == 0:
        return {"n": 0}
    p = per[on].astype(np.float64)
    ideal = prefix[np.minimum(per[on][:, 5], len(gains))].astype(np.float64)
    precision = np.where(p[:, 0] > 0, p[:, 1] / np.maximum(p[:, 0], 1), 0.0)
    rr = np.where(p[:, 3] > 0, 1.0 / np.maximum(p[:, 3], 1), 0.0)
    return {"n": n, "precision": precision.sum() / n, "recall": (p[:, 1] / p[:, 5]).sum() / n,
            "ndcg": (p[:, 4] / ideal).sum() / n, "mrr": rr.sum() / n}


# ------------------------------------------------------------------------------------------------------------ cases
def split_case(seed, nu, nq, fill, held, longest_q=6, ku=3):
    """A random hold-out: truth = random ratings 1..100 with `fill` of the cells rated, train = truth with about `held`
    of the rated cells zeroed (numpy's generator: the split rule itself is pinned by the evaluation tests); random lists
    as evaluate_cases.random_case draws them -- all shorter than 8, so both sum orders give the same predictions.
    -> (train, truth, coo, qs, us)"""
    truth, coo, qs, us = EC.random_case(seed, nu, nq, longest_q, ku, fill=fill)
    rng = np.random.default_rng(seed + 1000003)
    gone = (truth != 0) & (rng.random(truth.shape) < held)
    return np.where(gone, 0, truth).astype(np.int32), truth, coo, qs, us


KNIFE_USERS, KNIFE_QUERIES = 3, 24


def knife_split(seed, nu, nq, fill=0.9, held=0.5):
    """A hold-out over predict_cases.build_case, whose knife-edge cells (the first KNIFE_USERS users x KNIFE_QUERIES
    queries, unrated) land on k + 1/2 and move with the sum order: train = its matrix, truth = train plus ratings 1..100
    at about `held` of train's unrated cells -- in the knife users' rows at the knife cells and nowhere else, so that
    their held-out candidates are exactly the cells that tell the orders apart.  -> (train, truth, coo, qs, us)"""
    import predict_cases as PC
    c = PC.build_case(seed, nu, nq, KNIFE_USERS, KNIFE_QUERIES, user_longest=16, fill=fill, ordinary_query_longest=12,
                      ordinary_user_longest=8)
    rng = np.random.default_rng(seed + 1000003)
    train = c.ratings
    add = (train == 0) & (rng.random(train.shape) < held)
    add[:KNIFE_USERS] = False
    add[c.knife[:, 0], c.knife[:, 1]] = True
    truth = np.where(add, rng.integers(1, 101, size=train.shape), train).astype(np.int32)
    return train, truth, EC.coo_of(c.qs), c.qs, c.us


QUEUE_COUNTS = (0, 1, 1023, 1024, 1025, 2047, 2048, 4100)
QUEUE_NQ = 8192


def queue_case(seed=81):
    """nq = 8192, every cell rated in truth; user x has exactly QUEUE_COUNTS[x] test cells at random columns, and user 8
    has 2048: columns 1024 .. 2047 all test cells, 2048 .. 3071 none, the other 1024 scattered over the rest.  With one
    slice the LDS queue fills, overflows 1024 and drains at each of these counts."""
    nu, nq = len(QUEUE_COUNTS) + 1, QUEUE_NQ
    truth, coo, qs, us = EC.random_case(seed, nu, nq, 5, 3, fill=1.0)
    rng = np.random.default_rng(seed + 7)
    train = truth.copy()
    for u, n in enumerate(QUEUE_COUNTS):
        train[u, rng.choice(nq, size=n, replace=False)] = 0
    rest = np.concatenate([np.arange(0, 1024), np.arange(3072, nq)])
    train[nu - 1, 1024:2048] = 0
    train[nu - 1, rng.choice(rest, size=1024, replace=False)] = 0
    return train, truth, coo, qs, us


CUT_TARGETS = 1100          # target columns [0, C): unrated in train; source columns [C, 2 C): the targets' only neighbours
CUT_RELEVANT = 70
REL, NOT_REL = 80, 30       # truth values on either side of CUT_RELEVANT
CUT_USERS = ("ties", "short", "nothing", "no_relevant", "first", "last", "unlisted")


def cut_case(k):
    """Predictions under full control: user lists are empty and target query j has one neighbour, source C + j, at
    similarity 1.0, so the prediction of cell (u, j) is round(0.8 train[u][C + j] + 12) -- 0 when the source is unrated.
    Seven users (CUT_USERS), built around the cut at k:
      ties        k - t higher cells (t = min(3, k)), then SIX cells tied at 20 of which t are listed: truth relevant,
                  relevant, not | relevant, not, not for t = 3 -- the reverse tie order loses a hit; plus one relevant
                  test cell no neighbour rates (prediction 0: counted in word 5, never eligible)
      short       three eligible cells (k > avail for k > 3), the second relevant
      nothing     no eligible cell at all (avail 0), two relevant test cells
      no_relevant plenty of eligible cells, test cells below the threshold only
      first       the top cell is the one relevant test cell (first hit rank 1)
      last        the only relevant listed cell sits at position k (first hit rank k)
      unlisted    a relevant test cell at position k + 1: just outside (no hit)
    -> (train, truth, coo, qs, us, rows) with rows = {name: user}"""
    C = CUT_TARGETS
    nu, nq = len(CUT_USERS), 2 * C
    assert k + 8 <= C
    train = np.zeros((nu, nq), dtype=np.int32)
    truth = np.zeros((nu, nq), dtype=np.int32)
    rng = np.random.default_rng(1000 + k)
    rows = {name: u for u, name in enumerate(CUT_USERS)}

    def source_for(pred):
        """a source rating r with round(0.8 r + 12) == pred (pred in 13 .. 92, not every value has one)"""
        for r in range(1, 101):
            if round(0.8 * r + 12) == pred:
                return r
        raise AssertionError(pred)

    def put(u, col, pred, tv):
        train[u, C + col] = source_for(pred) if pred else 0
        truth[u, col] = tv

    # ties: columns drawn at random, the tie group in ascending column order c1 < .. < c6
    u = rows["ties"]
    t = min(3, k)
    cols = rng.permutation(C - 1)[:k - t + 6]
    for c in cols[:k - t]:
        put(u, int(c), int(rng.choice([28, 44, 60, 76, 92])), int(rng.choice([0, 0, NOT_REL, REL])))
    tie = np.sort(cols[k - t:])
    for c, tv in zip(tie.tolist(), (REL, REL, NOT_REL, REL, NOT_REL, NOT_REL)):
        put(u, c, 20, tv)
    put(u, C - 1, 0, REL)                                    # unreachable relevant test cell
    # short
    u = rows["short"]
    for c, pred, tv in ((5, 60, 0), (700, 44, REL), (C - 2, 28, NOT_REL)):
        put(u, c, pred, tv)
    # nothing: test cells without any rated neighbour
    u = rows["nothing"]
    put(u, 3, 0, REL)
    put(u, 900, 0, REL)
    # no_relevant
    u = rows["no_relevant"]
    for c in range(0, C, 3):
        put(u, c, int(rng.choice([20, 28, 44, 60])), NOT_REL if c % 2 else 0)
    # first / last / unlisted: k + 4 cells with strictly falling groups so that the positions are known
    for name, at in (("first", 0), ("last", k - 1), ("unlisted", k)):
        u = rows[name]
        cols = np.sort(rng.permutation(C)[:k + 4])
        for p, c in enumerate(cols.tolist()):        # equal values: the order is the column order
            put(u, c, 60, REL if p == at else (NOT_REL if p % 2 else 0))
    # the source columns are rated in truth as they are in train (they are not test cells)
    truth[:, C:] = train[:, C:]
    qs = {j: {"indexes": np.array([C + j], dtype=np.int64), "values": np.array([1.0])} for j in range(C)}
    return train, truth, EC.coo_of(qs), qs, {}, rows


def primes(k):
    """the first k primes, descending: a gain table no default could be mistaken for"""
    out, n = [], 2
    while len(out) < k:
        if all(n % p for p in out):
            out.append(n)
        n += 1
    return out[::-1]
