"""Cases and host restatements for the diversified lists (qrlsh.diversify / for_users_diverse / list_redundancy).

Lists are dicts of rows {q: (ids int64, milli int64)}, rows value descending then id ascending, no duplicates, milli in
1 .. 1000.  greedy_ref and redundancy_ref restate the rule in plain numpy / Python; brute_sim is an independent dense
form of sim for small nq.  Every builder plants what its name claims, so its conditions hold by construction; the host
test asserts them on the restatement alone."""
import numpy as np

NQ = 5003
RESERVED = 3900          # ids from here on have rows only where a builder plants them, and no base row names them
K_LISTS = 28
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
MODERATE = 20000         # 20 rating points per unit of similarity
# (penalty, max_sim) settings every planted request is served under
SETTINGS = ((0, 1001), (MODERATE, 1001), (1 << 20, 1001), (0, 1000), (0, 1), (5000, 500))


# ------------------------------------------------------------------------------------------------------ restatements
def lists_from_sims(qs):
    """{q: {'indexes', 'values'}} (values = milli / 1000) -> {q: (ids, milli)}"""
    return {int(q): (np.asarray(v["indexes"], dtype=np.int64), np.rint(np.asarray(v["values"]) * 1000).astype(np.int64))
            for q, v in qs.items()}


def coo_of(lists):
    """-> (q_src, q_dst, q_milli) int32 arrays sorted by source"""
    src, dst, mil = [], [], []
    for q in sorted(lists):
        ids, milli = lists[q]
        src += [q] * len(ids)
        dst += [int(x) for x in ids]
        mil += [int(x) for x in milli]
    return tuple(np.asarray(x, dtype=np.int32) for x in (src, dst, mil))


def stored(lists):
    """{a: {b: the largest milli stored under a -> b}}"""
    fwd = {}
    for a, (ids, milli) in lists.items():
        row = fwd.setdefault(int(a), {})
        for b, v in zip(ids.tolist(), milli.tolist()):
            row[b] = max(row.get(b, 0), int(v))
    return fwd


def sim_both(fwd):
    def sim(a, b):
        return max(fwd.get(a, {}).get(b, 0), fwd.get(b, {}).get(a, 0))
    return sim


def sim_picked_row_only(fwd):
    """the WRONG similarity that reads only the picked entry's own row: sim(c, s) = stored s -> c"""
    def sim(c, s):
        return fwd.get(s, {}).get(c, 0)
    return sim


def brute_sim(lists, nq):
    """dense (nq, nq): the larger of the two directions, built without the dict lookups"""
    d = np.zeros((nq, nq), dtype=np.int64)
    for a, (ids, milli) in lists.items():
        for b, v in zip(ids, milli):
            d[a, b] = max(d[a, b], v)
    return np.maximum(d, d.T)


def greedy_ref(cand_idx, cand_val, avail, lists, k, penalty, max_sim, sim=None, trace=None):
    """the rule, request by request -> (idx int32 (m, k), val int32 (m, k), red int32 (m, k), count int32 (m,)).
    sim: a callable (c, s) -> milli instead of the stored lists' both-direction one.  trace: a list that gets one
    (request, step, tied) per pick, tied = another eligible candidate had the pick's score."""
    cand_idx, cand_val = np.asarray(cand_idx), np.asarray(cand_val)
    m, N = cand_idx.shape
    sim = sim_both(stored(lists)) if sim is None else sim
    idx = np.full((m, k), -1, dtype=np.int32)
    val = np.zeros((m, k), dtype=np.int32)
    red = np.zeros((m, k), dtype=np.int32)
    count = np.zeros((m,), dtype=np.int32)
    for x in range(m):
        n = min(N, max(int(avail[x]), 0))
        cols = [int(c) for c in cand_idx[x, :n]]
        vals = [int(v) for v in cand_val[x, :n]]
        r = [0] * n
        picked = [False] * n
        for t in range(k):
            best, best_c, tied = None, -1, False
            for c in range(n):
                if picked[c] or not r[c] < max_sim:
                    continue
                score = 1000 * vals[c] - penalty * r[c]
                if best is None or score > best:
                    best, best_c, tied = score, c, False
                elif score == best:
                    tied = True
            if best_c < 0:
                break
            idx[x, t], val[x, t], red[x, t] = cols[best_c], vals[best_c], r[best_c]
            picked[best_c] = True
            count[x] = t + 1
            if trace is not None:
                trace.append((x, t, tied))
            for c in range(n):
                if not picked[c]:
                    r[c] = max(r[c], sim(cols[c], cols[best_c]))
    return idx, val, red, count


def greedy_brute(cand_idx, cand_val, avail, dense, k, penalty, max_sim):
    """the rule from its definition over a dense sim: r_c recomputed from every pick at every step"""
    cand_idx, cand_val = np.asarray(cand_idx), np.asarray(cand_val)
    m, N = cand_idx.shape
    out = (np.full((m, k), -1, dtype=np.int32), np.zeros((m, k), dtype=np.int32), np.zeros((m, k), dtype=np.int32),
           np.zeros((m,), dtype=np.int32))
    for x in range(m):
        n = min(N, max(int(avail[x]), 0))
        cols, vals = cand_idx[x, :n].astype(np.int64), cand_val[x, :n].astype(np.int64)
        picks = []
        for t in range(k):
            rest = [c for c in range(n) if c not in picks]
            r = {c: int(dense[cols[c], cols[picks]].max()) if picks else 0 for c in rest}
            elig = [c for c in rest if r[c] < max_sim]
            if not elig:
                break
            c = max(elig, key=lambda c: (1000 * int(vals[c]) - penalty * r[c], -c))
            out[0][x, t], out[1][x, t], out[2][x, t] = cols[c], vals[c], r[c]
            picks.append(c)
            out[3][x] = t + 1
    return out


def redundancy_ref(idx, lists, sim=None):
    """-> (words int64 (m, 4), totals int64 (4,)): entries listed, in-list pairs with sim > 0, their sum, the largest"""
    idx = np.asarray(idx)
    sim = sim_both(stored(lists)) if sim is None else sim
    words = np.zeros((idx.shape[0], 4), dtype=np.int64)
    for x, row in enumerate(idx):
        cols = [int(c) for c in row if c != -1]
        words[x, 0] = len(cols)
        for i in range(len(cols)):
            for j in range(i + 1, len(cols)):
                s = sim(cols[i], cols[j])
                if s > 0:
                    words[x, 1] += 1
                    words[x, 2] += s
                    words[x, 3] = max(words[x, 3], s)
    totals = np.array([words[:, 0].sum(), words[:, 1].sum(), words[:, 2].sum(), words[:, 3].max() if len(words) else 0],
                      dtype=np.int64)
    return words, totals


# ------------------------------------------------------------------------------------------------------------ builders
def _row(ids, milli):
    """a list row in stored order: value descending, id ascending"""
    ids, milli = np.asarray(ids, dtype=np.int64), np.asarray(milli, dtype=np.int64)
    assert len(set(ids.tolist())) == len(ids) and (len(milli) == 0 or (milli.min() >= 1 and milli.max() <= 1000))
    o = np.lexsort((ids, -milli))
    return ids[o], milli[o]


def base_lists(seed, nq=NQ, limit=RESERVED, longest=K_LISTS, window=48):
    """every query below `limit` gets 0 .. `longest` neighbours out of its id window (so pools cut from a window are
    full of stored neighbours, one direction more often than both); a fifth of the values are 1000 (equal answer
    sets).  Queries 0 and 1 have rows of length 0 and 1."""
    rng = np.random.default_rng(seed)
    lists = {}
    for q in range(limit):
        n = int(rng.integers(0, longest + 1))
        n = 0 if q == 0 else 1 if q == 1 else n
        lo, hi = max(0, q - window), min(limit, q + window + 1)
        pool = np.array([x for x in range(lo, hi) if x != q])
        ids = rng.choice(pool, size=min(n, len(pool)), replace=False)
        milli = np.where(rng.random(len(ids)) < 0.2, 1000, rng.integers(1, 1001, size=len(ids)))
        if len(ids):
            lists[q] = _row(ids, milli)
    return lists


def serve_order(cols, vals):
    """a pool in served order: value descending, column ascending"""
    cols, vals = np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64)
    assert len(set(cols.tolist())) == len(cols)
    o = np.lexsort((cols, -vals))
    return cols[o], vals[o]


class Case:
    """pools of one call: cand_idx / cand_val int32 (m, N) padded -1 / 0, avail int32 (m,), the lists and k"""

    def __init__(self, name, lists, N, k, nq=NQ):
        self.name, self.lists, self.N, self.k, self.nq = name, lists, N, k, nq
        self.rows, self.avail, self.notes = [], [], {}

    def add(self, cols, vals, avail=None, note=None, ordered=False):
        cols, vals = (np.asarray(cols), np.asarray(vals)) if ordered else serve_order(cols, vals)
        assert len(cols) <= self.N
        if note:
            self.notes[note] = len(self.rows)
        self.rows.append((cols, vals))
        self.avail.append(len(cols) if avail is None else avail)
        return len(self.rows) - 1

    def arrays(self):
        m = len(self.rows)
        ci = np.full((m, self.N), -1, dtype=np.int32)
        cv = np.zeros((m, self.N), dtype=np.int32)
        for x, (cols, vals) in enumerate(self.rows):
            ci[x, :len(cols)], cv[x, :len(cols)] = cols, vals
        return ci, cv, np.asarray(self.avail, dtype=np.int32)

    def coo(self):
        return coo_of(self.lists)


def _window_pool(rng, n, lo_val=45, hi_val=60, limit=RESERVED):
    """n distinct columns out of a window of about 1.5 n ids, values in a narrow range (many ties)"""
    span = min(limit, max(n + 1, int(1.5 * n) + 2))
    start = int(rng.integers(0, limit - span + 1))
    cols = start + rng.choice(span, size=n, replace=False)
    return cols, rng.integers(lo_val, hi_val + 1, size=n)


def size_case(N, seed=11):
    """a call at pool width N: a full pool whose avail says more were eligible, a full one, one short of full, an
    empty one (avail 0) and a request flagged as a bad user (avail -1)"""
    rng = np.random.default_rng(seed + N)
    c = Case("size%d" % N, base_lists(3), N, min(N, 28 if N >= 1023 else 10))
    c.add(*_window_pool(rng, N), avail=N + 37)
    c.add(*_window_pool(rng, N))
    c.add(*_window_pool(rng, N - 1))
    c.add([], [], avail=0)
    c.add([], [], avail=-1)
    return c


def full_order_case(N=257):
    """k = N: the whole pool is reordered"""
    rng = np.random.default_rng(5)
    c = Case("full%d" % N, base_lists(3), N, N)
    c.add(*_window_pool(rng, N))
    c.add(*_window_pool(rng, N // 2))
    return c


def main_case(m=300, N=256, k=10, seed=21):
    """m requests of mixed sizes in one call, some below k and some empty; avail between k and N and above N"""
    rng = np.random.default_rng(seed)
    c = Case("main", base_lists(3), N, k)
    for x in range(m):
        kind = x % 10
        n = 0 if kind == 0 and x % 20 == 0 else int(rng.integers(1, k)) if kind == 1 else int(rng.integers(k, N + 1))
        c.add(*_window_pool(rng, n), avail=n + int(rng.integers(0, 50)) if n == N else n)
    return c


def planted_case():
    """one call (N = 320, k = 12) of requests that each plant one structure over reserved ids; c.notes names them"""
    lists = base_lists(3)
    rng = np.random.default_rng(77)
    free = [RESERVED]

    def take(n):
        ids = np.arange(free[0], free[0] + n)
        free[0] += n
        assert free[0] <= NQ
        return ids

    c = Case("planted", lists, 320, 12)
    # a hub every other candidate names and that names nobody: reverse edges only, pool degree n - 1; the hub is served
    # first, so everything after it is decided by edges stored only in the OTHER entry's row
    ids = take(200)
    hub, others = ids[0], ids[1:]
    for j, q in enumerate(others):
        lists[int(q)] = _row([hub], [1 + (j * 37) % 1000])
    c.add(ids, np.concatenate(([90], rng.integers(40, 60, size=len(others)))), note="hub")
    # a row of 256, entirely inside the pool; a row of 1 and rows of 0 beside it
    ids = take(300)
    lists[int(ids[0])] = _row(ids[1:257], rng.integers(1, 1001, size=256))
    lists[int(ids[1])] = _row([ids[2]], [640])
    c.add(ids, np.concatenate(([80], rng.integers(40, 70, size=299))), note="row256")
    # one-directional edges a -> b: a served (and picked) first; then b first
    for note, va, vb in (("a_first", 70, 69), ("b_first", 69, 70)):
        ids = take(8)
        a, b = ids[0], ids[1]
        lists[int(a)] = _row([b], [900])
        c.add(ids, [va, vb, 68, 67, 66, 65, 64, 63], note=note)
    # runs of equal val across positions 63 / 64 and 255 / 256, every member with r = 0: the tie rule orders them; the
    # head of the pool is a star around position 0 that a penalty sends below the run
    for note, first in (("tie63", 58), ("tie255", 250)):
        ids = take(first + 14)
        for q in ids[1:first]:
            lists[int(q)] = _row([ids[0]], [1000])
        vals = np.concatenate(([99], np.full(first - 1, 60), np.full(14, 59)))
        c.add(ids, vals, note=note, ordered=True)
    # negative values
    ids = take(40)
    for q in ids[::3]:
        lists[int(q)] = _row(rng.choice(ids[ids != q], size=5, replace=False), rng.integers(1, 1001, size=5))
    c.add(ids, -rng.integers(1, 30, size=40), note="negative")
    # a clique of similarity 1000 at the head of the pool
    ids = take(30)
    for q in ids[:10]:
        lists[int(q)] = _row(ids[:10][ids[:10] != q], np.full(9, 1000))
    c.add(ids, np.concatenate((np.full(10, 95), rng.integers(40, 60, size=20))), note="clique")
    # a neighbour outside the pool: z is named by a with 1000 and names b with 1000, and is not a candidate
    ids = take(6)
    a, b, z = ids[0], ids[1], ids[5]
    lists[int(a)] = _row([z], [1000])
    lists[int(z)] = _row([b, a], [1000, 990])
    c.add(ids[:5], [70, 69, 68, 67, 66], note="outside")
    assert sorted(c.notes) == sorted(["hub", "row256", "a_first", "b_first", "tie63", "tie255", "negative", "clique",
                                      "outside"])
    return c


def small_case(seed, nq=60, m=6, N=24, k=8):
    """small enough for the dense brute form"""
    rng = np.random.default_rng(seed)
    lists = {}
    for q in range(nq):
        n = int(rng.integers(0, 9))
        if n:
            ids = rng.choice(np.array([x for x in range(nq) if x != q]), size=n, replace=False)
            lists[q] = _row(ids, np.where(rng.random(n) < 0.3, 1000, rng.integers(1, 1001, size=n)))
    c = Case("small%d" % seed, lists, N, k, nq=nq)
    for x in range(m):
        n = int(rng.integers(0, N + 1))
        c.add(rng.choice(nq, size=n, replace=False), rng.integers(-5, 6, size=n))
    return c
