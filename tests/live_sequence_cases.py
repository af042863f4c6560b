"""One host model of the whole live state (test infrastructure only: numpy, the oracle and the restatements of the other
*_cases modules), and seeded schedules that mix every live operation of the Recommender.

LiveModel holds plain host state -- string cells per slot, the served queries as strings, ids, ratings, labels, the two
list lengths and the run's permutation array -- and has one method per live operation with the Recommender's signature.
Each method does the bookkeeping only and returns what the real call must return.  expected() recomputes everything a
device structure holds from that state, from scratch, with restatements that already exist:

  answer sets over the live slots      table_rows_cases.brute_answer_sets (and the oracle's, which must agree)
  signatures                            table_rows_cases.oracle_signatures (oracle.answer_sets + oracle.minhash)
  query lists                           lists_update_cases.full_lists (oracle candidates, scores, top-K) at query_K
  user lists                            user_lists_cases.reference_lists at user_K
  newcomers' labels                     user_rows_cases.nearest_rule + assign_labels
  position maps                         user_rows_cases.new_positions

generate(seed) draws a deterministic list of operations with concrete arguments against the model (so a schedule runs
on the CPU alone) and records, per step, the operation, the return value, a note with the figures the schedule
conditions are stated in, expected() and a copy of the host state; run(seed) is that, computed once.
test_live_sequence_host.py checks the conditions; the GPU tests
drive the real structures through the same operations and compare after every step."""
import collections
import copy
import functools

import numpy as np

import lists_update_cases as LC
import table_rows_cases as TC
import user_lists_cases as UC
import user_rows_cases as RC

FAMILIES = ("queries", "rows", "users", "ratings", "lengths")
FAMILY = {"add_queries": "queries", "remove_queries": "queries", "replace_queries": "queries", "add_rows": "rows",
          "remove_rows": "rows", "add_users": "users", "remove_users": "users", "rate": "ratings",
          "set_list_lengths": "lengths"}
KINDS = tuple(FAMILY)
QUERY_MAX_K, USER_MAX_K = 256, 64
LC_TILE = 2048            # one tile of the cut and removal kernels
SERVED_MAX = 64           # the longest list the prediction kernels take
SHAPE = dict(N=340, P=16, b=8, K=8, D=60, cap=120, nu=100, user_K=6, nfeat=3, nvals=4, table_seed=3)
SERVED_USER_K = 4         # user lists below this length grow at their next change: the blend is served from several neighbours
SEEDS = (2, 6, 8)
STEPS = 36                # drawn steps of a schedule
EPILOGUE_SEED = 6
EPILOGUE_STEPS = 20       # drawn steps of the schedule that carries the epilogue (9 scripted steps)
SERVE_EVERY = 5


def steps_of(seed):
    return EPILOGUE_STEPS if seed == EPILOGUE_SEED else STEPS


def serve_points(count):
    """the steps after which the served predictions are compared: every fifth and the last"""
    return [i for i in range(count) if i % SERVE_EVERY == SERVE_EVERY - 1 or i == count - 1]


def _obj(a):
    """rows of strings as a 2-D object array"""
    out = np.asarray(a, dtype=object)
    return out if out.ndim == 2 else out.reshape(-1, out.shape[-1])


class LiveModel:
    def __init__(self, cells, queries, query_ids, user_ids, ratings, labels, query_K, user_K, perms, b, capacity=None):
        """cells: string cells [D, nfeat] of the dataset at the start (slot = position); perms int32 [P, capacity]"""
        cells = _obj(cells)
        self.perms = np.ascontiguousarray(perms, dtype=np.int32)
        self.capacity = int(self.perms.shape[1] if capacity is None else capacity)
        self.nfeat = cells.shape[1]
        self.D = cells.shape[0]                                   # the high-water slot
        self.cells = np.full((self.capacity, self.nfeat), None, dtype=object)
        self.cells[:self.D] = cells
        self.live = np.zeros(self.capacity, dtype=bool)
        self.live[:self.D] = True
        self.row_slots = np.arange(self.D, dtype=np.int64)        # the slot of every dataset position
        self.queries = _obj(queries).copy()
        self.query_ids = np.asarray(query_ids).astype(str)
        self.user_ids = np.asarray(user_ids).astype(str)
        self.ratings = np.array(ratings, dtype=np.int64)
        self.labels = np.array(labels, dtype=np.int64)
        self.query_K, self.user_K, self.b = int(query_K), int(user_K), int(b)
        self._memo_q = self._memo_u = None
        assert self.ratings.shape == (self.user_ids.size, self.query_ids.size) and self.queries.shape[0] == self.n

    def copy(self):
        return copy.deepcopy(self)

    n = property(lambda self: self.query_ids.size)
    nu = property(lambda self: self.user_ids.size)
    free_slots = property(lambda self: self.capacity - self.D)

    def dataset(self):
        """the string cells of every dataset position"""
        return self.cells[self.row_slots]

    # ---- from scratch ------------------------------------------------------------------------------------------------
    def encoded(self):
        """(cells int32 [capacity, nfeat], qrows int32 [n, nfeat]): one id per (feature, value) the live rows or the
        queries hold; -1 = unconstrained, -2 = a slot that is free or dead"""
        cells = np.full((self.capacity, self.nfeat), -2, dtype=np.int32)
        qrows = np.full((self.n, self.nfeat), -1, dtype=np.int32)
        nxt = 0
        for f in range(self.nfeat):
            col, q = self.cells[:, f], self.queries[:, f]
            vals = sorted(set(str(v) for v in col[self.live]) | set(str(v) for v in q if str(v) != ""))
            code = {v: nxt + k for k, v in enumerate(vals)}
            nxt += len(vals)
            for s in np.flatnonzero(self.live):
                cells[s, f] = code[str(col[s])]
            for k in range(self.n):
                if str(q[k]) != "":
                    qrows[k, f] = code[str(q[k])]
        return cells, qrows

    def _touch(self, q=False, u=False):
        """forget what an operation made stale: q = the query side (answer sets, signatures, query lists), u = the user
        side (user lists, means, norms)"""
        if q:
            self._memo_q = None
        if u:
            self._memo_u = None

    def expected(self):
        """everything the device holds, recomputed from the host state (each side memoised until an operation touches it)"""
        from oracle import oracle as O
        if self._memo_q is None:
            cells, qrows = self.encoded()
            off, rows = TC.brute_answer_sets(cells, qrows, self.live)
            sig, ooff, orows = TC.oracle_signatures(cells, qrows, self.perms, self.live)
            assert np.array_equal(off, ooff) and np.array_equal(rows, orows), "the two answer-set restatements differ"
            s = sig.astype(np.int64)
            qlists = LC.full_lists(sig, self.b, self.query_K)
            self._memo_q = dict(off=off, rows=rows, sig=sig, norm2=(s * s).sum(axis=1), qlists=qlists,
                                qfill=np.bincount(qlists[0], minlength=self.n), qdict=O.sims_to_dict(*qlists))
        if self._memo_u is None:
            c = UC.centred(self.ratings)
            cnt = (self.ratings != 0).sum(axis=1)
            mean = np.zeros(self.nu, dtype=np.float64)
            for u in np.flatnonzero(cnt):
                mean[u] = float(self.ratings[u].sum()) / float(cnt[u])
            self._memo_u = dict(ulists=UC.reference_lists(self.ratings, self.labels, self.user_K), mean=mean,
                                unorm2=(c * c).sum(axis=1))
        return dict(self._memo_q, **self._memo_u)

    def state(self):
        """a copy of the host state, for the comparisons of a step"""
        return dict(cells=self.cells.copy(), live=self.live.copy(), D=self.D, row_slots=self.row_slots.copy(),
                    queries=self.queries.copy(), query_ids=self.query_ids.copy(), user_ids=self.user_ids.copy(),
                    ratings=self.ratings.copy(), labels=self.labels.copy(), query_K=self.query_K, user_K=self.user_K)

    def full_rows_naming(self, ids):
        return full_rows_naming(self.expected(), self.query_K, ids)

    # ---- the operations ----------------------------------------------------------------------------------------------
    def add_queries(self, queries, ratings=None, ids=None):
        q = _obj(queries)
        m = q.shape[0]
        pos = np.arange(self.n, self.n + m, dtype=np.int64)
        block = np.zeros((self.nu, m), dtype=np.int64) if ratings is None else np.asarray(ratings, dtype=np.int64)
        labels = pos.astype(str) if ids is None else np.asarray(ids).astype(str)
        self.queries = np.concatenate((self.queries, q), axis=0)
        self.query_ids = np.concatenate((self.query_ids, labels))
        self.ratings = np.hstack((self.ratings, block))
        self._touch(q=True, u=True)
        return pos

    def remove_queries(self, positions):
        new_pos, keep = RC.new_positions(self.n, positions)
        self.queries, self.query_ids = self.queries[keep], self.query_ids[keep]
        self.ratings = np.ascontiguousarray(self.ratings[:, keep])
        self._touch(q=True, u=True)
        return new_pos

    def replace_queries(self, positions, queries, ratings=None):
        pos = np.asarray(positions, dtype=np.int64)
        assert np.unique(pos).size == pos.size
        self.queries = self.queries.copy()
        self.queries[pos] = _obj(queries)
        if ratings is not None:
            self.ratings[:, pos] = np.asarray(ratings, dtype=np.int64)
        self._touch(q=True, u=True)

    def add_rows(self, rows):
        r = _obj(rows)
        m = r.shape[0]
        assert m <= self.free_slots
        slots = np.arange(self.D, self.D + m, dtype=np.int64)      # dead slots are never used again
        first = self.row_slots.size
        self.cells[slots] = r
        self.live[slots] = True
        self.D += m
        self.row_slots = np.concatenate((self.row_slots, slots))
        self._touch(q=True)
        return np.arange(first, first + m, dtype=np.int64)

    def remove_rows(self, positions):
        new_pos, keep = RC.new_positions(self.row_slots.size, positions)
        gone = self.row_slots[~keep]
        self.live[gone] = False
        self.cells[gone] = None
        self.row_slots = self.row_slots[keep]
        self._touch(q=True)
        return new_pos

    def rate(self, users, queries, values):
        """-> the rows of the user lists rewritten: the users named and the full rows that named one of them"""
        u, q, v = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (users, queries, values))
        if u.size == 0:
            return 0
        idx, _, ln = self.expected()["ulists"]
        R = np.unique(u)
        inR = np.zeros(self.nu, dtype=bool)
        inR[R] = True
        picked = [w for w in range(self.nu) if not inR[w] and ln[w] == self.user_K and inR[idx[w, :ln[w]]].any()]
        for a, b, c in zip(u.tolist(), q.tolist(), v.tolist()):     # in order: the last repeat of a cell wins
            self.ratings[a, b] = c
        self._touch(u=True)
        return int(R.size) + len(picked)

    def add_users(self, ratings, ids=None, labels=None):
        """-> (positions, labels held): labels=None follows the nearest rule over the matrix before the batch"""
        block = np.asarray(ratings, dtype=np.int64).reshape(-1, self.n)
        m = block.shape[0]
        pos = np.arange(self.nu, self.nu + m, dtype=np.int64)
        if labels is None:
            user, milli, _ = RC.nearest_rule(self.ratings, block)
            lab = RC.assign_labels(self.labels, user, milli)
        else:
            lab = np.asarray(labels, dtype=np.int64)
        self.user_ids = np.concatenate((self.user_ids, pos.astype(str) if ids is None else np.asarray(ids).astype(str)))
        self.ratings = np.vstack((self.ratings, block))
        self.labels = np.concatenate((self.labels, lab))
        self._touch(u=True)
        return pos, lab.copy()

    def remove_users(self, positions):
        new_pos, keep = RC.new_positions(self.nu, positions)
        assert keep.any()
        self.user_ids, self.labels = self.user_ids[keep], self.labels[keep]
        self.ratings = np.ascontiguousarray(self.ratings[keep])
        self._touch(u=True)
        return new_pos

    def set_list_lengths(self, query_K=None, user_K=None):
        """-> (query rows probed again, user rows rescored), None for a side left alone: a regrow takes the rows that
        are full at the old length, a cut none"""
        e = self.expected()
        pq = pu = None
        if query_K is not None:
            pq = int((e["qfill"] == self.query_K).sum()) if query_K > self.query_K else 0
        if user_K is not None:
            pu = int((e["ulists"][2] == self.user_K).sum()) if user_K > self.user_K else 0
        if query_K is not None:
            self.query_K = int(query_K)
        if user_K is not None:
            self.user_K = int(user_K)
        self._touch(q=query_K is not None, u=user_K is not None)
        return pq, pu


def predictions(step, users, summation):
    """oracle.predict_cells over the two lists of a recorded step, for every cell of the chosen users: int64
    [len(users), n]"""
    from oracle import oracle as O
    e, r = step.expected, step.state["ratings"]
    idx, mil, ln = e["ulists"]
    us = {u: {"indexes": idx[u, :ln[u]].astype(np.int64), "values": mil[u, :ln[u]].astype(np.float64) / 1000.0}
          for u in users}
    cells = [(u, q) for u in users for q in range(r.shape[1])]
    return O.predict_cells(r, e["qdict"], us, cells, summation).reshape(len(users), r.shape[1])


def full_rows_naming(e, K, ids):
    """the query rows of the lists of e outside ids that hold exactly K entries, one of which names a query of ids: the
    rows the device must probe again"""
    src, dst, _ = e["qlists"]
    n = len(e["qfill"])
    mark = np.zeros(n, dtype=bool)
    mark[np.asarray(ids, dtype=np.int64)] = True
    named = np.zeros(n, dtype=bool)
    named[src[mark[dst]]] = True
    return np.flatnonzero(named & ~mark & (e["qfill"] == K))


# ---- the starting state ------------------------------------------------------------------------------------------------
def start_ratings(seed=77):
    """mixed_matrix's recipe at the model's shape: 55 like-minded users (cluster 0) and 45 random ones over clusters
    1 .. 5, interleaved in id order"""
    s = SHAPE
    rng = np.random.default_rng(seed)
    like = 55
    r = np.vstack((UC._like_minded(rng, like, s["N"], noise=2), UC._random(rng, s["nu"] - like, s["N"], fill=0.3)))
    lab = np.concatenate((np.zeros(like, dtype=np.int64), 1 + rng.integers(0, 5, size=s["nu"] - like)))
    perm = rng.permutation(s["nu"])
    return r[perm], lab[perm]


def start_model():
    from oracle import oracle as O
    s = SHAPE
    columns, queries = TC.string_table(s["N"], s["D"], 0, nfeat=s["nfeat"], nvals=s["nvals"])
    ratings, labels = start_ratings()
    perms = O.legacy_permutations(s["table_seed"], s["P"], s["cap"])
    return LiveModel(np.stack(columns, axis=1), queries, ["q%d" % k for k in range(s["N"])],
                     ["u%d" % k for k in range(s["nu"])], ratings, labels, s["K"], s["user_K"], perms, s["b"])


def golden_model(sub="cfg2", spare=40):
    """the model of a generator data set under tests/golden (its table, queries, string ids and utility matrix as the
    reference's main flow reads them), as a Recommender holds it after a run under the data set's own seed and P with
    `spare` free slots: K = round(log_1.5 queries), the band rule, the user lists at round(log_1.5 users) over the
    reference's clustering (labels are data here: BIRCH is not part of the live state)"""
    import csv
    import os
    from oracle import oracle as O
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(root, sub + "_scores.npz"))
    with open(os.path.join(root, sub, "dataset.csv"), newline="") as fh:
        table = list(csv.reader(fh))
    features, cells = table[0][1:], [r[1:] for r in table[1:]]
    ids, queries = [], []
    with open(os.path.join(root, sub, "queries.csv")) as fh:
        for line in fh:
            parts = line.rstrip("\n").split(",")
            ids.append(parts[0])
            row = [""] * len(features)
            for item in parts[1:]:
                name, value = item.split("=")
                row[features.index(name)] = value
            queries.append(row)
    with open(os.path.join(root, sub, "users.csv")) as fh:
        users = [line.strip() for line in fh if line.strip()]
    ratings = np.asarray(g["ratings"], dtype=np.int64)
    P, seed = int(g["P"]), int(g["seed"])
    cap = len(cells) + spare
    return LiveModel(cells, queries, ids, users, ratings, O.user_cluster_labels(ratings), O.max_candidates(len(ids)),
                     O.max_candidates(len(users)), O.legacy_permutations(seed, P, cap), O.select_bands(P))


GOLDEN_SEED = 5


@functools.lru_cache(maxsize=None)
def golden_run(sub="cfg2"):
    """(the step of golden_model(sub) as it stands, a run of the committed generator drawn against it): the schedules of
    start_model() name positions of its 340 queries and cannot run here, so this data set gets a draw of its own"""
    model = golden_model(sub)
    return step_of(model), run_from(model, GOLDEN_SEED, STEPS)


# ---- operations as data ------------------------------------------------------------------------------------------------
def apply(model, op):
    """run one operation (kind, kwargs) on the model -> what the real call must return"""
    kind, kw = op
    return getattr(model, kind)(**kw)


def describe(op):
    """the operation with its arguments, short enough for an assertion message"""
    kind, kw = op
    parts = []
    for k, v in kw.items():
        if v is None or np.isscalar(v):
            parts.append("%s=%r" % (k, v))
        else:
            a = np.asarray(v, dtype=object)
            parts.append("%s=%s" % (k, a.tolist() if a.size <= 12 else "%s%s..." % (a.shape, a.reshape(-1)[:6].tolist())))
    return "%s(%s)" % (kind, ", ".join(parts))


def _circuit(rng):
    """a closed walk over the families that takes every ordered pair once (self loops included) and query set -> list
    lengths four times (a cut and a regrow directly after a removal and after an append): 32 steps"""
    edges = {a: list(FAMILIES) for a in FAMILIES}
    edges["queries"] += ["lengths"] * 3
    edges["lengths"] += ["queries"] * 3
    for a in FAMILIES:
        edges[a] = [edges[a][k] for k in rng.permutation(len(edges[a]))]
    stack, out = [FAMILIES[int(rng.integers(0, 5))]], []
    while stack:
        if edges[stack[-1]]:
            stack.append(edges[stack[-1]].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


MOTIFS = (("remove_queries", "cut"), ("remove_queries", "regrow"), ("add_queries", "cut"), ("add_queries", "regrow"))
SHORT_PLAN = 20


def _kinds(rng, fams):
    """kinds inside the families of a walk, least used first; a query step directly before a list-length step takes the
    next motif and tells that step what to do.  -> [(kind, hint)]"""
    motifs = [MOTIFS[k] for k in rng.permutation(4)]
    used = {k: 0 for k in KINDS}
    plan, told = [], None
    for i, f in enumerate(fams):
        hint, told = (told if f == "lengths" else None), None
        if f == "queries" and i + 1 < len(fams) and fams[i + 1] == "lengths" and motifs:
            kind, told = motifs.pop(0)
        else:
            kinds = [k for k in KINDS if FAMILY[k] == f]
            low = min(used[k] for k in kinds)
            kinds = [k for k in kinds if used[k] == low]
            kind = kinds[int(rng.integers(0, len(kinds)))]
        used[kind] += 1
        plan.append((kind, hint))
    return plan


def _plan(rng, steps):
    """the kinds of a schedule -> [(kind, hint)]: hint = what a list-length step directly after a query step does.
    steps >= 32: the circuit over the families, further steps drawn freely.  Fewer (the schedule that carries the
    epilogue: the pairs of families are a condition over all seeds, not per seed): the four motifs as adjacent pairs and
    every other kind twice, in a drawn order -- 20 steps -- then free steps."""
    if steps >= 32:
        fams = _circuit(rng)
    else:
        units = [("queries", "lengths")] * 4 + [("queries",)] * 2 + [(f,) for f in ("rows", "users") for _ in range(4)] + \
                [("ratings",)] * 2
        fams = [f for k in rng.permutation(len(units)) for f in units[k]]
    fams += [FAMILIES[int(rng.integers(0, 5))] for _ in range(steps - len(fams))]
    return _kinds(rng, fams)


def _texts(rng, model, m, step):
    """m query texts: copies of served queries (their signatures collide), fresh draws over the values the table holds,
    and now and then a value new to the dictionary"""
    pool = [sorted(set(str(v) for v in model.cells[model.live, f])) for f in range(model.nfeat)]
    out = np.empty((m, model.nfeat), dtype=object)
    for k in range(m):
        if rng.random() < 0.4:
            out[k] = model.queries[int(rng.integers(0, model.n))]
        else:
            for f in range(model.nfeat):
                out[k, f] = "" if rng.random() < 0.5 else pool[f][int(rng.integers(0, len(pool[f])))]
            if not any(out[k]):
                out[k, 0] = pool[0][0]
    if m >= 3 and rng.random() < 0.5:
        out[m - 1, int(rng.integers(0, model.nfeat))] = "novel%d" % step
    return out


def _block(rng, rows, cols, fill=0.15):
    return (rng.integers(1, 101, size=(rows, cols)) * (rng.random((rows, cols)) < fill)).astype(np.int64)


def _positions(rng, pool, count, must=()):
    """unordered positions with a duplicate"""
    pool = np.asarray(pool, dtype=np.int64)
    pick = rng.choice(pool, size=min(count, pool.size), replace=False).tolist() + [int(x) for x in must]
    pick = list(dict.fromkeys(pick))
    pick.append(pick[int(rng.integers(0, len(pick)))])
    return np.asarray(pick, dtype=np.int64)[rng.permutation(len(pick))]


def _named_by_full_rows(rng, model):
    """a query that full rows name, or nothing"""
    e = model.expected()
    src, dst, _ = e["qlists"]
    full = e["qfill"][src] == model.query_K
    return [int(dst[full][int(rng.integers(0, int(full.sum())))])] if full.any() else []


def _lengths(rng, model, hint, step):
    e = model.expected()
    kw = {}
    sides = ("query", "user", "both")[int(rng.integers(0, 3))] if hint is None else ("query", "both")[step % 2]

    def draw(cur, fill, top, mode, keep_long):
        """from {1, cur - 1, cur + 1, a length above every row's fill, the maximum}; the maximum is drawn seldom (beyond
        64 entries no list is served), and lists below one tile of entries grow"""
        above = min(top, int(fill.max(initial=0)) + int(rng.integers(1, 8)))
        opts, w = [1, cur - 1, cur + 1, above, top], np.array([0.15, 0.25, 0.2, 0.35, 0.05])
        ok = np.array([1 <= x <= top and x != cur for x in opts])
        if mode == "cut" or (mode is None and cur > SERVED_MAX):
            ok &= np.array([x < cur for x in opts])
        elif mode == "regrow" or keep_long:
            ok &= np.array([x > cur for x in opts])
        if not ok.any():
            return cur - 1 if cur > 1 else cur + 1
        w = np.where(ok, w, 0.0)
        return int(opts[int(rng.choice(5, p=w / w.sum()))])
    if sides in ("query", "both"):
        short = len(e["qlists"][0]) <= LC_TILE
        kw["query_K"] = draw(model.query_K, e["qfill"], QUERY_MAX_K, hint, short)
    if sides in ("user", "both"):
        kw["user_K"] = draw(model.user_K, e["ulists"][2], USER_MAX_K, None, model.user_K < SERVED_USER_K)
    return kw


def _draw(rng, model, kind, hint, step, seen):
    """seen: how often the kind occurred before in this schedule (variants take turns)"""
    n, nu = model.n, model.nu
    if kind == "add_queries":
        m = int(rng.integers(8, 30))
        kw = dict(queries=_texts(rng, model, m, step), ids=np.asarray(["s%dq%d" % (step, k) for k in range(m)]))
        kw["ratings"] = _block(rng, nu, m) if rng.random() < 0.6 else None
        return kind, kw
    if kind == "remove_queries":
        count = int(rng.integers(4, 30))
        return kind, dict(positions=_positions(rng, np.arange(n), min(count, n - 3), _named_by_full_rows(rng, model)))
    if kind == "replace_queries":
        m = int(rng.integers(2, 10))
        pos = np.unique(_positions(rng, np.arange(n), m, _named_by_full_rows(rng, model)))
        pos = pos[rng.permutation(pos.size)]
        q = _texts(rng, model, pos.size, step)
        other = int(rng.integers(0, n))
        q[0] = model.queries[other if other != pos[0] else (other + 1) % n]       # the text of another: signatures collide
        return kind, dict(positions=pos, queries=q, ratings=_block(rng, nu, pos.size) if rng.random() < 0.5 else None)
    if kind == "add_rows":
        m = int(rng.integers(1, 5))
        m = min(m, model.free_slots)
        rows = model.dataset()[rng.integers(0, model.row_slots.size, size=m)].copy()
        how = seen % 3
        if how == 0:                        # values nobody names: only an all-unconstrained query can match
            rows[:] = [["nobody%d_%d_%d" % (step, k, f) for f in range(model.nfeat)] for k in range(m)]
        elif how == 1:                      # one value new to the dictionary; the other features match many queries
            rows[0, int(rng.integers(0, model.nfeat))] = "brandnew%d" % step
        return kind, dict(rows=rows)
    if kind == "remove_rows":
        count = int(rng.integers(1, 6))
        return kind, dict(positions=_positions(rng, np.arange(model.row_slots.size), count))
    if kind == "rate":
        c = int(rng.integers(5, 14))
        u, q, v = rng.integers(0, nu, size=c), rng.integers(0, n, size=c), rng.integers(0, 101, size=c)
        v[rng.random(c) < 0.3] = 0
        u, q, v = np.concatenate((u, u[:2])), np.concatenate((q, q[:2])), np.concatenate((v, [0, 55]))   # repeated cells
        return kind, dict(users=u, queries=q, values=v)
    if kind == "add_users":
        src = model.ratings[int(rng.integers(0, nu))]
        copy_ = np.where(rng.random(n) < rng.uniform(0.1, 0.2), 0, src)          # 10-20 % of the cells blanked
        more = model.ratings[rng.integers(0, nu, size=int(rng.integers(1, 5)))]
        rows = np.vstack((copy_, np.zeros(n, dtype=np.int64), _block(rng, 1, n, fill=0.3)[0],
                          np.where(rng.random(more.shape) < 0.15, 0, more)))
        given = None
        if seen % 2:
            given = np.concatenate(([int(model.labels[0]), 1000 + step, 1000 + step], model.labels[:rows.shape[0] - 3]))
        return kind, dict(ratings=rows, ids=np.asarray(["s%du%d" % (step, k) for k in range(rows.shape[0])]), labels=given)
    if kind == "remove_users":
        count = int(rng.integers(2, 7))
        return kind, dict(positions=_positions(rng, np.arange(nu), min(count, nu - 3)))
    if kind == "set_list_lengths":
        return kind, _lengths(rng, model, hint, step)
    raise AssertionError(kind)


def _feasible(model, kind):
    if kind == "add_rows" and model.free_slots < 1:
        return "remove_rows"
    if kind == "remove_rows" and model.row_slots.size < 12:
        return "add_rows" if model.free_slots else "rate"
    if kind == "remove_queries" and model.n < 40:
        return "add_queries"
    if kind == "remove_users" and model.nu < 12:
        return "add_users"
    return kind


def _epilogue(rng, model, do):
    """cut both sides to 1, regrow both to their maxima, queries and users down to two, back to about the starting
    size, a few more ratings, and a cut to a length the serving kernels take.  do(kind, **kw) runs and records"""
    do("set_list_lengths", query_K=1, user_K=1)
    do("set_list_lengths", query_K=QUERY_MAX_K, user_K=USER_MAX_K)
    do("remove_queries", positions=rng.permutation(model.n)[2:])
    do("remove_users", positions=rng.permutation(model.nu)[2:])
    m = SHAPE["N"] - 2
    start = start_model()
    do("add_queries", queries=start.queries[rng.permutation(SHAPE["N"])[:m]], ratings=_block(rng, 2, m, fill=0.5),
       ids=np.asarray(["e%d" % k for k in range(m)]))
    mu = SHAPE["nu"] - 2
    rows = start.ratings[rng.permutation(SHAPE["nu"])[:mu]][:, rng.permutation(SHAPE["N"])[:model.n]]
    half = mu // 2
    do("add_users", ratings=rows[:half], ids=np.asarray(["eu%d" % k for k in range(half)]), labels=None)
    do("add_users", ratings=rows[half:], ids=np.asarray(["ev%d" % k for k in range(mu - half)]),
       labels=rng.integers(0, 4, size=mu - half))
    c = 12
    do("rate", users=rng.integers(0, model.nu, size=c), queries=rng.integers(0, model.n, size=c),
       values=rng.integers(0, 101, size=c))
    do("set_list_lengths", query_K=12, user_K=9)


def _generate(rng, model, steps, epilogue):
    """draw the operations against the model and record every step on the way -> [Step]"""
    out, seen = [], {k: 0 for k in KINDS}

    def do(kind, **kw):
        ret, note = step(model, (kind, kw))
        out.append(Step((kind, kw), ret, note, model.expected(), model.state()))
    for i, (kind, hint) in enumerate(_plan(rng, steps)):
        kind = _feasible(model, kind)
        op = _draw(rng, model, kind, hint, i, seen[kind])
        seen[kind] += 1
        do(op[0], **op[1])
    if epilogue:
        _epilogue(rng, model, do)
    return out


def generate(seed, steps=None, epilogue=None):
    """the run of a seed from start_model(): [Step] -- the operation (kind, kwargs) drawn against the model, what it
    returns, the note, expected() and a copy of the host state afterwards.  The same seed gives the same run; the run of
    EPILOGUE_SEED is shorter (steps_of) and ends with the scripted epilogue."""
    return _generate(np.random.default_rng(seed), start_model(), steps_of(seed) if steps is None else steps,
                     (seed == EPILOGUE_SEED) if epilogue is None else epilogue)


def run_from(model, seed, steps):
    """a run drawn against another starting state (the model is not modified)"""
    return _generate(np.random.default_rng(seed), model.copy(), steps, False)


@functools.lru_cache(maxsize=None)
def run(seed):
    """generate(seed), computed once and shared by every test"""
    return generate(seed)


def schedule(seed, steps=None):
    """the operations of a seed: [(kind, kwargs)] with concrete arguments; steps: the drawn steps (default: steps_of(seed),
    the committed schedule, taken from run(seed))"""
    trace = run(seed) if steps is None or steps == steps_of(seed) else generate(seed, steps)
    return [s.op for s in trace]


# ---- a run on the host -------------------------------------------------------------------------------------------------
def step(model, op):
    """apply op -> (what the call returns, the note of the step): the figures the schedule conditions are stated in"""
    kind, kw = op
    before = model.expected()
    n0, K0 = model.n, model.query_K
    note = dict(kind=kind, family=FAMILY[kind], full_hit=None, changed=None, picked=(None, None), joined=0, founded=0)
    if kind == "remove_queries":
        note["full_hit"] = len(model.full_rows_naming(np.unique(kw["positions"])))
    elif kind == "replace_queries":
        note["full_hit"] = len(model.full_rows_naming(kw["positions"]))
    elif kind in ("add_rows", "remove_rows"):
        note["slots"] = (model.row_slots[np.unique(kw["positions"])] if kind == "remove_rows" else
                         np.arange(model.D, model.D + len(kw["rows"]), dtype=np.int64))
    elif kind == "add_users" and kw["labels"] is None:
        top = int(model.labels.max())
    ret = apply(model, op)
    if kind == "add_users" and kw["labels"] is None:
        note["founded"], note["joined"] = int((ret[1] > top).sum()), int((ret[1] <= top).sum())
    if kind == "set_list_lengths":
        note["picked"] = ret
        note["query_mode"] = None if kw.get("query_K") is None else ("cut" if kw["query_K"] < K0 else "regrow")
    after = model.expected()
    if kind in ("add_rows", "remove_rows"):
        ids = np.flatnonzero((after["sig"] != before["sig"]).any(axis=1))
        note["changed"], note["full_hit"] = len(ids), len(full_rows_naming(before, K0, ids))
    note.update(stored=len(after["qlists"][0]), n=model.n, nu=model.nu, longest=int(after["qfill"].max(initial=0)))
    return ret, note


Step = collections.namedtuple("Step", "op returned note expected state")


def step_of(model):
    """the state of a model as it stands, in the form of a recorded step"""
    e = model.expected()
    note = dict(kind="start", stored=len(e["qlists"][0]), n=model.n, nu=model.nu, longest=int(e["qfill"].max(initial=0)))
    return Step(("start", {}), None, note, e, model.state())


def start_step():
    return step_of(start_model())


def replay_model(seed, upto):
    """the model after the first `upto` operations of schedule(seed)"""
    model = start_model()
    for op in schedule(seed)[:upto]:
        apply(model, op)
    return model


def conditions(seed):
    """the figures of the schedule conditions for one seed"""
    return conditions_of(run(seed))


def conditions_of(trace):
    notes = [x.note for x in trace]
    kinds = [x["kind"] for x in notes]
    s = SHAPE
    after = lambda prev, mode: sum(1 for a, b in zip(notes, notes[1:]) if a["kind"] == prev and b["kind"] == "set_list_lengths"
                                   and b.get("query_mode") == mode)
    return dict(
        steps=len(notes),
        kinds={k: kinds.count(k) for k in KINDS},
        pairs={(a["family"], b["family"]) for a, b in zip(notes, notes[1:])},
        long_steps=sum(1 for x in notes if x["stored"] > LC_TILE),
        full_hits={k: sum(1 for x in notes if x["kind"] == k and x["full_hit"]) for k in
                   ("remove_queries", "replace_queries", "remove_rows", "add_rows")},
        reprobed=sum(1 for x in notes if x["full_hit"]),
        query_regrows=sum(1 for x in notes if x["picked"][0]),
        user_regrows=sum(1 for x in notes if x["picked"][1]),
        cut_after_removal=after("remove_queries", "cut"), regrow_after_removal=after("remove_queries", "regrow"),
        cut_after_append=after("add_queries", "cut"), regrow_after_append=after("add_queries", "regrow"),
        quiet_add_rows=sum(1 for x in notes if x["kind"] == "add_rows" and x["changed"] == 0),
        loud_add_rows=sum(1 for x in notes if x["kind"] == "add_rows" and x["changed"]),
        joined=sum(x["joined"] for x in notes), founded=sum(x["founded"] for x in notes),
        n_range=(min(x["n"] for x in notes), max(x["n"] for x in notes)),
        nu_range=(min(x["nu"] for x in notes), max(x["nu"] for x in notes)),
        served_user_K=[trace[i].state["user_K"] for i in serve_points(len(trace)) if trace[i].note["longest"] <= SERVED_MAX],
        start=(s["N"], s["nu"]))
