"""Drop-in for the hot-path half of the reference's recommender.py (lines 105-214).

Same names and return types as the reference's Recommender for the query-similarity path:

    compute_shingles()            -> dict row -> [queries]            (recommender.py:68-103)
    compute_signatures()          -> int64 ndarray (nq, PERM)         (recommender.py:105-143)
    compute_querySimilarities()   -> {q: {'indexes', 'values'}}       (recommender.py:145-214)

The MinHash / LSH / scoring / top-K work runs in libqrlsh (HIP, gfx950).  The module constant
PERM and the global legacy numpy RNG are honoured exactly like the reference: under
np.random.seed(s) the signatures are bit-identical to the reference's.  Tie order inside a
query's top-K list is defined here (value descending, then neighbour id ascending); the
reference's is arbitrary.

Widening beyond the hot path: answer sets (compute_shingles, N2) and the
hybrid prediction loop (compute_scores / weighted_average, N1) run on the device; CSV ingest
(init / parse_queries, N3) takes datatable Frames (what main.py passes) or pandas frames; user similarity (N4) is the same
sklearn pipeline the reference calls, on the host.
"""
import math
import time

import numpy as np
import pandas as pd
import torch

import qrlsh
from qrlsh import ops, pipeline
from qrlsh._args import _int_in
from qrlsh._inputs import sum_order_code
from lsh import LSH  # noqa: F401  (same import the reference has)

# constants (recommender.py:30-34)
PERM = 180  # number of independent hash functions

QUERY_WEIGHT = 0.6
USER_WEIGHT = 0.4
DEFAULT_MEAN = 60

LSH_THRESH = 0.2  # recommender.py:153


def _as_pandas(x):
    """pandas view of a frame-like argument of init(): a pandas DataFrame as is, a datatable Frame (or any object
    with .to_pandas()) through its own conversion, anything else through numpy"""
    if isinstance(x, pd.DataFrame):
        return x
    if hasattr(x, "to_pandas"):
        return x.to_pandas()
    names = getattr(x, "names", None)
    return pd.DataFrame(np.asarray(x), columns=list(names) if names is not None else None)


def _as_numpy(x):
    return x.to_numpy() if hasattr(x, "to_numpy") else np.asarray(x)


def _diversify():
    """the module qrlsh.diversify (the package attribute of that name is the function)"""
    import importlib
    return importlib.import_module("qrlsh.diversify")


def _ids_arg(ids):
    """chosen users or positions as the device wrappers take them: a tensor stays, None (= all) stays, anything else
    becomes an array"""
    return ids if ids is None or isinstance(ids, torch.Tensor) else np.asarray(ids)


def _positions(positions, below=None, distinct=None):
    """positions -> flat int64 host array, ValueError unless they are integers.  below=n: unique and sorted, all in
    [0, n); distinct=(m, n): m different ones in [0, n), in the caller's order"""
    pos = np.asarray(_as_numpy(positions)).reshape(-1)
    if pos.size and not np.issubdtype(pos.dtype, np.integer):
        raise ValueError("positions must be integers")
    pos = pos.astype(np.int64)
    if below is not None:
        pos = np.unique(pos)
        if pos.size and (pos[0] < 0 or pos[-1] >= below):
            raise ValueError("position outside [0, %d)" % below)
    if distinct is not None:
        m, n = distinct
        if pos.size != m or np.unique(pos).size != m or (m and (pos.min() < 0 or pos.max() >= n)):
            raise ValueError("positions must be %d distinct integers in [0, %d)" % (m, n))
    return pos


def _ratings_block(ratings, rows, cols):
    """an integer ratings block of `cols` columns as int64: [users, m] with `rows` rows, [m, queries] with any (None)"""
    block = np.asarray(_as_numpy(ratings))
    if block.ndim != 2 or block.shape[1] != cols or rows not in (None, block.shape[0]) or \
            not np.issubdtype(block.dtype, np.integer):
        raise ValueError("ratings must be an integer [m, queries] = [m, %d] block" % cols if rows is None else
                         "ratings must be an integer [users, m] = [%d, %d] block" % (rows, cols))
    return block.astype(np.int64)


def _served(chosen, first, values, avail, length, key, redundancy=None):
    """The dict the recommend* calls return, from the device's padded rows: {id: {key: int64, 'values': int64,
    'available': int[, 'redundancy': int64]}} with id = chosen[i] (None: i) and row i cut to its first length[i] entries;
    length = k stands for min(k, avail[i])"""
    first, values, avail = ops.to_host(first), ops.to_host(values), ops.to_host(avail)
    length = np.minimum(int(length), avail) if np.ndim(length) == 0 else ops.to_host(length)
    redundancy = None if redundancy is None else ops.to_host(redundancy)
    out = {}
    for i, x in enumerate(range(len(avail)) if chosen is None else [int(x) for x in ops.to_host(chosen)]):
        n = int(length[i])
        out[x] = {key: first[i, :n].astype(np.int64), "values": values[i, :n].astype(np.int64),
                  "available": int(avail[i])}
        if redundancy is not None:
            out[x]["redundancy"] = redundancy[i, :n].astype(np.int64)
    return out


class Recommender:

    device = "cuda"
    verbose = True
    bands = None            # override the band rule (BASELINE shapes 128/32, 256/64 need it)
    max_candidates = None   # override K
    row_capacity = None     # dataset rows the permutation table is drawn for (None: the dataset's own, as the reference);
                            # a value >= the dataset's rows leaves free slots for add_rows

    def _log(self, *a):
        if self.verbose:
            print(*a)

    cluster_on_device = True   # StandardScaler + PCA of compute_userSimilarities on the device (False: scikit-learn on the host)
    sum_order = "sequential"   # order of weighted_average's two np.sum calls, see compute_scores
    query_weight = QUERY_WEIGHT   # the blend every serving call uses (recommender.py:32-34 of the reference); tune(apply=True)
    user_weight = USER_WEIGHT     # sets the three on the instance
    default_mean = DEFAULT_MEAN
    diversity_penalty = 0      # the rerank recommend_users_diverse applies when called without one: the plain list;
    diversity_max_sim = 1001   # tune_diversity(apply=True) sets the two on the instance

    # the state of a run, None until its setter has run
    last_result = None         # compute_querySimilarities: the run's HotPathResult
    last_table = None          # compute_querySimilarities: the permutation table the run was drawn with
    _query_index = None        # _run_index, on the first live call after a run; compute_querySimilarities resets it
    _live_table = None         # _live_rows, on the first add_rows / remove_rows; compute_querySimilarities resets it
    row_slots = None           # _live_rows, with _live_table: the table slot of every dataset position
    _answer_index = None       # answer_sets_device: the dataset's AnswerIndex,
    _answer_index_key = None   # and the id() of the dataset it encodes
    user_index = None          # live_user_similarities: the UserLists that follow self.ratings

    def init(self, users, queries, queriesIDs, dataset, ratings):
        """recommender.py:51-64.  Takes what main.py:23-85 passes -- `datatable` Frames (anything Frame-like:
        `.to_pandas()` / `.to_numpy()` / `.names`) -- and pandas frames / arrays alike (N3): users = one column
        of user ids, queries = the frame parse_queries returned, dataset = the table (every column becomes
        str, :57), ratings = the utility matrix with its leading 'user' column (dropped, :61; missing ratings
        become 0, :62).  The caller's frames are not modified (the reference edits `dataset` and `ratings` in
        place; nothing reads them afterwards)."""
        self.usersIDs = _as_numpy(users).T[0]
        self.queries = _as_numpy(queries)
        self.queriesIDs = np.array(queriesIDs)
        self.dataset = _as_pandas(dataset).astype(str)
        self.tupleCount = {}
        r = _as_pandas(ratings)
        if "user" in list(r.columns):
            r = r.drop(columns=["user"])
        r = r.apply(pd.to_numeric, errors="coerce") if any(dt == object for dt in r.dtypes) else r
        self.ratings = np.nan_to_num(r.to_numpy(dtype=np.float64, na_value=np.nan), nan=0.0).astype(np.int64)

    def parse_queries(self, path: str):
        """recommender.py:386-416: one query per line, `id,attr=value,attr=value,...`;
        -> (DataFrame with one column per dataset feature, "" where unconstrained; list of ids)"""
        ids, data = [], []
        with open(path) as fh:
            for line in fh:
                parts = line.rstrip("\n").split(",")
                ids.append(parts[0])
                row = ["" for _ in self.datasetFeatures]
                for item in parts[1:]:
                    name, value = item.split("=")
                    row[self.datasetFeatures.index(name)] = value
                data.append(row)
        return pd.DataFrame(data, columns=list(self.datasetFeatures), dtype=object), ids

    # ---- producer of the hot path's input (row N2: answer sets on the device) -----
    def answer_sets_device(self):
        """CSR answer sets on the device: (offsets int64 [nq+1], rows int32 [nnz]); the table is
        dictionary-encoded into per-(feature, value) bitmaps once and cached."""
        return self._answer_sets_of(self.queries)

    def _answer_sets_of(self, queries):
        """CSR answer sets of `queries` through the dataset's AnswerIndex, (re)built when the dataset is another one"""
        from qrlsh import answers
        if self._answer_index is None or self._answer_index_key != id(self.dataset):
            cols = [self.dataset[f].to_numpy() for f in self.datasetFeatures]
            self._answer_index, self._answer_index_key = answers.build_answer_index(cols, self.device), id(self.dataset)
        return answers.answer_sets(self._answer_index, answers.encode_queries(self._answer_index, queries))

    def answer_sets(self):
        """host copy of answer_sets_device(): (offsets int64 [nq+1], rows int32 [nnz])"""
        off, rows = self.answer_sets_device()
        off, rows = ops.to_host(off), ops.to_host(rows)
        for q, n in enumerate(np.diff(off)):
            self.tupleCount[q] = int(n)      # recommender.py:93
        return off, rows

    def compute_shingles(self):
        """recommender.py:68-103: inverted index row -> [queries containing it]."""
        drows = self.dataset.shape[0]
        self._log("\nDataset : {}, Total queries: {}".format(drows, self.queriesIDs.size))
        initial = time.time()
        offsets, rows = self.answer_sets()
        shingles_dict = {d: [] for d in range(drows)}
        for q in range(self.queriesIDs.size):
            for ind in rows[offsets[q]:offsets[q + 1]]:
                shingles_dict[int(ind)].append(q)
        self._log(str(round(time.time() - initial, 3)) + "s for shingles_dict")
        return shingles_dict

    # ---- hot path ------------------------------------------------------------------
    def _device_inputs(self):
        offsets, rows = self.answer_sets_device()
        drows = self.dataset.shape[0]
        self._log("\nPermutations: {}".format(PERM))
        # PERM consecutive draws from the global legacy RNG, exactly as recommender.py:120
        cap = drows
        if self.row_capacity is not None:
            cap = int(self.row_capacity)
            if cap < drows:
                raise ValueError("row_capacity %d is below the dataset's %d rows" % (cap, drows))
        perms = ops.legacy_permutations(PERM, cap, rng=np.random)
        table = ops.perm_table(perms, self.device)
        return offsets, rows, table

    def compute_signatures(self):
        """(nq, PERM) int64 signature matrix (recommender.py:105-143)."""
        initial = time.time()
        offsets, rows, table = self._device_inputs()
        sig, _, _ = ops.minhash(offsets, rows, table, b=None, want_norm=False)
        out = ops.to_host(sig).astype(np.int64)
        self._log(str(round(time.time() - initial, 3)) + "s for signature_matrix")
        return out

    def _band_rule(self):
        if self.bands is not None:
            return self.bands
        for b in list(range(1, PERM + 1))[::-1]:
            if PERM % b == 0 and b % 10 == 0:
                r = PERM / b
                thresh = round((1 / b) ** (1 / r), 2)
                if thresh >= LSH_THRESH:
                    return b
        raise ValueError("no band count satisfies the rule of recommender.py:156-163 for PERM=%d "
                         "(the reference raises UnboundLocalError here); set Recommender.bands" % PERM)

    def compute_querySimilarities(self):
        """{q: {'indexes': int64[<=K], 'values': float64[<=K]}} (recommender.py:145-214)."""
        queryTime = time.time()
        nq = self.queriesIDs.size
        MAX_CANDIDATES = self.max_candidates if self.max_candidates is not None else round(math.log(nq, 1.5))
        self._log("\nQuery Thresh: " + str(LSH_THRESH))
        band = self._band_rule()
        offsets, rows, table = self._device_inputs()
        self._log("\nMax query candidates: {}, Max bands: {}, Band size: {}, Total queries: {}".format(
            MAX_CANDIDATES, band, PERM / band, nq))
        initial = time.time()
        res = pipeline.query_similarities(offsets, rows, table, band, MAX_CANDIDATES)
        torch.cuda.synchronize()
        self._log("Candidate pairs [{}s]: {}".format(round(time.time() - initial, 3), res.pairs.numel()))
        self.last_result = res
        self.last_table = table      # kept for serving new queries (similar_queries & co.)
        self._query_index = None
        self._live_table, self.row_slots = None, None      # row operations start afresh with the run
        query_sim = pipeline.sims_to_dict(res.src, res.dst, res.val)
        self._log("\n" + str(round(time.time() - queryTime, 3)) + "s for overall queries_similarity scores")
        return query_sim

    # ---- new queries: probes of the index of the last compute_querySimilarities run (device) ---------------------------
    def _run_index(self, tail, count=None, lists=False):
        """The QueryIndex of the last run, every live operation's way to it: made from the run's result on first need
        (with the run's lists, at the run's K) and bound there and then.  ValueError, in this order: no finished run
        ("... has not run: " + tail); count="queries" / "columns": an index that does not hold the served queries
        (/ the ratings' columns); lists=True: live lists that a call without update_lists=True dropped."""
        from qrlsh.index import QueryIndex
        if self.last_result is None or self.last_table is None:
            raise ValueError("compute_querySimilarities has not run: " + tail)
        if self._query_index is None:
            self._query_index = QueryIndex.from_result(self.last_result, self.last_table, lists=True)
        qi = self._query_index
        if count is not None:
            self._index_in_step(qi, columns=count == "columns")
        if lists and qi.lists is None:
            raise ValueError("the live lists were dropped by a call without update_lists=True; "
                             "compute_querySimilarities starts afresh")
        return qi

    def _index_in_step(self, qi, columns=False):
        if qi.n != self.queriesIDs.size or (columns and self.ratings.shape[1] != qi.n):
            raise ValueError("the index holds %d queries, the recommender %d" % (qi.n, self.queriesIDs.size))

    def _new_query_rows(self, queries, lists=False):
        """(index, sig, norm2, keys) of new queries given in parse_queries' form (one column per dataset feature,
        "" = unconstrained): answer sets through the cached AnswerIndex, MinHash under the run's own table.  lists=True
        refuses dropped live lists (_run_index) before the new texts reach the live table's dictionary."""
        qi = self._run_index("there is no index to look new queries up in", lists=lists)
        q = np.asarray(_as_numpy(queries), dtype=object)
        if q.ndim != 2 or q.shape[1] != len(self.datasetFeatures):
            raise ValueError("queries must have one column per dataset feature (%d)" % len(self.datasetFeatures))
        lt = self._live_table
        if lt is not None:          # rows have come or gone: the table in slot numbering answers
            offsets, rows = lt.answer_sets(lt.encode(q))
        else:
            offsets, rows = self._answer_sets_of(q)
        sig, norm2, keys = qi.signatures(offsets, rows)
        return qi, sig, norm2, keys

    @staticmethod
    def _ids_like(cur, ids, pos, what, name):
        """the labels of new entries of an id array `cur` (queriesIDs, usersIDs), kept in its kind: ids (default: the
        positions) as strings in a string-labelled set, integers only in an integer one, otherwise what converts to
        cur's dtype; ValueError for a wrong count or kind"""
        m = pos.size
        labels = pos if ids is None else np.asarray(ids)
        if labels.ndim != 1 or labels.size != m:
            raise ValueError("ids must hold one label per new %s (%d)" % (what, m))
        if cur.dtype.kind in "US":
            labels = labels.astype(str)           # a string-labelled set stays one: default labels are str(position)
        elif cur.dtype.kind in "iu":
            if labels.dtype.kind not in "iu":
                raise ValueError("ids of dtype %s do not fit %s of dtype %s" % (labels.dtype, name, cur.dtype))
        else:                                     # object, float, ...: labels (the positions by default) in that dtype
            try:
                labels = labels.astype(cur.dtype)
            except (TypeError, ValueError):
                raise ValueError("ids of dtype %s do not fit %s of dtype %s" % (labels.dtype, name, cur.dtype))
        return labels

    def _user_index_in_step(self, block=None):
        """self.user_index when it holds self.ratings' shape now (it then follows the column operation under way), else
        None: an index that is already out of step is left alone.  A ratings block the index would refuse is refused
        here, before the query index takes the batch."""
        ui = self.user_index
        if ui is None or (ui.nu, ui.nq) != tuple(self.ratings.shape):
            return None
        if block is not None and block.size and (block.min() < 0 or block.max() >= 2**31):
            raise ValueError("ratings must lie in [0, 2^31) while a user index follows them")
        return ui

    def add_queries(self, queries, ratings=None, ids=None, update_lists=False):
        """Take m new queries (parse_queries' form) into the served set without a new run: their answer sets and
        signatures under the last run's table are appended to the run's index (QueryIndex.append: no rebuild), and
        self.queries, self.queriesIDs and self.ratings grow by the same m.  ratings: integer [users, m] block of their
        ratings (default: zeros, nothing rated); ids: their labels (default: their positions).  queriesIDs keeps
        its kind: in a string-labelled set (parse_queries' ids) labels are stored as strings, the default ones as
        str(position); integer queriesIDs take integer labels only, any other dtype (object, float) takes what
        converts to it (ValueError otherwise).  -> int64 [m], the
        positions assigned.  Afterwards similar_queries, predict_new_queries and recommend_new_queries see them as
        indexed queries.  last_result stays the closed-set run's output; the next compute_querySimilarities starts
        afresh over all queries.  (Nothing per query is cached on the device between calls: the cached AnswerIndex
        belongs to the dataset and stays.)
        update_lists=True: the index also keeps the run's top-K lists current (QueryIndex.append(update_lists=True)):
        current_query_similarities() then returns what compute_querySimilarities would over all queries at the run's
        K, and compute_scores(reuse_lists=True) predicts from them.  last_result is still left alone.  Without the flag
        the live lists are dropped (they would be stale), and a later update_lists=True raises ValueError before anything
        changes (the live table's dictionary included).
        A user index in step with self.ratings (live_user_similarities) follows, whatever update_lists says:
        UserLists.add_columns takes the block (m unrated columns without one), so rate, recommend_users and
        predict_users keep serving from it."""
        qi, sig, norm2, keys = self._new_query_rows(queries, lists=update_lists)
        q = np.asarray(_as_numpy(queries), dtype=object)
        m = q.shape[0]
        nu = self.usersIDs.size
        block = np.zeros((nu, m), dtype=np.int64) if ratings is None else _ratings_block(ratings, nu, m)
        self._index_in_step(qi, columns=True)
        pos = np.arange(qi.n, qi.n + m, dtype=np.int64)
        cur = self.queriesIDs
        labels = self._ids_like(cur, ids, pos, "query", "queriesIDs")
        ui = self._user_index_in_step(None if ratings is None else block)
        qi.append(sig, norm2, keys, update_lists=update_lists)
        if self._live_table is not None:
            self._live_table.add_queries(self._live_table.encode(q))
        if ui is not None:
            ui.add_columns(m if ratings is None else block)
        self.queries = np.concatenate((np.asarray(self.queries, dtype=object), q), axis=0)
        self.queriesIDs = np.concatenate((cur, labels))
        self.ratings = np.hstack((self.ratings, block))
        return pos

    def remove_queries(self, positions, update_lists=False):
        """Take queries out of the served set without a new run, the mirror of add_queries: positions (integers, any
        order, duplicates allowed; ValueError for one outside the set, nothing changed) leave self.queries,
        self.queriesIDs, self.ratings and the run's index (QueryIndex.remove: no rebuild), and the queries left are
        renumbered by rank.  -> int64 host array [old count]: the new position of every old one, -1 for a removed one.
        update_lists=True: the index keeps the run's top-K lists exact (QueryIndex.remove(update_lists=True)), so
        current_query_similarities() and compute_scores(reuse_lists=True) serve the shrunk set at the run's K.  Without
        the flag the live lists are dropped, and a later update_lists=True raises ValueError.  last_result stays the
        closed-set run's output.  A user index in step with self.ratings follows (UserLists.remove_columns), whatever
        update_lists says."""
        qi = self._run_index("there is no index to take queries out of", count="columns", lists=update_lists)
        pos = _positions(positions)
        ui = self._user_index_in_step()
        new_pos = ops.to_host(qi.remove(pos, update_lists=update_lists))
        if self._live_table is not None:
            self._live_table.remove_queries(new_pos)
        if ui is not None:
            ui.remove_columns(pos)
        keep = new_pos >= 0
        self.queries = np.asarray(self.queries, dtype=object)[keep]
        self.queriesIDs = self.queriesIDs[keep]
        self.ratings = np.ascontiguousarray(self.ratings[:, keep])
        return new_pos

    def replace_queries(self, positions, queries, ratings=None, update_lists=False):
        """Give served queries new texts without a new run: queries (parse_queries' form, one per position) go through
        the same answer-set and signature route as add_queries and overwrite self.queries[positions] and the rows of
        the run's index (QueryIndex.replace: no rebuild, no renumbering).  positions: distinct integers in any order
        (ValueError for a duplicate or one outside the set, nothing changed).  queriesIDs stay.  ratings=None keeps the
        ratings columns -- an edited query keeps its ratings; an integer [users, m] block overwrites them.
        update_lists=True: the index keeps the run's top-K lists exact (QueryIndex.replace(update_lists=True)), so
        current_query_similarities(), compute_scores(reuse_lists=True) and recommend_users serve the edited set at the
        run's K.  Without the flag the live lists are dropped, and a later update_lists=True raises ValueError
        before anything changes.  last_result stays the closed-set run's output.  With a ratings block, a user index in step with self.ratings
        follows (UserLists.set_columns), whatever update_lists says; without one it is not touched."""
        qi, sig, norm2, keys = self._new_query_rows(queries, lists=update_lists)
        self._index_in_step(qi, columns=True)
        q = np.asarray(_as_numpy(queries), dtype=object)
        m = q.shape[0]
        pos = _positions(positions, distinct=(m, qi.n))
        block = None if ratings is None else _ratings_block(ratings, self.usersIDs.size, m)
        ui = self._user_index_in_step(block) if block is not None else None
        qi.replace(pos, sig, norm2, keys, update_lists=update_lists)
        if self._live_table is not None:
            self._live_table.set_queries(pos, self._live_table.encode(q))
        if ui is not None:
            ui.set_columns(pos, block)
        self.queries = np.array(np.asarray(self.queries, dtype=object), copy=True)
        self.queries[pos] = q
        if block is not None:
            self.ratings = np.array(self.ratings, copy=True)
            self.ratings[:, pos] = block.astype(self.ratings.dtype)

    # ---- dataset rows come and go (qrlsh.LiveTable) ------------------------------------------------------------------
    def _live_rows(self, update_lists):
        """(LiveTable, QueryIndex) of the last run; the table is built on first use from self.dataset (slot = position),
        self.queries and the run's permutation table (its rows are the capacity)"""
        from qrlsh.table import LiveTable
        qi = self._run_index("there is no index for rows to come and go under", count="queries", lists=update_lists)
        if self._live_table is None:
            if len(self.datasetFeatures) > 63:
                raise ValueError("rows come and go under at most 63 dataset features, got %d" % len(self.datasetFeatures))
            cols = [self.dataset[f].to_numpy() for f in self.datasetFeatures]
            self._live_table = LiveTable.build(cols, self.queries, capacity=self.last_table.D, device=self.device)
            self.row_slots = np.arange(self.dataset.shape[0], dtype=np.int64)
        return self._live_table, qi

    def add_rows(self, rows, update_lists=False):
        """Take m new tuples into the dataset without a new run: rows = a frame or array with one column per entry of
        datasetFeatures (a frame that names all of self.dataset's columns is appended whole; otherwise the other columns
        get "").  Each row takes a free slot of the run's permutation table (row_capacity), the served queries whose
        signature it lowers get their new rows through qrlsh.LiveTable.add_rows / QueryIndex.replace, and self.dataset
        grows by the m rows (index reset); self.row_slots holds the slot of every dataset position.  update_lists as
        replace_queries treats it -- except that a batch that changes no query leaves the index and its lists alone.
        ValueError, nothing changed: no finished run, a wrong column count, or fewer than m free slots (raise
        row_capacity before the run).  -> int64 [m], the positions assigned in self.dataset."""
        feats = list(self.datasetFeatures)
        if isinstance(rows, pd.DataFrame) or hasattr(rows, "to_pandas"):
            frame = _as_pandas(rows).astype(str)
            if not all(f in frame.columns for f in feats):
                if frame.shape[1] != len(feats):
                    raise ValueError("rows must have one column per dataset feature (%d)" % len(feats))
                frame.columns = feats
        else:
            a = np.asarray(rows, dtype=object)
            if a.ndim != 2 or a.shape[1] != len(feats):
                raise ValueError("rows must have one column per dataset feature (%d)" % len(feats))
            frame = pd.DataFrame(a, columns=feats).astype(str)
        lt, qi = self._live_rows(update_lists)
        m = frame.shape[0]
        if lt.D + m > lt.capacity:
            raise ValueError("%d rows for %d free slots: row_capacity (%d) must be raised before the run"
                             % (m, lt.capacity - lt.D, lt.capacity))
        slots = lt.add_rows(frame[feats].to_numpy(), qi, update_lists=update_lists)
        first = self.dataset.shape[0]
        self.dataset = pd.concat((self.dataset, frame.reindex(columns=self.dataset.columns, fill_value="")),
                                 ignore_index=True)
        self.row_slots = np.concatenate((self.row_slots, slots))
        return np.arange(first, first + m, dtype=np.int64)

    def remove_rows(self, positions, update_lists=False):
        """Take tuples out of the dataset without a new run, under remove_queries' contract: positions in the current
        self.dataset (integers, any order, duplicates allowed; ValueError for one outside, nothing changed).  Their slots
        die, the served queries whose minimum sat on one of them get their answer sets taken again
        (qrlsh.LiveTable.remove_rows / QueryIndex.set), and self.dataset keeps the live rows only (index reset).
        -> int64 host array [old rows]: the new position of every old one, -1 for a removed one."""
        pos = _positions(positions)
        lt, qi = self._live_rows(update_lists)
        drows = self.dataset.shape[0]
        pos = _positions(pos, below=drows)
        lt.remove_rows(self.row_slots[pos], qi, update_lists=update_lists)
        keep = np.ones(drows, dtype=bool)
        keep[pos] = False
        self.dataset = self.dataset[keep].reset_index(drop=True)
        self.row_slots = self.row_slots[keep]
        return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)

    def _live_lists(self):
        """(src, dst, val) that know every added query, or None: the run's own lists before any append, the index's
        while add_queries(update_lists=True) kept them current"""
        res, qi = self.last_result, self._query_index
        if res is None:
            return None
        if qi is None:
            return (res.src, res.dst, res.val) if res.sig.shape[0] == self.queriesIDs.size else None
        return qi.lists if qi.n == self.queriesIDs.size else None

    def _lists_or_refuse(self, lists=None):
        """a caller's triple (_lists_or_live) or the live lists; ValueError when there are none"""
        lists = self._lists_or_live(lists)
        if lists is None:
            raise ValueError("there are no live lists: run compute_querySimilarities, and add queries with update_lists=True")
        return lists

    def _sum_order(self, sum_order):
        """the checked summation order of a serving call (None: self.sum_order)"""
        sum_order = self.sum_order if sum_order is None else sum_order
        sum_order_code(sum_order)
        return sum_order

    def current_query_similarities(self):
        """the dict compute_querySimilarities returns, from the live lists: before any add_queries the run's own, after
        add_queries(update_lists=True) those of all queries served now (list length: the run's K).  ValueError when
        there are none (no run yet, or an add_queries without update_lists dropped them)."""
        return pipeline.sims_to_dict(*self._lists_or_refuse())

    def similar_queries(self, queries):
        """{x: {'indexes': int64[<=K], 'values': float64[<=K]}} for new queries x = 0 .. m-1 (rows of `queries`): the
        indexed queries each would get as neighbours if appended alone (K of the last run; value descending, then id
        ascending); queries without candidates are absent, as in compute_querySimilarities."""
        qi, sig, norm2, keys = self._new_query_rows(queries)
        off, idx, milli, _ = qi.neighbours(sig, norm2, keys)
        off, idx, milli = ops.to_host(off), ops.to_host(idx), ops.to_host(milli)
        out = {}
        for x in range(len(off) - 1):
            if off[x + 1] > off[x]:
                out[x] = {"indexes": idx[off[x]:off[x + 1]].astype(np.int64),
                          "values": milli[off[x]:off[x + 1]].astype(np.float64) / 1000.0}
        return out

    def _new_query_columns(self, queries, sum_order):
        sum_order = self._sum_order(sum_order)
        qi, sig, norm2, keys = self._new_query_rows(queries)
        off, idx, milli, _ = qi.neighbours(sig, norm2, keys)
        return qi.predict_columns(self.ratings, off, idx, milli, sum_order, self.query_weight, self.user_weight,
                                  self.default_mean)

    def predict_new_queries(self, queries, sum_order=None):
        """DataFrame usersIDs x new queries (0 .. m-1): the prediction compute_scores would give each user's cell of a
        new query appended as an unrated column (recommender.py:313-331; its user side is 0)."""
        final = ops.to_host(self._new_query_columns(queries, sum_order)).T
        return pd.DataFrame(final, index=self.usersIDs, columns=range(final.shape[1])).astype(int)

    def recommend_new_queries(self, queries, k, sum_order=None):
        """{x: {'users': int64[user rows, 0-based], 'values': int64[predicted values], 'available': int}}: per new query
        the k users with the largest non-zero predictions (value descending, then user ascending) and how many users
        have one."""
        from qrlsh import recommend as rec
        from qrlsh.index import QueryIndex
        k = _int_in(k, "k", 1, rec.MAX_K)
        users, vals, avail = QueryIndex.top_users(self._new_query_columns(queries, sum_order), k)
        return _served(None, users, vals, avail, k, "users")

    # ---- N4: user similarity (clustering = the reference's sklearn call on the host; the rest on the device) ----
    def compute_userSimilarities(self):
        """{u: {'indexes', 'values'}} (recommender.py:216-290): StandardScaler -> PCA -> BIRCH (scikit-learn, as
        in the reference), then on the device the centred cosine inside each cluster (with the reference's
        integer truncation of the centred rows); the per-user cut is the reference's own numpy call
        (np.argsort(row)[::-1][:K], :282) on those scores, so the lists -- tie order and zero-valued entries
        included -- are the reference's.  qrlsh.users.user_similarities is the all-device variant with a
        defined tie order (value descending, id ascending) for sizes where a host loop per user is not wanted."""
        return self._user_similarities_over(self.ratings)

    def _user_similarities_over(self, ratings):
        """compute_userSimilarities over `ratings` (host integers, one row per entry of usersIDs): self.ratings, or the
        train matrix of evaluate(holdout=True)"""
        from qrlsh import users
        t0 = time.time()
        nu = self.usersIDs.size
        top = round(math.log(nu, 1.5))
        n_clusters = round(nu ** (1 / 1.3))
        self._log("\nMax user candidates: {}, Total users: {}".format(top, nu))
        self._log("\nCluster count: {}, Total users: {}".format(n_clusters, nu))
        # StandardScaler + PCA on the device (Gram matrix on the matrix cores), BIRCH by the reference's own
        # scikit-learn call; cluster_on_device = False: the whole clustering on the host, as the reference runs it
        label = users.cluster_labels(ratings, device=self.device if self.cluster_on_device else None)
        pairs, milli = users.cluster_pair_scores(ratings, label, self.device)
        user_sim = users.reference_cut(pairs, milli, label, top)
        self._log("\n" + str(round(time.time() - t0, 3)) + "s for overall users_similarity scores")
        return user_sim

    # ---- user lists that follow the ratings (qrlsh.UserLists) -------------------------------------------------------
    def live_user_similarities(self, labels=None, K=None):
        """Build self.user_index (qrlsh.UserLists) over self.ratings: the all-device user lists (value descending, then
        id ascending; positive values only) at list length K (default round(log_1.5 users)), which rate() then keeps
        exact without a recompute, add_queries / remove_queries / replace_queries keep in step with the served
        queries (UserLists.add_columns / remove_columns / set_columns), and add_users / remove_users with the served users.  labels: cluster ids per user, held fixed from here on (default:
        users.cluster_labels, on the device when cluster_on_device).  While the index exists, recommend_users and
        predict_users called without user_sim / ratings serve from it.  -> self.user_index"""
        from qrlsh import users
        from qrlsh.userlists import UserLists
        if labels is None:
            labels = users.cluster_labels(self.ratings, device=self.device if self.cluster_on_device else None)
        self.user_index = UserLists.build(np.asarray(self.ratings), labels, K=K, device=self.device)
        return self.user_index

    def add_users(self, ratings, ids=None, labels=None):
        """Take m new users into the served set without a rebuild: ratings = integer [m, queries] block of their
        ratings; ids: their entries of usersIDs, under the dtype rule add_queries applies to queriesIDs (default: their
        positions).  self.usersIDs and self.ratings grow by the same m.  A user index in step with self.ratings
        (live_user_similarities) follows (UserLists.add_users): labels = one cluster label per new user in the label
        space the index was built with, or None -- each joins the cluster of the existing user it is most similar to,
        or gets a cluster of its own where no similarity is positive.  Afterwards rate, recommend_users and
        predict_users serve the new user set from the index.  An index that is out of step is left alone (labels then
        go unused); the query side is not touched -- its lists do not depend on ratings.  ValueError for a wrong shape,
        a non-integer block, a value the index refuses or a wrong id count or kind (nothing changed).
        -> int64 [m], the positions assigned."""
        nu, nq = self.ratings.shape
        block = _ratings_block(ratings, None, nq)
        m = block.shape[0]
        pos = np.arange(nu, nu + m, dtype=np.int64)
        new_ids = self._ids_like(self.usersIDs, ids, pos, "user", "usersIDs")
        ui = self._user_index_in_step(block)
        if ui is not None:
            ui.add_users(block, labels=labels)
        self.usersIDs = np.concatenate((self.usersIDs, new_ids))
        self.ratings = np.vstack((self.ratings, block.astype(self.ratings.dtype)))
        return pos

    def remove_users(self, positions):
        """Take users out of the served set without a rebuild, the mirror of add_users: positions (integers, any order,
        duplicates allowed; ValueError for one outside the set or when nobody would be left, nothing changed) leave
        self.usersIDs and self.ratings, and the users left are renumbered by rank.  A user index in step with
        self.ratings follows (UserLists.remove_users: the lists stay exact); one out of step is left alone.
        -> int64 host array [old count]: the new position of every old one, -1 for a removed one."""
        nu = self.usersIDs.size
        pos = _positions(positions, below=nu)
        if pos.size >= nu:
            raise ValueError("no user would be left")
        ui = self._user_index_in_step()
        if ui is not None:
            ui.remove_users(pos)
        keep = np.ones(nu, dtype=bool)
        keep[pos] = False
        self.usersIDs = self.usersIDs[keep]
        self.ratings = np.ascontiguousarray(self.ratings[keep])
        return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)

    def rate(self, users, queries, values):
        """"user u rated query q": users / queries are 0-based positions, values the new ratings (0 = unrate; repeats
        of one cell keep the last).  Edits self.ratings and self.user_index (UserLists.rate: the lists of the touched
        clusters are brought up to date, nothing is recomputed).  ValueError when live_user_similarities has not built
        an index, for a position outside range or a negative value (nothing changed), and for an index that fell out of
        step with self.ratings (add_queries, remove_queries and replace_queries keep an index in step that was in step
        when they were called).  -> rows of the lists rewritten"""
        ui = self.user_index
        if ui is None:
            raise ValueError("there is no user index: call live_user_similarities first")
        if ui.nu != self.ratings.shape[0] or ui.nq != self.ratings.shape[1]:
            raise ValueError("the user index holds a %d x %d matrix, the recommender %d x %d (queries were added or "
                             "removed: call live_user_similarities again)" % ((ui.nu, ui.nq) + tuple(self.ratings.shape)))
        n = ui.rate(users, queries, values)
        u, q, v = (np.asarray(ops.to_host(a)).reshape(-1).astype(np.int64) for a in (users, queries, values))
        self.ratings[u, q] = v.astype(self.ratings.dtype)       # numpy assigns in order: the last repeat wins here too
        return n

    # ---- the list lengths of the live lists, changed in place ------------------------------------------------------
    def _cut_plan(self, q_cut, u_cut):
        """What tune(apply_cuts=True) does with the best setting's cuts (None: that side's cuts were not given):
        -> (query_K, user_K) for set_list_lengths, None for a side left alone -- one whose best cut is >= its current
        length (tune never regrows).  ValueError before anything changes: a best cut of 0 (a side switched off is not a
        list length), or a user cut without a user index in step."""
        query_K = user_K = None
        if q_cut is not None:
            if q_cut < 1:
                raise ValueError("the best setting switches the query side off (cut 0): a list length is >= 1, nothing applied")
            qi = self._run_index("there are no lists to change")
            if qi.lists is not None and q_cut < qi.lists_K:
                query_K = int(q_cut)
        if u_cut is not None:
            if u_cut < 1:
                raise ValueError("the best setting switches the user side off (cut 0): a list length is >= 1, nothing applied")
            ui = self._user_index_in_step()
            if ui is None:
                raise ValueError("a user cut needs a user index in step with self.ratings (live_user_similarities)")
            if u_cut < ui.K:
                user_K = int(u_cut)
        return query_K, user_K

    def set_list_lengths(self, query_K=None, user_K=None):
        """Change the list length of the live lists in place, without a run: query_K (1..256) goes to the run's index
        (QueryIndex.set_list_length; the index is made from the last run's result if absent, as add_queries does),
        user_K (1..64) to the user index (UserLists.set_list_length), which must be in step with self.ratings.  None
        leaves a side alone.  Afterwards the lists are element for element those of a full run / build at the new
        lengths, and everything that serves or measures from them does so at those lengths: current_query_similarities,
        compute_scores(reuse_lists=True), recommend_users, predict_users, evaluate*, tune*, add_queries / remove_queries
        / replace_queries(update_lists=True), rate, add_users, remove_users and the row operations.  A smaller length
        cuts; a larger one probes (rescores) the rows the old length had filled.  last_result is left alone.
        ValueError before anything changes: a length outside range, no finished run, no live lists, an index that does
        not hold the served queries, or user_K without a user index in step.
        -> (query rows probed again, user rows rescored), None for a side left alone."""
        from qrlsh.index import MAX_K
        from qrlsh.userlists import MAX_K as USER_MAX_K
        qi = ui = None
        if query_K is not None:
            query_K = _int_in(query_K, "query_K", 1, MAX_K)
            qi = self._run_index("there are no lists to change", count="queries", lists=True)
        if user_K is not None:
            user_K = _int_in(user_K, "user_K", 1, USER_MAX_K)
            ui = self._user_index_in_step()
            if ui is None:
                raise ValueError("user_K needs a user index in step with self.ratings (live_user_similarities)")
        picked_q = picked_u = None
        if qi is not None:
            picked_q = qi.set_list_length(query_K)      # raises before it changes anything
        if ui is not None:
            picked_u = ui.set_list_length(user_K)
        return picked_q, picked_u

    # ---- N1: hybrid prediction (device) ------------------------------------------------
    def compute_scores(self, reuse_lists=False):
        """(scores_to_predict, finalPredictions DataFrame, scores_missed), recommender.py:292-343.
        reuse_lists=True with live lists present (current_query_similarities): the query side comes from them instead
        of from a new compute_querySimilarities run; the user side and the prediction are unchanged.  Without live
        lists, and by default, the run happens as always."""
        from qrlsh import predict
        self._log("\n========== QUERY SIMILARITY ==========")
        lists = self._live_lists() if reuse_lists else None
        if lists is None:
            self.compute_querySimilarities()
            res = self.last_result
            lists = (res.src, res.dst, res.val)
        self._log("\n========== USER SIMILARITY ==========")
        user_sim = self.compute_userSimilarities()
        self._log("\n========== WEIGHTED AVERAGES ==========")
        t0 = time.time()
        scores_to_predict = np.array(np.where(self.ratings == 0)).T
        # weighted_average (recommender.py:36) is @jit(nopython=True): where the reference runs as shipped
        # (requirements.txt: numba) its np.sum is ONE accumulator in index order -> sum_order "sequential" (default).
        # "pairwise" is numpy's own np.sum order, what the reference does with @jit removed -- the run the committed
        # fixtures were captured from (numba is not installable here), on which both orders give the same matrices;
        # parity with the numba build itself stays unpinned.
        final = predict.fill_predictions(self.ratings, lists[0], lists[1], lists[2], user_sim, self.query_weight,
                                         self.user_weight, self.default_mean, self.device, sum_order=self.sum_order)
        final = ops.to_host(final)
        self._log(str(round(time.time() - t0, 3)) + "s for weighted averages")
        finalPredictions = pd.DataFrame(final, columns=self.queriesIDs, index=self.usersIDs).astype(int)
        scores_missed = np.array(np.where(finalPredictions == 0)).T
        return scores_to_predict, finalPredictions, scores_missed

    # ---- recommendations (device): the selection of top_k_queries for many users at once --------------------------
    def recommend(self, predictions, k, users=None):
        """Top-k unrated queries of each requested user (default: every user), the batch form of the selection in
        top_k_queries (recommender.py:357-375) on the device.  predictions: compute_scores' DataFrame, or an array /
        tensor of the same shape; the unrated cells are those of self.ratings.
        -> {u: {'indexes': int64[query columns, 0-based], 'values': int64[predicted values], 'available': int}}: the
        eligible queries (unrated, non-zero prediction: just_scored of :361) with the largest values, value
        descending then index ascending (the reference's order among equal values is np.argsort's, arbitrary);
        'available' = len(just_scored), the prompt's [Max: N].  Raises ValueError for a bad k, shape or user id."""
        from qrlsh import recommend as rec
        pred = predictions.to_numpy() if hasattr(predictions, "to_numpy") else predictions
        users = _ids_arg(users)
        idx, val, avail = rec.top_k(self.ratings, pred, k, users=users, device=self.device)
        return _served(users, idx, val, avail, k, "indexes")

    # ---- serving chosen users from the live lists: no prediction matrix -------------------------------------------
    def _lists_or_live(self, lists):
        """a caller's (src, dst, milli) triple covering all served queries (e.g. ExactLists.coo()), or (None) the live lists"""
        if lists is None:
            return self._live_lists()
        lists = tuple(lists)
        if len(lists) != 3:
            raise ValueError("lists must be a (src, dst, milli) triple")
        return lists

    def _serving_inputs(self, sum_order, user_sim, ratings, lists=None):
        lists, sum_order = self._lists_or_refuse(lists), self._sum_order(sum_order)
        ui = self.user_index
        if ui is not None and user_sim is None and ratings is None and (ui.nu, ui.nq) == tuple(self.ratings.shape):
            return lists, sum_order, ui.as_user_sims(), ui.ratings   # the live user lists and their device matrix
        if user_sim is None:
            user_sim = self.compute_userSimilarities()
        return lists, sum_order, user_sim, self.ratings if ratings is None else ratings

    def recommend_users(self, users, k, sum_order=None, user_sim=None, ratings=None, lists=None):
        """recommend(compute_scores(reuse_lists=True)[1], k, users) for the requested users only, without the
        prediction of every user's row: the query side comes from the live lists (current_query_similarities; ValueError
        when there are none), so the answer is current after add_queries / remove_queries(update_lists=True).
        lists: a (src, dst, milli) triple covering all served queries, used in place of the live lists (e.g.
        exact_query_lists().coo()); None = the live lists.
        user_sim: compute_userSimilarities' dict or qrlsh.user_lists' prepared tuple (default: computed here);
        ratings: the utility matrix where the caller holds it, e.g. its device copy (default: self.ratings).
        -> the dict recommend() returns.  Raises ValueError for a bad k, sum_order or user id."""
        from qrlsh import recommend as rec
        k, users = _int_in(k, "k", 1, rec.MAX_K), _ids_arg(users)
        lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, ratings, lists)
        idx, val, avail = rec.for_users(ratings, lists[0], lists[1], lists[2], user_sim, users, k,
                                        sum_order=sum_order, query_weight=self.query_weight,
                                        user_weight=self.user_weight, default_mean=self.default_mean,
                                        device=self.device)
        return _served(users, idx, val, avail, k, "indexes")

    def recommend_users_diverse(self, users, k, penalty=None, max_sim=None, pool=None, sum_order=None, user_sim=None,
                                ratings=None):
        """recommend_users with the lists reranked on the device by the live neighbour lists (qrlsh.for_users_diverse):
        from each user's `pool` best candidates (default min(1024, max(4 k, 64))) the k are picked greedily by
        1000 * value - penalty * r, r = the largest stored similarity (milli) to a query already picked; candidates
        with r >= max_sim are left out (1001: none is).  penalty / max_sim = None: self.diversity_penalty /
        self.diversity_max_sim (0 and 1001, the plain list, until tune_diversity(apply=True) sets them).  The remaining
        arguments as recommend_users takes them.
        -> recommend_users' dict with 'redundancy' added: int64, the r each listed query had when it was picked (the
        lists can be shorter than min(k, available) when max_sim excludes).  Raises ValueError for a bad k, pool,
        penalty, max_sim, sum_order or user id."""
        dv = _diversify()
        penalty = self.diversity_penalty if penalty is None else penalty
        max_sim = self.diversity_max_sim if max_sim is None else max_sim
        k, penalty, max_sim = dv._check_rule(k, penalty, max_sim)
        pool = dv._check_pool(k, pool)
        users = _ids_arg(users)
        lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, ratings)
        idx, val, red, count, avail = dv.for_users_diverse(
            ratings, lists[0], lists[1], lists[2], user_sim, users, k, pool=pool, penalty=penalty, max_sim=max_sim,
            sum_order=sum_order, query_weight=self.query_weight, user_weight=self.user_weight,
            default_mean=self.default_mean, device=self.device)
        return _served(users, idx, val, avail, count, "indexes", redundancy=red)

    def list_redundancy(self, recs):
        """How redundant served lists are, by the live neighbour lists: recs is a dict recommend / recommend_users /
        recommend_users_diverse returned.  -> qrlsh.Redundancy: .words[i] = (entries, in-list pairs of stored
        neighbours, the sum of their similarities in milli, the largest) for the i-th user of the dict, .totals,
        .pairs_per_list, .mean_sim."""
        lists = self._lists_or_refuse()
        rows = [np.asarray(r["indexes"], dtype=np.int64) for r in recs.values()]
        idx = np.full((len(rows), max([len(r) for r in rows] + [1])), -1, dtype=np.int64)
        for i, r in enumerate(rows):
            idx[i, :len(r)] = r
        return _diversify().list_redundancy(idx, lists[0], lists[1], lists[2], int(self.queriesIDs.size),
                                            device=self.device)

    # ---- how good are the lists themselves: the exact answer-set overlap (qrlsh.fidelity) ----------------------------
    def _answer_set_inputs(self):
        """(offsets, rows, D) as served now: the answer sets from the live table in slot numbering once rows have come or
        gone, otherwise through the cached AnswerIndex"""
        lt = self._live_table
        if lt is not None:
            offsets, rows = lt.answer_sets()
            return offsets, rows, int(lt.D)
        offsets, rows = self.answer_sets_device()
        return offsets, rows, int(self.dataset.shape[0])

    def _fidelity_inputs(self):
        """(offsets, rows, D, lists, K of the lists) as served now"""
        lists = self._lists_or_refuse()
        offsets, rows, D = self._answer_set_inputs()
        qi = self._query_index
        K = int(qi.lists_K) if qi is not None else int(self.last_result.K)
        return offsets, rows, D, lists, K

    def list_fidelity(self, positions=None, sample=1024, seed=0, K=None, lists=None):
        """How many of a query's true nearest neighbours -- by Jaccard over the answer sets, the quantity MinHash
        estimates -- does its served list hold?  -> qrlsh.ListFidelity (.recall, .sure_recall, .disjoint_share,
        .inversion_share, .per_request, .entries, .totals) over the live lists and the answer sets as served now, so
        current after add_queries / remove_queries / replace_queries(update_lists=True), add_rows / remove_rows and
        set_list_lengths; nothing is modified.  positions: 0-based queries (any order; a host sequence or a device
        tensor), None = `sample` of them drawn by `seed` (qrlsh.fidelity.sample_positions; all when sample >= their
        number).  K: the list length to judge, 1..64 (the first min(len, K) entries of every row), None = the lists' own.
        lists: a (src, dst, milli) triple covering all served queries, judged in place of the live lists (which are then
        not needed); K is required with it.
        ValueError when there are no live lists, for a bad K, sample, seed or position, and for more than 2^20 table rows."""
        from qrlsh import fidelity as fd
        if lists is None:
            offsets, rows, D, lists, own_K = self._fidelity_inputs()
        else:
            if K is None:
                raise ValueError("K is required with lists: they carry no list length of their own")
            lists, own_K = self._lists_or_live(lists), K
            offsets, rows, D = self._answer_set_inputs()
        nq = int(self.queriesIDs.size)
        K = _int_in(own_K if K is None else K, "K", 1, fd.MAX_K)
        if positions is None:
            positions = fd.sample_positions(nq, sample, seed)
        return fd.list_fidelity(offsets, rows, D, lists[0], lists[1], lists[2], nq, K, queries=_ids_arg(positions),
                                device=self.device)

    def edge_overlaps(self):
        """The exact overlap of every stored edge of the live lists -> (src, dst, val, inter) int32 device tensors and
        sizes int64 device tensor [queries]: inter[e] = |A(src[e]) & A(dst[e])| and sizes[q] = |A(q)|, so Jaccard of edge e
        is inter / (sizes[src] + sizes[dst] - inter) beside its stored val (milli).  Current after every live operation;
        nothing is modified.  ValueError when there are no live lists."""
        from qrlsh import fidelity as fd
        offsets, rows, _, lists, _ = self._fidelity_inputs()
        inter = fd.edge_overlaps(offsets, rows, lists[0], lists[1], device=self.device)
        return lists[0], lists[1], lists[2], inter, offsets[1:] - offsets[:-1]

    def answer_postings(self):
        """The row -> queries index of the answer sets as served now -> qrlsh.AnswerPostings, built on the device from the
        CSR every other call here reads (current after every live operation).  Nothing is kept on the instance: postings
        held across add_queries / remove_queries / replace_queries, add_rows or remove_rows are the caller's, and
        exact_query_lists refuses them once the shape of the answer sets has moved (queries, entries or table rows).
        Held postings whose shape still fits -- a replace_queries whose new answer sets have the same total size --
        are NOT refused: every position is then served from the old lists with wrong numbers and no error.  Rebuild
        after every live operation, or pass postings=True."""
        from qrlsh import postings as po
        offsets, rows, D = self._answer_set_inputs()
        return po.answer_postings(offsets, rows, D, device=self.device)

    def exact_query_lists(self, K=None, positions=None, postings=None):
        """The exact neighbour lists of the queries as served now -> qrlsh.ExactLists (.dst, .inter, .union, .listed,
        .positives, .coo()): per requested position the top K queries by Jaccard over the answer sets, J descending,
        ties by position ascending -- what list_fidelity holds the served lists to.  Read from the answer sets as they
        stand, so current after add_queries / remove_queries / replace_queries, add_rows and remove_rows; nothing is
        modified and NOTHING IS INSTALLED: the live lists stay the LSH lists (QueryIndex would maintain installed lists by
        LSH from the next operation on).  .coo() is the `lists` argument of evaluate, evaluate_ranking, recommend_users
        and list_fidelity when positions is None.  K: 1..64, None = the live lists' own (ValueError when there are none);
        positions: 0-based queries (any order; a host sequence or a device tensor), None = all -- every query against
        every query: by the sweep (postings=None) minutes at 10 M queries.
        postings: None = the sweep over all queries; True = build the row -> queries index for this call
        (answer_postings()) and serve every request from the posting lists of its own rows, the same lists word for
        word at a cost that follows the matches; a qrlsh.AnswerPostings = used as given (ValueError when its shape is no
        longer that of the answer sets; held postings of the same shape are NOT refused, whatever changed -- see
        answer_postings()).
        ValueError for a bad K or position and for more than 2^20 table rows."""
        from qrlsh import exactlists as el
        from qrlsh import fidelity as fd
        if K is None:
            K = self._fidelity_inputs()[4]
        K = _int_in(K, "K", 1, fd.MAX_K)
        offsets, rows, D = self._answer_set_inputs()
        if int(offsets.numel()) - 1 != int(self.queriesIDs.size):
            raise ValueError("the answer sets cover %d queries, %d are served" % (int(offsets.numel()) - 1,
                                                                               int(self.queriesIDs.size)))
        if postings is True:
            from qrlsh import postings as po
            postings = po.answer_postings(offsets, rows, D, device=self.device)
        elif postings is False:
            postings = None
        return el.exact_neighbours(offsets, rows, D, K, queries=_ids_arg(positions), device=self.device,
                                   postings=postings)

    def predict_users(self, users, sum_order=None, user_sim=None, ratings=None):
        """DataFrame requested users x queriesIDs: their rows of compute_scores(reuse_lists=True)'s finalPredictions,
        from the live lists (arguments as recommend_users takes them)."""
        from qrlsh import predict
        users = _ids_arg(users)
        lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, ratings)
        rows = predict.predict_users(ratings, lists[0], lists[1], lists[2], user_sim, users, self.query_weight,
                                     self.user_weight, self.default_mean, self.device, sum_order=sum_order)
        ids = np.arange(self.usersIDs.size) if users is None else np.asarray(ops.to_host(users), dtype=np.int64)
        return pd.DataFrame(ops.to_host(rows), index=self.usersIDs[ids], columns=self.queriesIDs).astype(int)

    # ---- serving chosen queries from the live lists: their audience, their columns, their utility --------------------
    def recommend_queries(self, positions, k, sum_order=None, user_sim=None, ratings=None):
        """"Whom do I show query j?" for queries that are columns of the matrix (recommend_new_queries covers new ones):
        per requested position the k users with the largest non-zero predictions among those who have not rated it,
        value descending then user ascending -- recommend()'s selection over the transposed columns of
        compute_scores(reuse_lists=True)[1], from the live lists and the live user lists in step (ValueError when there
        are no live lists), so current after every live operation.  positions: 0-based columns (any order; a host
        sequence or a device tensor), None = every column.  user_sim / ratings as recommend_users takes them.
        -> {j: {'users': int64[user rows, 0-based], 'values': int64, 'available': int}}, recommend_new_queries' shape.
        Raises ValueError for a bad k, sum_order or position."""
        from qrlsh import recommend as rec
        from qrlsh import servequeries as sq
        k, positions = _int_in(k, "k", 1, rec.MAX_K), _ids_arg(positions)
        lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, ratings)
        users, val, avail = sq.for_queries(ratings, lists[0], lists[1], lists[2], user_sim, positions, k,
                                           sum_order=sum_order, query_weight=self.query_weight,
                                           user_weight=self.user_weight, default_mean=self.default_mean,
                                           device=self.device)
        return _served(positions, users, val, avail, k, "users")

    def predict_queries(self, positions, sum_order=None, user_sim=None, ratings=None):
        """DataFrame usersIDs x queriesIDs[positions]: those columns of compute_scores(reuse_lists=True)'s
        finalPredictions, from the live lists (arguments as recommend_queries takes them)."""
        from qrlsh import servequeries as sq
        positions = _ids_arg(positions)
        lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, ratings)
        cols =sq.predict_queries(ratings, lists[0], lists[1], lists[2], user_sim, positions, self.query_weight,
                                  self.user_weight, self.default_mean, self.device, sum_order=sum_order)
        ids = np.arange(self.queriesIDs.size) if positions is None else np.asarray(ops.to_host(positions), dtype=np.int64)
        return pd.DataFrame(ops.to_host(cols).T, index=self.usersIDs, columns=self.queriesIDs[ids]).astype(int)

    def query_utility(self, positions=None, sum_order=None, user_sim=None, ratings=None):
        """"How useful is query j to the whole user base?" -> qrlsh.QueryUtility over the requested positions (default:
        every column): per query the users who rated it, predicted and missed users, the sums, the blend's branches,
        and .utility / .mean_rating / .mean_prediction / .coverage (arguments as recommend_queries takes them)."""
        from qrlsh import servequeries as sq
        positions = _ids_arg(positions)
        lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, ratings)
        return sq.query_utility(ratings, lists[0], lists[1], lists[2], user_sim, positions, self.query_weight,
                                self.user_weight, self.default_mean, self.device, sum_order=sum_order)

    # ---- how good is the served model: the prediction error on rated cells (qrlsh.evaluate) -----------------------
    def evaluate(self, fraction=1.0, seed=0, holdout=False, cells=None, sum_order=None, user_sim=None, lists=None):
        """The prediction error of the model served now, on the device -> qrlsh.Evaluation (.mae, .rmse, .bias,
        .coverage, .by_branch, .per_user, .totals).  The query side comes from the live lists (ValueError when there are
        none); the sample is about `fraction` of the rated cells, chosen by `seed` (qrlsh.evaluate.is_kept).
        holdout=False: leave-one-out -- every kept rated cell is predicted without its own rating, from the live lists
        and the user index when it is in step (otherwise user_sim, default compute_userSimilarities): _serving_inputs'
        choice, so the answer is current after rate, add_queries(update_lists=True), remove_rows and the rest.  THE LISTS
        ARE HELD FIXED: the user similarities were computed with the cell present, which flatters the user side.
        holdout=True is the protocol without that leak: the kept rated cells are zeroed in a train copy on the device,
        the user side is built over that copy (a user index in step: UserLists.build over it with the index's labels
        and K; otherwise user_sim, default the compute_userSimilarities route over it) and the held-out cells are
        predicted from it and compared with self.ratings.  The query lists do not depend on ratings and are used as
        they stand.  Neither self.ratings nor user_index is modified.
        cells=(users, queries, values): an explicit test set instead of the sample (0-based positions; every triplet
        counts), predicted from the ratings as they stand as if each cell were unrated.
        lists: a (src, dst, milli) triple covering all served queries, used as the query side in place of the live lists
        (e.g. exact_query_lists().coo()); None = the live lists.
        ValueError for a fraction outside [0, 1], a bad sum_order, or cells together with holdout."""
        from qrlsh.evaluate import keep_word, evaluate as sweep, evaluate_cells
        keep_word(fraction)
        if cells is not None and holdout:
            raise ValueError("cells name their own test set: holdout=True does not apply")
        weights = dict(query_weight=self.query_weight, user_weight=self.user_weight, default_mean=self.default_mean,
                       device=self.device)
        if not holdout:
            lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, None, lists)
            if cells is not None:
                users, queries, values = cells
                return evaluate_cells(ratings, lists[0], lists[1], lists[2], user_sim, users, queries, values,
                                      sum_order=sum_order, **weights)
            return sweep(ratings, lists[0], lists[1], lists[2], user_sim, fraction=fraction, seed=seed,
                         sum_order=sum_order, **weights)
        lists, sum_order, train, truth, user_sim = self._holdout_inputs(fraction, seed, sum_order, user_sim, lists)
        return sweep(train, lists[0], lists[1], lists[2], user_sim, truth=truth, fraction=fraction, seed=seed,
                     sum_order=sum_order, **weights)

    def _holdout_inputs(self, fraction, seed, sum_order, user_sim, lists=None):
        """The hold-out split evaluate(holdout=True), evaluate_ranking and tune share: the live lists (ValueError when
        there are none), the checked sum_order, a train copy on the device with the kept rated cells zeroed, the full
        matrix, and the user side over the train copy (a user index in step: UserLists.build over it with the index's
        labels and K; otherwise user_sim, default the compute_userSimilarities route over it).  Nothing of self is
        modified.  -> (lists, sum_order, train, truth, user_sim)"""
        from qrlsh.evaluate import holdout as train_copy
        from qrlsh.userlists import UserLists
        lists, sum_order = self._lists_or_refuse(lists), self._sum_order(sum_order)
        ui = self._user_index_in_step() if user_sim is None else None
        truth = ui.ratings if ui is not None else torch.from_numpy(
            np.ascontiguousarray(self.ratings, dtype=np.int32)).to(self.device)
        train, _ = train_copy(truth, fraction, seed=seed, device=self.device)
        if ui is not None:
            user_sim = UserLists.build(train, ui.user_labels(), K=ui.K, device=self.device).as_user_sims()
        elif user_sim is None:
            user_sim = self._user_similarities_over(ops.to_host(train))
        return lists, sum_order, train, truth, user_sim

    # ---- which blend serves best: evaluate()'s figures over a grid of settings in one sweep (qrlsh.tune) -----------
    def tune(self, weights, q_cuts=None, u_cuts=None, fraction=0.1, seed=0, holdout=True, sum_order=None, user_sim=None,
             metric="rmse", min_coverage=0.0, apply=False, apply_cuts=False):
        """evaluate()'s error for every setting of a grid, from one sweep of the device -> qrlsh.GridEvaluation
        (.totals, .n, .mae, .rmse, .bias, .coverage, .best()).  weights: (W, 3) rows (query_weight, user_weight,
        default_mean); q_cuts / u_cuts: up to 4 list lengths each (default: the whole lists; 0 switches a side off) --
        the first `cut` entries of a stored list are the list a run with that K would have stored.
        The split and the user side are those of evaluate(holdout=...): holdout=True builds the user lists once over
        the train copy (they do not depend on the weights); holdout=False is leave-one-out with the lists held fixed.
        apply=True sets query_weight, user_weight and default_mean to the best triple by `metric` among the settings
        with coverage >= min_coverage (GridEvaluation.best), so every serving call uses it from then on.
        apply_cuts=True applies the cuts of that best setting to the live lists through set_list_lengths: a side whose
        cuts were not given, or whose best cut is >= its current length, is left alone -- TUNE NEVER REGROWS.  A best cut
        of 0 (side switched off) and a user cut without a user index in step raise ValueError; all of it is decided
        before weights or lists change, so a refusal leaves the recommender as it was.  By default (apply_cuts=False)
        cuts are only reported, and neither self.ratings, the lists nor user_index is modified.  ValueError as
        qrlsh.evaluate_grid raises it, and from best() when apply or apply_cuts is set."""
        from qrlsh.evaluate import keep_word
        from qrlsh.tune import evaluate_grid, METRICS
        keep_word(fraction)
        if metric not in METRICS:
            raise ValueError("metric must be one of %s" % (METRICS,))
        if holdout:
            lists, sum_order, ratings, truth, user_sim = self._holdout_inputs(fraction, seed, sum_order, user_sim)
        else:
            lists, sum_order, user_sim, ratings = self._serving_inputs(sum_order, user_sim, None)
            truth = None
        grid = evaluate_grid(ratings, lists[0], lists[1], lists[2], user_sim, weights, q_cuts=q_cuts, u_cuts=u_cuts,
                             truth=truth, fraction=fraction, seed=seed, sum_order=sum_order, device=self.device)
        return self._apply_best(grid, metric, min_coverage, q_cuts, u_cuts, apply, apply_cuts)

    def _apply_best(self, grid, metric, floor, q_cuts, u_cuts, apply, apply_cuts):
        """tune's and tune_ranking's tail: with apply / apply_cuts, grid.best(metric, floor) goes to the live lists (the
        cuts of the sides whose cuts were given: _cut_plan decides, set_list_lengths applies) and then to the weights, so
        a refused cut leaves the recommender as it was.  -> grid"""
        if apply or apply_cuts:
            qc, uc, (qw, uw, dm), _ = grid.best(metric, floor)
            if apply_cuts:
                self.set_list_lengths(*self._cut_plan(qc if q_cuts is not None else None, uc if u_cuts is not None else None))
            if apply:
                self.query_weight, self.user_weight, self.default_mean = qw, uw, dm
        return grid

    # ---- and are the lists it serves any good: precision / recall / NDCG at k on held-out cells (qrlsh.ranking) -----
    def evaluate_ranking(self, k, relevant, fraction=0.1, seed=0, candidates="all", users=None, sum_order=None,
                         user_sim=None, lists=None):
        """Score the top-k lists of the model served now against held-out ratings, on the device ->
        qrlsh.RankingEvaluation (.precision, .recall, .ndcg, .hit_rate, .known_share, .macro(), .per_user, .totals,
        .idx / .val / .avail).  The split and the user side are those of evaluate(holdout=True): about `fraction` of
        the rated cells, chosen by `seed`, are zeroed in a train copy on the device; the user side is built over that
        copy (a user index in step: UserLists.build over it with the index's labels and K; otherwise user_sim, default
        the compute_userSimilarities route over it); the query side comes from the live lists as they stand
        (ValueError when there are none).  Each requested user (default: all) is served its list from the train copy,
        and the list is held to self.ratings: a held-out cell rated >= relevant is a hit.  candidates: "all" ranks
        every unrated cell of the train copy, "heldout" the held-out cells only.  lists: a (src, dst, milli) triple
        covering all served queries, used in place of the live lists; None = the live lists.  Neither self.ratings nor
        user_index is modified.  ValueError for a bad k, relevant, candidates, fraction, sum_order or user id."""
        from qrlsh.evaluate import keep_word
        from qrlsh.ranking import check_arguments, evaluate_ranking as score
        keep_word(fraction)
        check_arguments(k, relevant, candidates)
        users = _ids_arg(users)
        lists, sum_order, train, truth, user_sim = self._holdout_inputs(fraction, seed, sum_order, user_sim, lists)
        return score(train, truth, lists[0], lists[1], lists[2], user_sim, k, relevant, users=users,
                     candidates=candidates, sum_order=sum_order, query_weight=self.query_weight,
                     user_weight=self.user_weight, default_mean=self.default_mean, device=self.device)

    # ---- which blend serves the best lists: evaluate_ranking's figures over a grid in one sweep (qrlsh.rankgrid) -----
    def tune_ranking(self, k, relevant, weights, q_cuts=None, u_cuts=None, fraction=0.1, seed=0, users=None,
                     sum_order=None, user_sim=None, metric="ndcg", min_recall=0.0, apply=False, apply_cuts=False):
        """evaluate_ranking(candidates="heldout")'s figures for every setting of a grid, from one sweep of the device ->
        qrlsh.RankingGridEvaluation (.totals, .precision, .recall, .ndcg, .hit_rate, .best()).  RMSE (tune) moves with
        the default-mean term of the blend, not with the order of the list; these are the figures for the order.
        weights, q_cuts, u_cuts: as tune takes them; k, relevant, users: as evaluate_ranking takes them.  The split and
        the user side are those of evaluate_ranking: _holdout_inputs, built once (they do not depend on the setting).
        apply=True sets query_weight, user_weight and default_mean to the best triple by `metric` ('ndcg', 'precision',
        'recall', 'hit_rate') among the settings with recall >= min_recall (RankingGridEvaluation.best), so every
        serving call uses it from then on.  apply_cuts=True applies the best setting's cuts through set_list_lengths
        under tune's rules (only cuts that shorten, never a regrow; a best cut of 0 or a user cut without a user index in
        step raises ValueError before anything changes).  By default cuts are only reported, and neither self.ratings,
        the lists nor user_index is modified.  ValueError as qrlsh.evaluate_ranking_grid raises it, and from best() when
        apply or apply_cuts is set."""
        from qrlsh.evaluate import keep_word
        from qrlsh.ranking import check_arguments
        from qrlsh.rankgrid import evaluate_ranking_grid, METRICS
        keep_word(fraction)
        check_arguments(k, relevant, "heldout")
        if metric not in METRICS:
            raise ValueError("metric must be one of %s" % (METRICS,))
        users = _ids_arg(users)
        lists, sum_order, train, truth, user_sim = self._holdout_inputs(fraction, seed, sum_order, user_sim)
        grid = evaluate_ranking_grid(train, truth, lists[0], lists[1], lists[2], user_sim, k, relevant, weights,
                                     q_cuts=q_cuts, u_cuts=u_cuts, users=users, sum_order=sum_order,
                                     device=self.device)
        return self._apply_best(grid, metric, min_recall, q_cuts, u_cuts, apply, apply_cuts)

    # ---- and which rerank: accuracy and redundancy of the diversified lists per (penalty, max_sim) (qrlsh.diversify) ---
    def tune_diversity(self, k, relevant, settings, pool=None, fraction=0.1, seed=0, users=None, sum_order=None,
                       user_sim=None, metric="ndcg", max_pairs_per_list=None, apply=False):
        """What each (penalty, max_sim) of `settings` costs in precision / recall / NDCG at k on held-out cells and what
        redundancy it removes, from one sweep and one adjacency per request -> qrlsh.DiversityGrid (.totals, .precision,
        .recall, .ndcg, .hit_rate, .pairs_per_list, .mean_sim, .changed_share, .ended_early, .best(),
        .least_redundant()).  The split and the user side are those of evaluate_ranking: _holdout_inputs; every
        requested user (default: all) is served a pool of `pool` candidates (default min(1024, max(4 k, 64))) from the
        train copy with the blend served now, the pool is reranked to k under every setting by the live neighbour
        lists as they stand, and each list is held to self.ratings.  Setting (0, 1001) is the plain list:
        evaluate_ranking(k, relevant)'s figures.
        apply=True sets diversity_penalty and diversity_max_sim to the best pair by `metric` among the settings with
        pairs_per_list <= max_pairs_per_list (DiversityGrid.best), so recommend_users_diverse called without a penalty
        uses it from then on.  Nothing else of self is modified.  ValueError as qrlsh.evaluate_diversity raises it, and
        from best() when apply is set."""
        from qrlsh.evaluate import keep_word
        dv = _diversify()
        keep_word(fraction)
        k = dv._check_rule(k, 0, 1001)[0]
        pool = dv._check_pool(k, pool)
        settings = dv._check_settings(settings)
        if metric not in dv.GRID_METRICS:
            raise ValueError("metric must be one of %s" % (dv.GRID_METRICS,))
        users = _ids_arg(users)
        lists, sum_order, train, truth, user_sim = self._holdout_inputs(fraction, seed, sum_order, user_sim)
        grid = dv.evaluate_diversity(train, truth, lists[0], lists[1], lists[2], user_sim, k, relevant, settings,
                                     pool=pool, users=users, sum_order=sum_order, query_weight=self.query_weight,
                                     user_weight=self.user_weight, default_mean=self.default_mean, device=self.device)
        if apply:
            self.diversity_penalty, self.diversity_max_sim, _ = grid.best(metric, max_pairs_per_list)
        return grid

    def top_k_queries(self, to_predict, predictions, missed, ask=input):
        """Interactive top-k prompt of recommender.py:345-381 (`ask` is injectable for tests)."""
        pred = predictions.to_numpy()
        nu = self.usersIDs.size
        again = ""
        while again.lower() != "no":
            user = -1
            while not (0 <= user < nu):
                txt = ask("Enter user ID: [int][Max: " + str(nu) + "] ")
                user = int(txt) - 1 if txt.isdigit() else -1
            fresh = [j for i, j in to_predict if i == user and pred[i][j] != 0]
            k = 0
            while not (0 < k <= len(fresh)):
                txt = ask("Enter number of recommendations: [int][Max: " + str(len(fresh)) + "] ")
                k = int(txt) if txt.isdigit() else 0
            order = np.argsort(pred[user][fresh])[::-1][:k]
            print("\nTop {} unrated query recommendations for U{}: ".format(k, user + 1))
            for rank, pos in enumerate(order):
                print("{}. Q{} - {}".format(rank + 1, fresh[pos] + 1, pred[user][fresh][pos]))
            print()
            again = ""
            while again.lower() not in ("yes", "no"):
                again = ask("Do you want more suggestions? [Yes-No][Default: Yes] ") or "yes"
