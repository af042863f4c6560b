"""Random interleavings of every live operation, held to one host model (tests/live_sequence_cases.py) after every step:
every check is exact.  The schedules mix the five families -- the query set, dataset rows, the user set, ratings and the
list lengths -- through QueryIndex / LiveTable / UserLists directly (both row formats) and through the Recommender's
public methods.  The first opinion is always the model's from-scratch recompute (the oracle and the numpy restatements of
the *_cases modules), never the operation itself and never the project's own device code.

A failure names the seed, the step and the operation with its arguments; replay(seed, upto) rebuilds device and model
state at any step, so a failing schedule can be cut down to its shortest prefix by hand."""
import numpy as np
import pytest
import torch

import lists_update_cases as LC
import live_sequence_cases as S
import predict_cases as PC
import user_lists_cases as UC

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORMATS = [False, True]      # int32 rows, compact uint16 rows
FEATURES = ["f%d" % f for f in range(S.SHAPE["nfeat"])]
USER_FIELDS = ("ratings", "idx", "milli", "len", "mean", "norm2", "label", "c_off", "c_mem", "c_pos")


@pytest.fixture(scope="module")
def traces():
    """the reference of every committed seed, computed once on the host and shared by the tests below (never modified)"""
    return {seed: S.run(seed) for seed in S.SEEDS}


ORDERS = ("pairwise", "sequential")


def _serve_refs(start, trace):
    """{step: (chosen users, {sum_order: oracle.predict_cells over the model's lists})} for every fifth step and the
    last one; no predictions where a list is longer than the prediction kernels take"""
    from oracle import oracle as O
    refs, prev = {}, start
    points = S.serve_points(len(trace))
    for i, step in enumerate(trace):
        if i in points:
            chosen = list(dict.fromkeys(_chosen(step, prev)))
            preds = None
            if step.note["longest"] <= S.SERVED_MAX:
                preds = {order: S.predictions(step, chosen, summation)
                         for order, summation in zip(ORDERS, (O.np_sum_order, PC.sequential_sum))}
            refs[i] = (chosen, preds)
        prev = step
    return refs


@pytest.fixture(scope="module")
def serve_refs(traces):
    start = S.start_step()
    return {seed: _serve_refs(start, traces[seed]) for seed in S.SEEDS}


def _named(what, check, *args):
    """a helper's assertion, with the seed, the step and the operation in front"""
    try:
        check(*args)
    except AssertionError as err:
        raise AssertionError("%s: %s" % (what, err)) from err


def _what(seed, i, step):
    return "seed %d, step %d: %s" % (seed, i, S.describe(step.op))


# ---- comparisons with a recorded step ----------------------------------------------------------------------------------
def _check_index(qi, step, compact, what, lists=True):
    """sig and norm2 against the oracle's, keys / ids / dir byte for byte against a fresh QueryIndex over the model's
    signatures, the lists against the oracle's at the model's length"""
    from qrlsh.index import QueryIndex
    from test_gpu_index_remove import _assert_snapshot, _dev, _host, _rows
    e, st = step.expected, step.state
    assert qi.n == len(e["sig"]) == st["query_ids"].size, what
    assert qi.sig.is_contiguous() and torch.equal(qi.sig, _rows(e["sig"], compact)), (what, "sig")
    assert np.array_equal(qi.norm2.cpu().numpy(), e["norm2"]), (what, "norm2")
    fresh = QueryIndex(_rows(e["sig"], compact), None, qi.b)
    arrays = {k: getattr(fresh, k) for k in ("keys", "ids", "dir", "sig", "norm2")}
    for k, w in arrays.items():
        g = getattr(qi, k)
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape) and torch.equal(g, w), (what, k)
    if lists:
        got = _host(qi.lists)
        assert qi.lists_K == st["query_K"], (what, "lists_K", qi.lists_K, st["query_K"])
        _assert_snapshot(qi, (arrays, _dev(e["qlists"])), what)
        assert LC.same(got, e["qlists"]), (what, "query lists", [len(a) for a in got], len(e["qlists"][0]))
    else:
        assert qi.lists is None, what


def _check_table(lt, step, what):
    """the live mask, D, the cells and the served queries' rows (decoded through the table's dictionary) and the answer
    sets against the model"""
    e, st = step.expected, step.state
    assert lt.D == st["D"] and np.array_equal(lt.live, st["live"]), (what, "live")
    cells = lt.cells.cpu().numpy()
    assert np.array_equal(cells, lt._cells), (what, "host mirror of the cells")
    qrows = lt.qrows.cpu().numpy()
    assert qrows.shape == st["queries"].shape, (what, "qrows")
    for f in range(lt.nfeat):
        names = np.full(lt.dictionary.nrows + 1, None, dtype=object)      # id -> value; -1 (free, dead, unconstrained) -> None
        for v, k in lt.dictionary.maps[f].items():
            names[k] = v
        want = np.array([None if w is None else str(w) for w in st["cells"][:, f]], dtype=object)
        assert np.array_equal(names[cells[:, f]], want), (what, "cells of feature", f, np.flatnonzero(names[cells[:, f]] != want)[:8])
        want = np.array([None if str(w) == "" else str(w) for w in st["queries"][:, f]], dtype=object)
        assert np.array_equal(names[qrows[:, f]], want), (what, "qrows of feature", f, np.flatnonzero(names[qrows[:, f]] != want)[:8])
    off, rows = lt.answer_sets()
    assert np.array_equal(off.cpu().numpy(), e["off"]) and np.array_equal(rows.cpu().numpy(), e["rows"]), (what, "answer sets")


def _check_users(ul, step, what):
    from test_gpu_user_rows import assert_lists, dense
    e, st = step.expected, step.state
    assert (ul.nu, ul.nq, ul.K) == st["ratings"].shape + (st["user_K"],), (what, "users, queries and K of the user index",
                                                                              ul.nu, ul.nq, ul.K, st["ratings"].shape, st["user_K"])
    assert ul.ratings.dtype == torch.int32 and np.array_equal(ul.ratings.cpu().numpy(), st["ratings"]), (what, "ratings")
    assert np.array_equal(ul.mean.cpu().numpy(), e["mean"]), (what, "mean")
    assert np.array_equal(ul.norm2.cpu().numpy(), e["unorm2"]), (what, "norm2")
    assert np.array_equal(ul.user_labels(), st["labels"]) and ul.user_labels().dtype == np.int64, (what, "labels")
    got = dense(ul)
    assert_lists(got, e["ulists"], what)
    assert UC.same(got, e["ulists"]), what


def _same_returned(kind, got, want, what):
    if kind == "set_list_lengths":
        assert tuple(got) == tuple(want), (what, "returned", got, want)
    elif kind == "rate":
        assert got == want, (what, "rows rewritten", got, want)
    elif want is not None:
        got = np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)
        assert got.dtype == np.int64 and np.array_equal(got, want), (what, "returned", got[:8], np.asarray(want)[:8])


# ---- a. the components -------------------------------------------------------------------------------------------------
class Components:
    """QueryIndex, LiveTable and UserLists over the model's starting state, set up as test_gpu_table_rows._live_setup"""

    def __init__(self, compact):
        from qrlsh import ops
        from qrlsh.index import QueryIndex
        from qrlsh.table import LiveTable
        from qrlsh.userlists import UserLists
        from test_gpu_index_remove import _dev
        m = S.start_model()
        self.compact = compact
        self.lt = LiveTable.build([m.cells[:m.D, f] for f in range(m.nfeat)], m.queries, capacity=m.capacity)
        self.table = ops.perm_table(m.perms)
        sig, norm2, _ = ops.minhash(*self.lt.answer_sets(), self.table, b=None, want_norm=True, compact=compact)
        self.qi = QueryIndex(sig, norm2, m.b, table=self.table, K=m.query_K, lists=_dev(m.expected()["qlists"]))
        self.ul = UserLists.build(m.ratings, m.labels, K=m.user_K, device=DEV)

    def do(self, step):
        """the operation of a recorded step on the three structures, every list kept -> what the call returned"""
        (kind, kw), qi, lt, ul = step.op, self.qi, self.lt, self.ul
        if kind == "add_queries":
            nq = lt.encode(kw["queries"])
            first, m = qi.add(*lt.answer_sets(nq), update_lists=True)
            lt.add_queries(nq)
            ul.add_columns(m if kw["ratings"] is None else kw["ratings"])
            return np.arange(first, first + m, dtype=np.int64)
        if kind == "remove_queries":
            new_pos = qi.remove(kw["positions"], update_lists=True)
            lt.remove_queries(new_pos)
            ul.remove_columns(kw["positions"])
            return new_pos
        if kind == "replace_queries":
            nq = lt.encode(kw["queries"])
            qi.set(kw["positions"], *lt.answer_sets(nq), update_lists=True)
            lt.set_queries(kw["positions"], nq)
            if kw["ratings"] is not None:
                ul.set_columns(kw["positions"], kw["ratings"])
            return None
        if kind == "add_rows":
            slots = lt.add_rows(kw["rows"], qi, update_lists=True)
            assert np.array_equal(slots, step.note["slots"]), (S.describe(step.op), "slots taken", slots, step.note["slots"])
            return None
        if kind == "remove_rows":
            lt.remove_rows(step.note["slots"], qi, update_lists=True)
            return None
        if kind == "rate":
            return ul.rate(kw["users"], kw["queries"], kw["values"])
        if kind == "add_users":
            return ul.add_users(kw["ratings"], labels=kw["labels"])
        if kind == "remove_users":
            return ul.remove_users(kw["positions"])
        if kind == "set_list_lengths":
            return (None if kw.get("query_K") is None else qi.set_list_length(kw["query_K"]),
                    None if kw.get("user_K") is None else ul.set_list_length(kw["user_K"]))
        raise AssertionError(kind)

    def check(self, step, what):
        _check_index(self.qi, step, self.compact, what)
        _check_table(self.lt, step, what)
        _check_users(self.ul, step, what)


def _check_picks(qi, lt, step, what):
    """a full row was hit: the device probed again"""
    kind, note = step.op[0], step.note
    if kind in ("add_rows", "remove_rows"):
        assert lt.last_changed == note["changed"], (what, "changed queries", lt.last_changed, note["changed"])
        if not note["changed"]:
            return
    if note["full_hit"] is not None:
        assert (qi.last_picked > 0) == (note["full_hit"] > 0), (what, "rows probed again", qi.last_picked, note["full_hit"])


@pytest.mark.parametrize("compact", FORMATS)
@pytest.mark.parametrize("seed", S.SEEDS)
def test_components_follow_the_model(traces, seed, compact):
    c = Components(compact)
    c.check(S.start_step(), "seed %d: built" % seed)
    for i, step in enumerate(traces[seed]):
        what = _what(seed, i, step)
        got = c.do(step)
        kind = step.op[0]
        want = step.returned[1] if kind == "add_users" else step.returned
        _same_returned(kind, got, None if kind in ("add_rows", "remove_rows") else want, what)
        _check_picks(c.qi, c.lt, step, what)
        c.check(step, what)


# ---- b. the Recommender ------------------------------------------------------------------------------------------------
def _refuse_user_similarities():
    raise AssertionError("compute_userSimilarities ran: the live user index did not serve")


class Served:
    """a Recommender over the model's starting state: one run, a live user index, then only live operations"""

    def __init__(self, monkeypatch, rec=None, model=None):
        """rec: a Recommender that holds its data and has not run yet (default: one over the synthetic string table);
        model: its LiveModel"""
        import pandas as pd
        import recommender as R
        m = S.start_model() if model is None else model
        if rec is None:
            rec = R.Recommender()
            rec.verbose = False
            rec.datasetFeatures = list(FEATURES)
            rec.dataset = pd.DataFrame(m.cells[:m.D], columns=FEATURES).astype(str)
            rec.queries, rec.queriesIDs, rec.usersIDs = m.queries.copy(), m.query_ids.copy(), m.user_ids.copy()
            rec.ratings, rec.tupleCount = m.ratings.copy(), {}
            monkeypatch.setattr(R, "PERM", m.perms.shape[0])
            rec.bands, rec.max_candidates = m.b, m.query_K
            np.random.seed(S.SHAPE["table_seed"])            # the draws the model's permutation array restates
        rec.row_capacity = m.capacity
        rec.compute_querySimilarities()
        assert (rec.last_result.b, rec.last_result.K) == (m.b, m.query_K)
        rec.live_user_similarities(labels=m.labels, K=m.user_K)
        rec.compute_userSimilarities = _refuse_user_similarities
        self.rec, self.ui, self.features = rec, rec.user_index, list(rec.datasetFeatures)
        self.id_kinds = (rec.queriesIDs.dtype.kind, rec.usersIDs.dtype.kind)
        self.dropped = self.index_made = self.table_made = False

    def do(self, step, update_lists=True):
        """the operation of a recorded step through the public method; a call that returns has made the structures it
        works on (index_made, table_made): from then on check() insists on them"""
        (kind, kw), rec = step.op, self.rec
        if kind in ("add_queries", "remove_queries", "replace_queries", "add_rows", "remove_rows"):
            got = getattr(rec, kind)(update_lists=update_lists, **kw)
            self.index_made = True
            self.table_made = self.table_made or kind in ("add_rows", "remove_rows")
            return got
        got = getattr(rec, kind)(**kw)
        self.index_made = self.index_made or (kind == "set_list_lengths" and kw.get("query_K") is not None)
        return got

    def check(self, step, what, compact=None):
        from test_gpu_index_remove import _host, _same_dict
        rec, e, st = self.rec, step.expected, step.state
        assert rec.user_index is self.ui, what
        assert np.array_equal(np.asarray(rec.queries, dtype=object), st["queries"]), (what, "queries")
        assert (rec.queriesIDs.dtype.kind, rec.usersIDs.dtype.kind) == self.id_kinds, (what, "the id arrays keep their kind")
        assert list(rec.queriesIDs) == list(st["query_ids"]), (what, "queriesIDs")
        assert list(rec.usersIDs) == list(st["user_ids"]), (what, "usersIDs")
        assert rec.ratings.dtype == np.int64 and np.array_equal(rec.ratings, st["ratings"]), (what, "ratings")
        data = st["cells"][st["row_slots"]]
        assert np.array_equal(rec.dataset[self.features].to_numpy().astype(object), data.astype(str).astype(object)), (what, "dataset")
        assert list(rec.dataset.index) == list(range(len(data))), (what, "dataset index")
        if rec.row_slots is None:
            assert np.array_equal(st["row_slots"], np.arange(len(data))), (what, "row_slots")
        else:
            assert rec.row_slots.dtype == np.int64 and np.array_equal(rec.row_slots, st["row_slots"]), (what, "row_slots")
        qi = rec._query_index
        assert qi is not None or not self.index_made, (what, "the query index is gone")
        assert rec._live_table is not None or not self.table_made, (what, "the live table is gone")
        if self.dropped:
            assert qi.lists is None and rec._live_lists() is None, (what, "the lists stay dropped")
            with pytest.raises(ValueError):
                rec.current_query_similarities()
        else:
            _named(what, _same_dict, rec.current_query_similarities(), e["qdict"])
            assert LC.same(_host(rec._live_lists()), e["qlists"]), (what, "live lists")
        if qi is not None:
            _check_index(qi, step, qi.sig.dtype == torch.int16, what, lists=not self.dropped)
        if rec._live_table is not None:
            _check_table(rec._live_table, step, what)
        _check_users(self.ui, step, what)

    def serve(self, step, chosen, preds, what):
        """recommend_users and predict_users for the chosen users against oracle.predict_cells over the model's lists
        (preds, by summation order); lists beyond what the prediction kernels take (preds None) are refused"""
        from test_gpu_recommend_users import _same_answers
        rec, st = self.rec, step.state
        if preds is None:
            with pytest.raises(ValueError, match="neighbours"):
                rec.predict_users(chosen)
            return
        k = 7
        for order in ORDERS:
            pred = preds[order]
            got = rec.predict_users(chosen, sum_order=order)
            assert np.array_equal(got.to_numpy(), pred), (what, order, "predict_users")
            assert list(got.index) == list(st["user_ids"][chosen]) and list(got.columns) == list(st["query_ids"]), what
            want = {}
            for row, u in enumerate(chosen):
                cols = np.nonzero((st["ratings"][u] == 0) & (pred[row] != 0))[0]
                v = pred[row][cols]
                top = np.lexsort((cols, -v))[:k]
                want[u] = {"indexes": cols[top].astype(np.int64), "values": v[top].astype(np.int64), "available": len(cols)}
            _named((what, order, "recommend_users"), _same_answers, rec.recommend_users(chosen, k, sum_order=order), want)


def _chosen(step, prev):
    """a handful of users: the first, the newest, one in the middle and one whose list just changed"""
    nu = step.state["ratings"].shape[0]
    users = [0, nu - 1, nu // 2]
    a, b = step.expected["ulists"][0], prev.expected["ulists"][0]
    if a.shape == b.shape and (a != b).any():
        users.append(int(np.argwhere(a != b)[0, 0]))
    if step.op[0] == "rate":
        users.append(int(step.op[1]["users"][0]))
    return users


def _follow(s, seed, start, trace, refs):
    s.check(start, "seed %d: after the run" % seed)
    for i, step in enumerate(trace):
        what = _what(seed, i, step)
        got = s.do(step)
        _same_returned(step.op[0], got, step.returned[0] if step.op[0] == "add_users" else step.returned, what)
        if step.op[0] == "add_users":
            m = len(step.returned[1])
            assert np.array_equal(s.ui.user_labels()[-m:], step.returned[1]), (what, "labels assigned")
        if s.rec._live_table is not None:
            _check_picks(s.rec._query_index, s.rec._live_table, step, what)
        s.check(step, what)
        if i in refs:
            s.serve(step, *refs[i], what)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_recommender_follows_the_model(traces, serve_refs, seed, monkeypatch):
    assert any(preds is not None for _, preds in serve_refs[seed].values()) and len(traces[seed]) - 1 in serve_refs[seed]
    _follow(Served(monkeypatch), seed, S.start_step(), traces[seed], serve_refs[seed])


@pytest.fixture(scope="module")
def generator_case():
    """golden cfg2 (700 rows of 5 features, 150 queries, 60 users, string ids, P = 180 under the band rule): a
    Recommender that holds it, and live_sequence_cases' model and run of it (the committed generator of schedules, drawn
    against that model; test_live_sequence_host pins what the run shows)"""
    from test_gpu_recommend import _recommender_on
    rec, g = _recommender_on("cfg2")
    model = S.golden_model("cfg2")
    assert np.array_equal(rec.dataset[rec.datasetFeatures].to_numpy().astype(object), model.cells[:model.D])
    assert np.array_equal(np.asarray(rec.queries, dtype=object), model.queries) and np.array_equal(rec.ratings, model.ratings)
    assert list(rec.queriesIDs) == list(model.query_ids) and list(rec.usersIDs) == list(model.user_ids)
    assert (model.perms.shape[0], model.b) == (int(g["P"]), rec._band_rule())
    start, trace = S.golden_run("cfg2")
    return rec, g, model, start, trace, _serve_refs(start, trace)


def test_recommender_on_a_generator_data_set_follows_the_model(generator_case, monkeypatch):
    import recommender as R
    rec, g, model, start, trace, refs = generator_case
    monkeypatch.setattr(R, "PERM", int(g["P"]))
    np.random.seed(int(g["seed"]))                           # the draws the model's permutation array restates
    _follow(Served(monkeypatch, rec=rec, model=model), S.GOLDEN_SEED, start, trace, refs)


# ---- c. refusals in evolved states -------------------------------------------------------------------------------------
def _everything(rec):
    """every device field and every host array of the live state: name -> (object, bytes)"""
    qi, lt, ui = rec._query_index, rec._live_table, rec.user_index
    dev = {"qi." + k: getattr(qi, k) for k in ("keys", "ids", "dir", "sig", "norm2")}
    if qi.lists is not None:
        dev.update({"qi.lists.%d" % k: t for k, t in enumerate(qi.lists)})
    if lt is not None:
        dev.update({"lt." + k: getattr(lt, k) for k in ("bitmaps", "cells", "qrows")})
    dev.update({"ui." + k: getattr(ui, k) for k in USER_FIELDS})
    host = dict(queries=np.asarray(rec.queries, dtype=object), queriesIDs=rec.queriesIDs, usersIDs=rec.usersIDs,
                ratings=rec.ratings, dataset=rec.dataset.to_numpy(), row_slots=rec.row_slots, labels=ui.user_labels())
    if lt is not None:
        host.update(live=lt.live, lt_cells=lt._cells)
    scalars = (qi.n, qi.K, qi.lists_K, ui.nu, ui.nq, ui.K, ui.nc, None if lt is None else (lt.D, lt.n, lt.dictionary.nrows, tuple(len(mp) for mp in lt.dictionary.maps)))
    return ({k: (t, t.clone()) for k, t in dev.items()}, {k: None if a is None else np.array(a, copy=True) for k, a in host.items()},
            scalars)


def _assert_nothing_changed(rec, snap, what):
    torch.cuda.synchronize()
    dev, host, scalars = snap
    now_dev, now_host, now_scalars = _everything(rec)
    assert now_scalars == scalars, (what, now_scalars, scalars)
    assert sorted(now_dev) == sorted(dev), what
    for k, (t, held) in dev.items():
        g = now_dev[k][0]
        assert g.dtype == held.dtype and tuple(g.shape) == tuple(held.shape), (what, k)
        assert torch.equal(g.contiguous().view(torch.uint8), held.contiguous().view(torch.uint8)), (what, k)
        if k.startswith("ui.") or k.startswith("qi.lists"):        # bound back / held by reference: the same tensors
            assert g is t, (what, k, "another tensor object")
    for k, a in host.items():
        b = now_host[k]
        assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and np.array_equal(a, b))), (what, k)


def _refused_calls(rec):
    """calls that must be refused in any state with queries, rows, users and lists"""
    n, nu, rows = rec.queriesIDs.size, rec.usersIDs.size, rec.dataset.shape[0]
    q = np.asarray(rec.queries, dtype=object)
    free = rec._live_table.capacity - rec._live_table.D
    cells = rec.dataset[FEATURES].to_numpy()
    held = rec.user_index

    def without_a_user_index(call):
        def run():
            rec.user_index = None
            try:
                call()
            finally:
                rec.user_index = held
        return run
    return {
        "remove_queries outside the set": lambda: rec.remove_queries([0, n], update_lists=True),
        "replace_queries outside the set": lambda: rec.replace_queries([n], q[:1], update_lists=True),
        "replace_queries with a duplicate": lambda: rec.replace_queries([1, 2, 1], q[:3], update_lists=True),
        "remove_rows outside the set": lambda: rec.remove_rows([rows], update_lists=True),
        "more rows than free slots": lambda: rec.add_rows(cells[np.arange(free + 1) % rows], update_lists=True),
        "a negative rating": lambda: rec.rate([0, 1], [0, 1], [5, -1]),
        "a negative rating in a newcomer's row": lambda: rec.add_users(np.full((1, n), -1, dtype=np.int64)),
        "a negative rating in a new query's column": lambda: rec.add_queries(q[:1], ratings=np.full((nu, 1), -3, dtype=np.int64),
                                                                             update_lists=True),
        "rate outside the set": lambda: rec.rate([nu], [0], [5]),
        "remove_users outside the set": lambda: rec.remove_users([nu]),
        "remove_users of everybody": lambda: rec.remove_users(np.arange(nu)),
        "a user-side length without an index in step": without_a_user_index(lambda: rec.set_list_lengths(query_K=3, user_K=2)),
        "a length outside range": lambda: rec.set_list_lengths(query_K=2, user_K=65),
    }


def test_refusals_in_evolved_states_change_nothing(traces, monkeypatch):
    seed = S.SEEDS[0]
    s = Served(monkeypatch)
    trace = traces[seed]
    rows_seen = [i for i, step in enumerate(trace) if step.op[0] in ("add_rows", "remove_rows")]
    points = sorted({max(rows_seen[0], len(trace) // 3), max(rows_seen[0], 2 * len(trace) // 3), len(trace) - 1})
    assert len(points) == 3
    for i, step in enumerate(trace):
        s.do(step)
        if i in points:
            what = _what(seed, i, step)
            s.check(step, what)
            snap = _everything(s.rec)
            for name, call in _refused_calls(s.rec).items():
                with pytest.raises(ValueError):
                    call()
                _assert_nothing_changed(s.rec, snap, (what, "refused: " + name))
            s.check(step, what)


# ---- d. the dropped-lists branch ---------------------------------------------------------------------------------------
def test_one_call_without_update_lists_drops_the_lists_for_good(traces, monkeypatch):
    seed = S.SEEDS[2]
    s = Served(monkeypatch)
    trace = traces[seed]
    middle = next(i for i, step in enumerate(trace) if i >= len(trace) // 3 and step.op[0] in
                  ("add_queries", "remove_queries", "replace_queries"))
    refused = set()
    for i, step in enumerate(trace):
        what = _what(seed, i, step)
        kind, kw = step.op
        if i == middle:
            s.do(step, update_lists=False)
            s.dropped = True
        elif not s.dropped:
            s.do(step)
        elif kind == "set_list_lengths":
            if kw.get("query_K") is not None:
                snap = _everything(s.rec)
                with pytest.raises(ValueError, match="dropped"):
                    s.rec.set_list_lengths(**kw)
                _assert_nothing_changed(s.rec, snap, (what, "no lists to change"))
            if kw.get("user_K") is not None:
                assert s.rec.set_list_lengths(user_K=kw["user_K"]) == (None, step.returned[1]), what
        elif S.FAMILY[kind] in ("queries", "rows"):
            snap = _everything(s.rec)
            with pytest.raises(ValueError, match="dropped"):
                s.do(step, update_lists=True)
            _assert_nothing_changed(s.rec, snap, (what, "no lists to update"))     # the table's dictionary included
            refused.add(kind)
            s.do(step, update_lists=False)
        else:
            s.do(step)
        s.check(step, what)
    assert s.dropped and s.rec._query_index.lists is None
    assert {"add_queries", "replace_queries", "remove_queries"} <= refused and refused & {"add_rows", "remove_rows"}, refused
    # and a query that names a value new to the dictionary, a new row: refused before the table sees them
    snap = _everything(s.rec)
    new = np.array([["never seen"] * len(FEATURES)], dtype=object)
    for call in (lambda: s.rec.add_queries(new, update_lists=True), lambda: s.rec.replace_queries([0], new, update_lists=True),
                 lambda: s.rec.add_rows(new, update_lists=True)):
        with pytest.raises(ValueError, match="dropped"):
            call()
        _assert_nothing_changed(s.rec, snap, "seed %d, after the last step: a new value in a refused call" % seed)


# ---- e. replay -----------------------------------------------------------------------------------------------------------
def replay(seed, upto, compact=False):
    """(Components, LiveModel) after the first `upto` operations of schedule(seed): the state a failure message names"""
    c = Components(compact)
    for step in S.run(seed)[:upto]:
        c.do(step)
    return c, S.replay_model(seed, upto)


def test_replay_rebuilds_the_state_of_any_step(traces):
    seed = S.SEEDS[0]
    trace = traces[seed]
    for upto in (0, 2, len(trace) // 2):
        c, model = replay(seed, upto)
        step = trace[upto - 1] if upto else S.start_step()
        c.check(step, "replay(%d, %d)" % (seed, upto))
        e = model.expected()
        assert LC.same(e["qlists"], step.expected["qlists"]) and np.array_equal(e["sig"], step.expected["sig"])
        assert np.array_equal(model.ratings, step.state["ratings"])
