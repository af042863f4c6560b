"""The schedules of tests/live_sequence_cases.py on the CPU: the conditions every committed schedule must meet (checked
from the model alone -- conditions, not measurements), determinism, the model's incremental bookkeeping against a
from-scratch recomputation after every step, and replay from a prefix."""
import numpy as np
import pytest

import live_sequence_cases as S


def _same_expected(a, b):
    for k in a:
        x, y = a[k], b[k]
        if k == "qdict":
            assert sorted(x) == sorted(y) and all(np.array_equal(x[q]["indexes"], y[q]["indexes"]) and
                                                  np.array_equal(x[q]["values"], y[q]["values"]) for q in x), k
        elif isinstance(x, tuple):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), k
        else:
            assert np.array_equal(x, y), k


def _same_op(a, b):
    assert a[0] == b[0] and list(a[1]) == list(b[1])
    for k in a[1]:
        x, y = a[1][k], b[1][k]
        assert (x is None) == (y is None) and (x is None or np.array_equal(np.asarray(x, dtype=object),
                                                                           np.asarray(y, dtype=object))), (a[0], k)


@pytest.mark.parametrize("seed", S.SEEDS)
def test_every_committed_schedule_meets_the_conditions(seed):
    c = S.conditions(seed)
    what = (seed, c)
    assert c["steps"] == S.steps_of(seed) + (9 if seed == S.EPILOGUE_SEED else 0), what
    assert all(v >= 2 for v in c["kinds"].values()), what
    assert 2 * c["long_steps"] >= c["steps"], what                     # rows straddle the starts of LC_TILE tiles
    assert all(c["full_hits"][k] >= 1 for k in ("remove_queries", "replace_queries", "remove_rows")), what
    assert c["query_regrows"] >= 1 and c["user_regrows"] >= 1, what
    assert min(c["cut_after_removal"], c["regrow_after_removal"], c["cut_after_append"], c["regrow_after_append"]) >= 1, what
    assert c["quiet_add_rows"] >= 1 and c["loud_add_rows"] >= 1, what
    assert c["joined"] >= 1 and c["founded"] >= 1, what
    N, nu = c["start"]
    assert c["n_range"][0] < N < c["n_range"][1] and c["nu_range"][0] < nu < c["nu_range"][1], what
    # the served predictions are compared at points where users have several neighbours, not one
    assert sum(k >= S.SERVED_USER_K for k in c["served_user_K"]) >= 3, what


def test_over_the_seeds_every_ordered_pair_of_families_is_adjacent():
    pairs = set().union(*(S.conditions(seed)["pairs"] for seed in S.SEEDS))
    assert pairs == {(a, b) for a in S.FAMILIES for b in S.FAMILIES}


def test_the_run_on_the_generator_data_set_is_not_a_quiet_one():
    """golden cfg2 is sparse (150 queries; its lists never reach one LC_TILE of entries, which is the synthetic table's
    part): what its run must still show is full rows hit by a removal and a replacement, regrows that pick rows on both
    sides, the four motifs, newcomers that join and found, every kind and every pair of families"""
    start, trace = S.golden_run("cfg2")
    c = S.conditions_of(trace)
    assert start.note["n"] == 150 and start.note["nu"] == 60 and c["steps"] == S.STEPS, c
    assert all(v >= 2 for v in c["kinds"].values()) and len(c["pairs"]) == 25, c
    assert c["full_hits"]["remove_queries"] >= 1 and c["full_hits"]["replace_queries"] >= 1, c
    assert c["query_regrows"] >= 1 and c["user_regrows"] >= 1, c
    assert min(c["cut_after_removal"], c["regrow_after_removal"], c["cut_after_append"], c["regrow_after_append"]) >= 1, c
    assert c["quiet_add_rows"] >= 1 and c["loud_add_rows"] >= 1 and c["joined"] >= 1 and c["founded"] >= 1, c
    assert c["n_range"][0] < 150 < c["n_range"][1] and c["nu_range"][1] > 60, c
    assert sum(k >= S.SERVED_USER_K for k in c["served_user_K"]) >= 3, c


def test_the_epilogue_goes_through_the_edges():
    notes = [x[2] for x in S.run(S.EPILOGUE_SEED)][S.EPILOGUE_STEPS:]
    ops = [x[0] for x in S.run(S.EPILOGUE_SEED)][S.EPILOGUE_STEPS:]
    assert ops[0][1] == dict(query_K=1, user_K=1) and ops[1][1] == dict(query_K=S.QUERY_MAX_K, user_K=S.USER_MAX_K)
    assert notes[1]["picked"][0] > 0 and notes[1]["picked"][1] > 0
    assert (notes[2]["n"], notes[3]["nu"]) == (2, 2)
    assert abs(notes[-1]["n"] - S.SHAPE["N"]) <= 5 and abs(notes[-1]["nu"] - S.SHAPE["nu"]) <= 5
    assert [o[0] for o in ops[-2:]] == ["rate", "set_list_lengths"] and notes[-1]["longest"] <= S.SERVED_MAX


@pytest.mark.parametrize("seed", S.SEEDS)
def test_the_same_seed_gives_the_same_schedule(seed):
    a, b = [x.op for x in S.generate(seed)], [x.op for x in S.generate(seed)]
    assert len(a) == len(b) == len(S.schedule(seed)) == len(S.schedule(seed, S.steps_of(seed)))
    for x, y, z in zip(a, b, S.schedule(seed)):
        _same_op(x, y)
        _same_op(x, z)


def test_a_schedule_of_another_length_is_drawn_afresh():
    seed = S.SEEDS[0]
    ops = S.schedule(seed, 40)
    assert len(ops) == 40 and len(S.schedule(S.EPILOGUE_SEED, 24)) == 24 + 9
    m = S.start_model()
    for op in ops:                                           # and runs on the model alone
        S.apply(m, op)


class _Universe:
    """the from-scratch side: nothing is ever deleted.  Every query, user and row keeps the number it was born with; texts,
    labels, cells and ratings are written by birth number; what is served is the living ones in birth order."""

    def __init__(self, m):
        self.q_alive, self.u_alive = list(range(m.n)), list(range(m.nu))
        self.q_ids, self.u_ids = m.query_ids.tolist(), m.user_ids.tolist()
        self.texts = [tuple(r) for r in m.queries.tolist()]
        self.labels = m.labels.tolist()
        self.r = {(u, q): int(m.ratings[u, q]) for u in range(m.nu) for q in range(m.n) if m.ratings[u, q]}
        self.rows = [tuple(r) for r in m.cells[:m.D].tolist()]       # by slot
        self.slots_alive = list(range(m.D))

    def apply(self, op, ret):
        kind, kw = op
        if kind == "add_queries":
            first = len(self.q_ids)
            for k, text in enumerate(np.asarray(kw["queries"], dtype=object).tolist()):
                self.q_alive.append(first + k)
                self.q_ids.append(str(kw["ids"][k]))
                self.texts.append(tuple(text))
                if kw["ratings"] is not None:
                    for row, u in enumerate(self.u_alive):
                        self.r[(u, first + k)] = int(kw["ratings"][row, k])
        elif kind == "remove_queries":
            gone = {self.q_alive[p] for p in np.asarray(kw["positions"]).tolist()}
            self.q_alive = [q for q in self.q_alive if q not in gone]
        elif kind == "replace_queries":
            for k, p in enumerate(np.asarray(kw["positions"]).tolist()):
                q = self.q_alive[p]
                self.texts[q] = tuple(np.asarray(kw["queries"], dtype=object)[k].tolist())
                if kw["ratings"] is not None:
                    for row, u in enumerate(self.u_alive):
                        self.r[(u, q)] = int(kw["ratings"][row, k])
        elif kind == "add_rows":
            for row in np.asarray(kw["rows"], dtype=object).tolist():
                self.slots_alive.append(len(self.rows))
                self.rows.append(tuple(row))
        elif kind == "remove_rows":
            gone = {self.slots_alive[p] for p in np.asarray(kw["positions"]).tolist()}
            self.slots_alive = [s for s in self.slots_alive if s not in gone]
        elif kind == "rate":
            for u, q, v in zip(*(np.asarray(kw[k]).tolist() for k in ("users", "queries", "values"))):
                self.r[(self.u_alive[u], self.q_alive[q])] = int(v)
        elif kind == "add_users":
            first = len(self.u_ids)
            for k in range(len(kw["ids"])):
                self.u_alive.append(first + k)
                self.u_ids.append(str(kw["ids"][k]))
                self.labels.append(int(ret[1][k]))
                for col, q in enumerate(self.q_alive):
                    self.r[(first + k, q)] = int(kw["ratings"][k, col])
        elif kind == "remove_users":
            gone = {self.u_alive[p] for p in np.asarray(kw["positions"]).tolist()}
            self.u_alive = [u for u in self.u_alive if u not in gone]

    def check(self, m, what):
        assert m.query_ids.tolist() == [self.q_ids[q] for q in self.q_alive], what
        assert m.user_ids.tolist() == [self.u_ids[u] for u in self.u_alive], what
        assert [tuple(r) for r in m.queries.tolist()] == [self.texts[q] for q in self.q_alive], what
        assert m.labels.tolist() == [self.labels[u] for u in self.u_alive], what
        want = np.array([[self.r.get((u, q), 0) for q in self.q_alive] for u in self.u_alive], dtype=np.int64)
        assert np.array_equal(m.ratings, want.reshape(len(self.u_alive), len(self.q_alive))), what
        assert m.row_slots.tolist() == self.slots_alive == np.flatnonzero(m.live).tolist(), what
        assert m.D == len(self.rows) and not m.live[m.D:].any(), what
        assert [tuple(r) for r in m.dataset().tolist()] == [self.rows[s] for s in self.slots_alive], what
        assert all(c is None for c in m.cells[~m.live].reshape(-1)), what


@pytest.mark.parametrize("seed", S.SEEDS)
def test_bookkeeping_equals_a_from_scratch_recomputation_after_every_step(seed):
    m = S.start_model()
    uni = _Universe(m)
    uni.check(m, (seed, "start"))
    for i, (op, ret, note, _, _) in enumerate(S.run(seed)):
        before = (m.n, m.nu, m.row_slots.size)
        got = S.apply(m, op)
        what = (seed, i, S.describe(op))
        uni.apply(op, got)
        uni.check(m, what)
        kind, kw = op
        # the return values: positions assigned, old-to-new maps
        if kind == "add_queries":
            assert np.array_equal(got, np.arange(before[0], m.n)) and got.dtype == np.int64, what
        elif kind in ("remove_queries", "remove_users", "remove_rows"):
            old = before[{"remove_queries": 0, "remove_users": 1, "remove_rows": 2}[kind]]
            gone = np.unique(kw["positions"])
            assert got.shape == (old,) and (got[gone] == -1).all() and (got >= 0).sum() == old - gone.size, what
            assert np.array_equal(got[got >= 0], np.arange(old - gone.size)), what
        elif kind == "add_users":
            assert np.array_equal(got[0], np.arange(before[1], m.nu)), what
            if kw["labels"] is not None:
                assert np.array_equal(got[1], kw["labels"]), what
        elif kind == "add_rows":
            assert np.array_equal(got, np.arange(before[2], m.row_slots.size)), what
        assert (note["n"], note["nu"]) == (m.n, m.nu), what


@pytest.mark.parametrize("seed", S.SEEDS)
def test_a_schedule_replayed_from_any_prefix_reaches_the_same_state(seed):
    trace = S.run(seed)
    ops = S.schedule(seed)
    for upto in sorted({1, 2, len(ops) // 3, len(ops) // 2, len(ops) - 1, len(ops)}):
        m = S.start_model()
        for op in ops[:upto]:
            S.apply(m, op)
        _same_expected(m.expected(), trace[upto - 1][3])
        for op in ops[upto:]:
            S.apply(m, op)
        _same_expected(m.expected(), trace[-1][3])
