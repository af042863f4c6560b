"""Ranking evaluation on the device (qrlsh.evaluate_ranking / Recommender.evaluate_ranking).  Expected values come
from the numpy restatement of tests/rank_eval_cases.py (the oracle's predictions in either sum order, a stable sort,
plain loops), never from the code under test.  Every comparison is exact integer equality, except macro(): float64."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import evaluate_cases as EC
import predict_cases as PC
import rank_eval_cases as RC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import recommend  # noqa: E402

DEV = "cuda"
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}
NAMES = ("idx", "val", "avail", "per_user", "totals")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def tensors(coo):
    return tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo)


def assert_ranking(ev, want, what):
    got = (host(ev.idx), host(ev.val), host(ev.avail), host(ev.per_user), ev.totals)
    assert got[3].dtype == np.int64 and got[4].dtype == np.int64 and got[4].shape == (16,)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, "%s %s shape %s != %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[:5]
            raise AssertionError("%s: %s differs at %s: %s != %s" % (
                what, name, at.tolist(), [g[tuple(a)] for a in at], [w[tuple(a)] for a in at]))


class Split:
    """a case and its restated predictions, computed once per sum order and request list"""

    def __init__(self, case):
        self.train, self.truth, coo, self.qs, self.us = case
        self.coo = tensors(coo)
        self.nu, self.nq = self.train.shape
        self._pred = {}

    def pred(self, order, users=None):
        rows = list(range(self.nu)) if users is None else [int(u) for u in users]
        cache = self._pred.setdefault(order, {})
        missing = sorted(set(rows) - set(cache))
        if missing:
            cache.update(zip(missing, RC.candidate_predictions(self.train, self.qs, self.us, missing, ORDERS[order])))
        return np.stack([cache[u] for u in rows])

    def want(self, users, k, relevant, candidates, gains=None, order="pairwise"):
        gains = RC.dcg_gains_ref(k) if gains is None else gains
        return RC.rank_eval_ref(self.train, self.truth, self.qs, self.us, users, k, relevant, candidates, gains,
                                ORDERS[order], pred=self.pred(order, users))

    def run(self, users, k, relevant, candidates, order="pairwise", **kw):
        return qrlsh.evaluate_ranking(self.train, self.truth, *self.coo, self.us, k, relevant, users=users,
                                      candidates=candidates, sum_order=order, device=DEV, **kw)


# ----------------------------------------------------------------------------------------------- 1. edges of the sweep
@pytest.fixture(scope="module")
def wide():
    """37 x 5003: five sweep slices of 1001 columns, the selection in its slice form (5003 % 4 != 0)"""
    return Split(RC.knife_split(5003, 37, 5003))


def edge_case(nq, wide):
    if nq == 5003:
        return wide
    return Split(RC.knife_split(nq, 37, nq) if nq > 1 else RC.split_case(1, 37, 1, fill=0.6, held=0.5))


@pytest.mark.parametrize("nq", [1, 1023, 1024, 1025, 5003])
def test_sweep_edges_both_candidate_sets_both_orders(nq, wide):
    """k = 10 cuts the lists; at k = 1024 every eligible cell of a row is listed, the knife-edge cells among them"""
    c = edge_case(nq, wide)
    relevant = 60
    repeats = list(range(c.nu - 1, -1, -3)) + [5, 2, 1, 0, 0, c.nu - 1]     # reverse order, with repeats
    wants = {}
    for order in ORDERS:
        for candidates in ("all", "heldout"):
            for k in (10, 1024):
                for users in (None, repeats):
                    want = c.want(users, k, relevant, candidates, order=order)
                    ev = c.run(users, k, relevant, candidates, order)
                    assert_ranking(ev, want, "nq=%d %s %s k=%d users=%s" % (nq, order, candidates, k, users is not None))
                    wants[order, candidates, k, users is None] = want
                if candidates == "all":
                    # second witness: the served lists are for_users' over the train matrix, output for output
                    served = qrlsh.for_users(c.train, *c.coo, c.us, repeats, k, sum_order=order, device=DEV)
                    for name, a, b in zip(NAMES, served, (ev.idx, ev.val, ev.avail)):
                        assert torch.equal(a, b), "%s differs from for_users (%s, k=%d)" % (name, order, k)
    assert ev.per_user.shape == (len(repeats), 8)
    assert all(w[4][6] > 0 for w in wants.values())                          # test cells everywhere
    if nq > 1:
        assert all(w[4][1] > 0 for w in wants.values())                      # and hits
        # the orders part -- in the held-out lists of the knife users already at k = 10: a wrong order shows
        for key in (("all", 1024, True), ("heldout", 10, True)):
            a, b = wants[("pairwise",) + key], wants[("sequential",) + key]
            assert not np.array_equal(a[1], b[1]), key


def test_macro_equals_numpy_over_the_expected_lines(wide):
    gains = RC.dcg_gains_ref(10)
    want = wide.want(None, 10, 60, "all")
    ev = wide.run(None, 10, 60, "all")
    got, ref = ev.macro(), RC.macro_ref(want[3], gains)
    assert got["n"] == ref["n"] > 30
    for name in ("precision", "recall", "ndcg", "mrr"):
        assert np.isclose(got[name], ref[name], rtol=1e-12, atol=0) and 0 < ref[name] <= 1, name
    t = [int(x) for x in want[4]]
    assert ev.precision == t[1] / t[0] and ev.recall == t[1] / t[5] and ev.ndcg == t[4] / t[11]
    assert ev.hit_rate == t[10] / t[9] and ev.known_share == t[2] / t[0] and ev.requests == 37


# ----------------------------------------------------------------------------------------------- 2. both row forms
def test_a_wide_value_sends_two_rows_to_the_global_form(wide):
    """a 256 in the rows of users 4 and 30: their workgroups read the row from memory, the others stage it in LDS.  Only
    the two rows and the two columns can move: the rest of the reference is the unplanted case's"""
    train, truth = wide.train.copy(), wide.truth.copy()
    spots = ((4, 17), (30, 5002))
    for u, j in spots:
        train[u, j] = truth[u, j] = 256
    c = Split((train, truth, [t.numpy() for t in wide.coo], wide.qs, wide.us))
    for order in ORDERS:
        pred = wide.pred(order).copy()
        only = np.zeros(train.shape, dtype=bool)
        for u, j in spots:
            only[u, :] = True
            only[:, j] = True
        fresh = RC.candidate_predictions(train, c.qs, c.us, None, ORDERS[order], only=only)
        pred[only] = fresh[only]
        c._pred[order] = dict(enumerate(pred))
        for candidates in ("all", "heldout"):
            assert_ranking(c.run(None, 10, 60, candidates, order), c.want(None, 10, 60, candidates, order=order),
                           "wide value %s %s" % (order, candidates))
    assert (c.pred("pairwise") != wide.pred("pairwise")).any()


def test_a_row_longer_than_the_lds_takes_the_global_form():
    c = Split(RC.split_case(131073, 8, 131073, fill=0.97, held=0.02, longest_q=4, ku=2))
    users = [6, 0, 3]
    for candidates in ("all", "heldout"):
        want = c.want(users, 28, 60, candidates)
        assert_ranking(c.run(users, 28, 60, candidates), want, "nq=131073 " + candidates)
        assert want[4][1] > 0 and want[4][6] > 5000


# ----------------------------------------------------------------------------------------------- 3. the queue
def test_heldout_queue_fills_overflows_and_drains():
    c = Split(RC.queue_case())
    counts = list(RC.QUEUE_COUNTS) + [2048]
    assert ((c.train == 0) & (c.truth != 0)).sum(axis=1).tolist() == counts and (c.truth != 0).all()
    last = c.nu - 1
    assert (c.train[last, 1024:2048] == 0).all() and (c.train[last, 2048:3072] != 0).all()
    want = c.want(None, 100, 60, "heldout")
    ev = c.run(None, 100, 60, "heldout", slices=1)
    assert_ranking(ev, want, "queue")
    assert want[3][:, 6].tolist() == counts and want[3][0].tolist() == [0] * 8
    # every unrated cell is a test cell here: ranking them all is the same evaluation, through the other sweep
    assert_ranking(c.run(None, 100, 60, "all", slices=1), want, "queue, all")
    # and cut into slices anywhere
    assert_ranking(c.run(None, 100, 60, "heldout", slices=5), want, "queue, 5 slices")


# ----------------------------------------------------------------------------------------------- 4. the cut
@pytest.mark.parametrize("k", [1, 64, 65, 1024])
def test_the_cut_at_k(k):
    train, truth, coo, qs, us, rows = RC.cut_case(k)
    c = Split((train, truth, coo, qs, us))
    gains = RC.primes(k)
    got = {}
    for candidates in ("heldout", "all"):
        want = c.want(None, k, RC.CUT_RELEVANT, candidates, gains=gains)
        ev = c.run(None, k, RC.CUT_RELEVANT, candidates, gains=gains)
        assert_ranking(ev, want, "cut k=%d %s" % (k, candidates))
        got[candidates] = want[3]
    # with every unrated cell a candidate the planted positions are those of cut_case's text
    per, t, u = got["all"], min(3, k), rows["ties"]
    assert per[u, 0] == k and per[u, 7] == k - t + 6 and per[u, 5] > per[u, 1]
    assert (host(ev.val)[u, k - t:] == 20).all()
    inside = host(ev.idx)[u, k - t:]
    assert (np.diff(inside) > 0).all() and (truth[u, inside] >= RC.CUT_RELEVANT).sum() == min(t, 2)
    assert per[rows["nothing"]].tolist() == [0, 0, 0, 0, 0, 2, 2, 0]                      # avail 0, unreachable cells
    assert per[rows["no_relevant"], 5] == 0 and per[rows["no_relevant"], 1] == 0
    assert per[rows["short"], 7] == 3 and (k <= 3 or per[rows["short"], 0] == 3)          # k > avail
    assert per[rows["first"], 3] == 1 and per[rows["last"], 3] == k
    assert per[rows["unlisted"]].tolist()[:6] == [k, 0, per[rows["unlisted"], 2], 0, 0, 1]
    # the held-out candidates alone: cells the truth does not rate are gone from the lists
    assert got["heldout"][rows["short"], 7] == 2 and (got["heldout"][:, 2] == got["heldout"][:, 0]).all()


# ----------------------------------------------------------------------------------------------- 5. gains are an input
def test_gains_are_an_input():
    k = 64
    train, truth, coo, qs, us, rows = RC.cut_case(k)
    c = Split((train, truth, coo, qs, us))
    default, primes = RC.dcg_gains_ref(k), RC.primes(k)
    assert default == qrlsh.dcg_gains(k).tolist()
    a = c.run(None, k, RC.CUT_RELEVANT, "all")
    b = c.run(None, k, RC.CUT_RELEVANT, "all", gains=np.array(primes))
    assert_ranking(a, c.want(None, k, RC.CUT_RELEVANT, "all", gains=default), "default gains")
    assert_ranking(b, c.want(None, k, RC.CUT_RELEVANT, "all", gains=primes), "prime gains")
    pa, pb = host(a.per_user), host(b.per_user)
    assert np.array_equal(np.delete(pa, 4, axis=1), np.delete(pb, 4, axis=1)) and (pa[:, 4] != pb[:, 4]).any()
    assert pb[rows["first"], 4] == primes[0] and pb[rows["last"], 4] == primes[k - 1] == 2
    assert pa[rows["first"], 4] == 2**32 and a.totals[11] != b.totals[11]
    assert b.totals[11] == sum(sum(primes[:min(k, int(r))]) for r in pb[:, 5])


# ----------------------------------------------------------------------------------------------- 6. slices and blocks
def test_three_slices_and_request_blocks_add_up(wide, monkeypatch):
    lib = qrlsh._lib.load()
    k, relevant = 28, 60
    want = wide.want(None, k, relevant, "all")
    whole = wide.run(None, k, relevant, "all", slices=3)
    assert_ranking(whole, want, "slices=3")
    budget = int(lib.qrlsh_evaluate_ranking_workspace_bytes(13, wide.nq, k, 3))
    assert budget < int(lib.qrlsh_evaluate_ranking_workspace_bytes(19, wide.nq, k, 3))
    monkeypatch.setattr(recommend, "WORKSPACE_BUDGET", budget)             # 37 -> 19 -> 10 requests per block: 4 blocks
    for candidates in ("all", "heldout"):
        blocks = wide.run(None, k, relevant, candidates, slices=3)
        assert_ranking(blocks, wide.want(None, k, relevant, candidates), "blocks " + candidates)
    assert np.array_equal(whole.totals, wide.run(None, k, relevant, "all", slices=3).totals)
    users = [36, 2, 2, 19] * 8
    assert_ranking(wide.run(users, k, relevant, "all", slices=3), wide.want(users, k, relevant, "all"), "blocks, a list")


# ----------------------------------------------------------------------------------------------- 7. flags
def test_flagged_inputs_raise_and_leave_no_fault(wide):
    c = wide
    rt, tt = torch.from_numpy(c.train).to(DEV), torch.from_numpy(c.truth).to(DEV)
    src, dst, mil = (t.clone() for t in c.coo)
    keep = src != 4000
    long_ = tuple(torch.cat([t[keep], extra]) for t, extra in (
        (src, torch.full((65,), 4000, dtype=torch.int32)), (dst, torch.arange(65, dtype=torch.int32)),
        (mil, torch.full((65,), 500, dtype=torch.int32))))
    order = torch.argsort(long_[0].to(torch.int64), stable=True)
    long_ = tuple(t[order] for t in long_)
    outside = dst.clone()
    outside[len(outside) // 2] = c.nq
    for candidates in ("all", "heldout"):
        def call(s, d, m, users):
            return qrlsh.evaluate_ranking(rt, tt, s, d, m, c.us, 5, 60, users=users, candidates=candidates, device=DEV)
        with pytest.raises(ValueError, match="more than 64"):
            call(*long_, None)
        with pytest.raises(ValueError, match="neighbour index"):
            call(src, outside, mil, [0, 1])
        with pytest.raises(ValueError, match="user id"):
            call(src, dst, mil, torch.tensor([3, c.nu], device=DEV))
        with pytest.raises(ValueError, match="user id"):
            call(src, dst, mil, torch.tensor([-1], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    users = [0, 36]
    assert_ranking(c.run(users, 5, 60, "all"), c.want(users, 5, 60, "all"), "after the flagged calls")


def test_no_queries_and_no_requests():
    empty = tuple(torch.zeros((0,), dtype=torch.int32) for _ in range(3))
    none = np.zeros((4, 0), dtype=np.int32)
    ev = qrlsh.evaluate_ranking(none, none, *empty, {}, 3, 50, users=[3, 0], device=DEV)
    assert host(ev.per_user).tolist() == [[0] * 8] * 2 and ev.totals.tolist() == [0] * 8 + [2] + [0] * 7
    assert (host(ev.idx) == -1).all() and np.isnan(ev.precision)
    m = np.ones((4, 9), dtype=np.int32)
    ev = qrlsh.evaluate_ranking(m, m, *empty, {}, 3, 50, users=[], device=DEV)
    assert ev.per_user.shape == (0, 8) and not ev.totals.any() and ev.macro()["n"] == 0


# ----------------------------------------------------------------------------------------------- 8. Recommender
def _index_lists(ui):
    idx, milli, n = (host(t) for t in (ui.idx, ui.milli, ui.len))
    return {u: {"indexes": idx[u, :n[u]].astype(np.int64), "values": milli[u, :n[u]] / 1000.0} for u in range(ui.nu)}


def test_recommender_scores_the_lists_it_serves():
    from test_gpu_recommend import _recommender_on
    from qrlsh import users as U
    from qrlsh.userlists import UserLists
    rec, g = _recommender_on("cfg2")
    nu, nq = rec.ratings.shape
    with pytest.raises(ValueError, match="no live lists"):
        rec.evaluate_ranking(5, 60)
    rec.compute_querySimilarities()
    rec.live_user_similarities(labels=U.cluster_labels(rec.ratings))
    ui = rec.user_index

    def raises():
        raise AssertionError("compute_userSimilarities ran: the user index did not serve")
    rec.compute_userSimilarities = raises
    summation = ORDERS[rec.sum_order]
    k, relevant, fraction, seed = 7, 60, 0.3, 11
    gains = RC.dcg_gains_ref(k)

    def in_step(what, users=None, candidates="all"):
        truth = rec.ratings.copy()
        held = [t.clone() for t in (ui.ratings, ui.idx, ui.milli, ui.len)]
        ev = rec.evaluate_ranking(k, relevant, fraction=fraction, seed=seed, users=users, candidates=candidates)
        train, count = EC.holdout_ref(truth, seed, EC.keep_of(fraction))
        fresh = UserLists.build(train, ui.user_labels(), K=ui.K, device=DEV)
        want = RC.rank_eval_ref(train, truth, rec.current_query_similarities(), _index_lists(fresh), users, k, relevant,
                                candidates, gains, summation)
        assert_ranking(ev, want, what)
        assert ev.totals[6] == (count if users is None else want[3][:, 6].sum()) > 0
        # nothing of the served state moved
        assert np.array_equal(rec.ratings, truth) and rec.user_index is ui
        assert all(torch.equal(a, b) for a, b in zip(held, (ui.ratings, ui.idx, ui.milli, ui.len)))
        return ev

    first = in_step("user index in step")
    assert first.totals[1] > 0 and first.requests == nu
    in_step("a request list, held-out candidates", users=[nu - 1, 0, 7, 7], candidates="heldout")
    # after rate(): the edit is in truth and in the lists
    rng = np.random.default_rng(7)
    us_, qs_, vs_ = rng.integers(0, nu, size=60), rng.integers(0, nq, size=60), rng.integers(60, 101, size=60)
    rec.rate(us_, qs_, vs_)
    after = in_step("after rate")
    assert not np.array_equal(after.totals, first.totals)
    # without a user index: the compute_userSimilarities route over the train matrix
    del rec.compute_userSimilarities
    del rec.user_index
    truth = rec.ratings.copy()
    train, _ = EC.holdout_ref(truth, seed, EC.keep_of(fraction))
    usim = rec._user_similarities_over(train)
    want = RC.rank_eval_ref(train, truth, rec.current_query_similarities(), usim, None, k, relevant, "all", gains,
                            summation)
    assert_ranking(rec.evaluate_ranking(k, relevant, fraction=fraction, seed=seed), want, "without a user index")
    assert np.array_equal(rec.ratings, truth)
