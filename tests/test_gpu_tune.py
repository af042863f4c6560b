"""The grid evaluation on the device (qrlsh_evaluate_grid, qrlsh.evaluate_grid, Recommender.tune).  Expected values come
from the numpy restatement of tests/tune_cases.py (lists cut on the host, the oracle's weighted_average and sum orders),
never from the code under test; every comparison is integer equality.

The sweep splits nq into min(ceil(4096 / nu), ceil(nq / 1024)) column slices, so with few users a workgroup sees at most
1024 columns and its queue drains only after the loop, however dense the matrix is.  The main case (nu = 3, nq = 2049: 3
slices of 683 columns) therefore covers the slice bounds and the tail drain; the drain INSIDE the loop needs one slice of
more than 1024 kept cells and has a case of its own with 4096 users (test_the_queue_drains_inside_the_loop)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import evaluate_cases as EC
import predict_cases as PC
import tune_cases as TC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib  # noqa: E402
from qrlsh.ops import _ptr, _stream  # noqa: E402

DEV = "cuda"
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}
ORDER_WORD = {"pairwise": _lib.SUM_PAIRWISE, "sequential": _lib.SUM_SEQUENTIAL}


def tensors(coo):
    return tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo)


def padded_user_lists(us, nu, ku):
    ui = np.full((nu, max(ku, 1)), -1, dtype=np.int32)
    uv = np.zeros((nu, max(ku, 1)), dtype=np.float64)
    for u, v in us.items():
        ui[u, :len(v["indexes"])] = v["indexes"]
        uv[u, :len(v["indexes"])] = v["values"]
    return ui, uv


class Abi:
    """qrlsh_evaluate_grid called directly: the inputs on the device once, one call per grid"""

    def __init__(self, ratings, truth, coo, us, ku):
        self.nu, self.nq = ratings.shape
        src, dst, mil = (np.asarray(x) for x in coo)
        off = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=self.nq)))).astype(np.int64)
        ui, uv = padded_user_lists(us, self.nu, ku)
        self.ku = ku
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
        self.r = up(ratings.astype(np.int32))
        self.t = self.r if truth is None else up(truth.astype(np.int32))
        self.off, self.idx, self.mil = up(off), up(dst.astype(np.int32)), up(mil.astype(np.int32))
        self.ui, self.uv = up(ui), up(uv)
        self.lib = _lib.load()

    def __call__(self, q_cuts, u_cuts, weights, order="pairwise", seed=0, keep=EC.ALL, per_user=True, workspace=None,
                 ncq=None, ncu=None, nw=None):
        """-> (return code, totals [CQ][CU][W][8], per_user [nu][CQ][CU][W][8] or None, flags)"""
        w = np.asarray(weights, dtype=np.float64).reshape(-1, 3)
        ncq = len(q_cuts) if ncq is None else ncq
        ncu = len(u_cuts) if ncu is None else ncu
        nw = len(w) if nw is None else nw
        s = max(ncq * ncu * nw, 1)
        dq = torch.tensor(list(q_cuts) + [0] * 8, dtype=torch.int32, device=DEV)
        du = torch.tensor(list(u_cuts) + [0] * 8, dtype=torch.int32, device=DEV)
        dw = torch.from_numpy(np.concatenate([w, np.zeros((1, 3))])).to(DEV)
        totals = torch.full((s * 8,), -1, dtype=torch.int64, device=DEV)
        per = torch.full((max(self.nu, 1) * s * 8,), -1, dtype=torch.int64, device=DEV) if per_user else None
        flags = torch.full((1,), 0x55, dtype=torch.int32, device=DEV)
        need = int(self.lib.qrlsh_evaluate_grid_workspace_bytes(self.nu, self.nq, s))
        ws = torch.empty((max(need if workspace is None else workspace, 16),), dtype=torch.uint8, device=DEV)
        rc = self.lib.qrlsh_evaluate_grid(_ptr(self.r), _ptr(self.t), self.nu, self.nq, _ptr(self.off), _ptr(self.idx),
                                          _ptr(self.mil), _ptr(self.ui), _ptr(self.uv), self.ku, _ptr(dq), ncq, _ptr(du),
                                          ncu, _ptr(dw), nw, ORDER_WORD[order], seed, keep, _ptr(per), _ptr(totals),
                                          _ptr(flags), _ptr(ws), need if workspace is None else workspace, _stream())
        torch.cuda.synchronize()
        shape = (ncq, ncu, nw, 8)
        got_per = per.cpu().numpy()[:self.nu * s * 8].reshape((self.nu,) + shape) if per_user and rc == 0 else None
        return rc, (totals.cpu().numpy().reshape(shape) if rc == 0 else None), got_per, int(flags.item())


def assert_grid(got, want, what):
    """got: (rc, totals, per_user or None, flags) of the ABI; want: grid_ref's (pred, per_user, totals)"""
    rc, totals, per, flags = got
    assert rc == 0 and flags == 0, "%s: rc %d flags %d" % (what, rc, flags)
    bad = np.argwhere(totals != want[2])
    assert len(bad) == 0, "%s: totals differ at (cq, cu, w, word) %s: %s != %s" % (
        what, bad[:5].tolist(), totals[tuple(bad[0])], want[2][tuple(bad[0])])
    if per is not None:
        bad = np.argwhere(per != want[1])
        assert len(bad) == 0, "%s: per_user differs at (user, cq, cu, w, word) %s" % (what, bad[:5].tolist())
        assert np.array_equal(per.sum(axis=0), totals)


# ------------------------------------------------------------------------------------------------ 1. the main case
Q_CUTS, U_CUTS = [0, 7, 8, 64], [0, 1, 8, 9]


class Main:
    """nu = 3, nq = 2049, half of the cells rated; query lists of exactly 0, 1, 7, 8, 9, 15, 16, 17 and 64 entries
    planted at both ends; user lists of 9 (with repeats and the own user: only 3 users exist); 4 x 4 cuts x 8 weight
    triples = 128 settings, the limit.  The references are computed once: every rated cell in both orders, and a thin
    sample."""
    seed, thin = 7, 0.05

    def __init__(self):
        self.ratings, self.coo, self.qs, self.us = TC.planted_case(21, 3, 2049, 9)
        self.weights = TC.weight_grid(8, seed=3)
        self.cells, self.values = EC.evaluated_cells(self.ratings, 0, EC.ALL)
        self.want = {o: TC.grid_ref(self.ratings, self.qs, self.us, self.cells, self.values, Q_CUTS, U_CUTS,
                                    self.weights, summation=s) for o, s in ORDERS.items()}
        self.thin_cells, self.thin_values = EC.evaluated_cells(self.ratings, self.seed, EC.keep_of(self.thin))
        self.want_thin = TC.grid_ref(self.ratings, self.qs, self.us, self.thin_cells, self.thin_values, Q_CUTS, U_CUTS,
                                     self.weights)
        self._abi = None

    @property
    def abi(self):
        if self._abi is None:
            self._abi = Abi(self.ratings, None, self.coo, self.us, 9)
        return self._abi


@pytest.fixture(scope="module")
def main():
    return Main()


def test_main_case_at_the_limit_of_128_settings_in_both_orders(main):
    lens = {len(main.qs[j]["indexes"]) if j in main.qs else 0 for j in list(range(9)) + list(range(2040, 2049))}
    assert lens == {0, 1, 7, 8, 9, 15, 16, 17, 64} and len(main.cells) > 2500
    t = main.want["pairwise"][2]
    print("cells %d; n per query cut %s, per user cut %s" % (len(main.cells), t[:, 3, 0, 0].tolist(), t[3, :, 0, 0].tolist()))
    # the restatement alone: the cuts, the weights and the orders all show in the expected words
    assert len({tuple(x) for x in t.reshape(128, 8).tolist()}) > 100
    assert not np.array_equal(t, main.want["sequential"][2])
    assert t[0, 0, :, 0].sum() == 0 and (t[0, 0, :, 4] == len(main.cells)).all()       # both sides off: all missed
    assert (t[0, 1:, :, 6] == 0).all() and (t[1:, 0, :, 7] == 0).all() and (t[1:, 0, :3, 6] > 0).all()
    for o in ORDERS:
        assert_grid(main.abi(Q_CUTS, U_CUTS, main.weights, order=o), main.want[o], "main " + o)
        rc, totals, per, flags = main.abi(Q_CUTS, U_CUTS, main.weights, order=o, per_user=False)   # per_user_out NULL
        assert rc == 0 and flags == 0 and per is None and np.array_equal(totals, main.want[o][2])
        ev = qrlsh.evaluate_grid(main.ratings, *tensors(main.coo), main.us, main.weights, q_cuts=Q_CUTS, u_cuts=U_CUTS,
                                 sum_order=o, want_per_user=True, device=DEV)
        assert np.array_equal(ev.totals, main.want[o][2]) and ev.totals.dtype == np.int64
        assert np.array_equal(ev.per_user.cpu().numpy(), main.want[o][1])
        assert ev.q_cuts == Q_CUTS and ev.u_cuts == U_CUTS and np.array_equal(ev.weights, main.weights)
    n, sq, cells = (ev.totals[..., k].astype(np.float64) for k in (0, 3, 5))
    assert np.array_equal(ev.n, n) and np.array_equal(ev.coverage, n / cells)
    assert np.isnan(ev.rmse[0, 0]).all() and np.array_equal(ev.rmse[1:, 1:], np.sqrt(sq[1:, 1:] / n[1:, 1:]))
    q, u, w, index = ev.best()
    assert ev.rmse.reshape(-1)[index] == np.nanmin(ev.rmse) and ev.setting(index) == (q, u, w)


def test_a_thin_sample_runs_the_tail_drain_only(main):
    assert 50 < len(main.thin_cells) < 400
    keep = EC.keep_of(main.thin)
    assert_grid(main.abi(Q_CUTS, U_CUTS, main.weights, seed=main.seed, keep=keep), main.want_thin, "thin")
    ev = qrlsh.evaluate_grid(main.ratings, *tensors(main.coo), main.us, main.weights, q_cuts=Q_CUTS, u_cuts=U_CUTS,
                             fraction=main.thin, seed=main.seed, device=DEV)
    assert np.array_equal(ev.totals, main.want_thin[2]) and ev.per_user is None
    # nothing kept: zeros, no figures
    rc, totals, per, flags = main.abi(Q_CUTS, U_CUTS, main.weights, keep=0)
    assert rc == 0 and flags == 0 and not totals.any() and not per.any()


def test_the_queue_drains_inside_the_loop():
    """4096 users -> one slice of 2500 columns; three users' rows of truth are 90 % rated, so their workgroups predict
    1024 cells twice inside the loop and the rest after it; six more rows hold exactly 1, 1023, 1024, 1025, 2047 and 2048
    rated cells (both sides of one drain inside the loop and of the ring's wrap); every other workgroup evaluates nothing"""
    nu, nq = 4096, 2500
    ratings, coo, qs, us = EC.random_case(61, nu, nq, 10, 5, fill=0.3)
    rng = np.random.default_rng(62)
    truth = np.zeros_like(ratings)
    rows = [0, 1777, nu - 1]
    truth[rows] = (rng.integers(1, 101, size=(3, nq)) * (rng.random((3, nq)) < 0.9)).astype(np.int32)
    edges = [1, 513, 2048, 3000, 4000, nu - 2]
    EC.rows_with_exact_counts(truth, edges, [1024, 1, 2047, 1023, 1025, 2048], seed=63)
    cells, values = EC.evaluated_cells(truth, 0, EC.ALL)
    assert all(int((truth[r] != 0).sum()) > 2048 for r in rows)
    assert sorted(int((truth[r] != 0).sum()) for r in edges) == list(EC.QUEUE_EDGES)
    weights = TC.weight_grid(4, seed=5)
    want = TC.grid_ref(ratings, qs, us, cells, values, [3, 64], [2, 5], weights)
    assert_grid(Abi(ratings, truth, coo, us, 5)([3, 64], [2, 5], weights), want, "drain in the loop")


def test_one_setting_is_evaluate_through_the_word_mapping(main):
    for o in ORDERS:
        for fraction, seed in ((1.0, 0), (main.thin, main.seed)):
            ev = qrlsh.evaluate(main.ratings, *tensors(main.coo), main.us, fraction=fraction, seed=seed, sum_order=o,
                                device=DEV)
            rc, totals, per, flags = main.abi([64], [64], [TC.DEFAULT], order=o, seed=seed, keep=EC.keep_of(fraction))
            assert rc == 0 and flags == 0
            assert np.array_equal(totals[0, 0, 0], TC.words8(ev.totals)), o
            assert np.array_equal(per[:, 0, 0, 0], TC.words8(ev.per_user.cpu().numpy())), o
            grid = qrlsh.evaluate_grid(main.ratings, *tensors(main.coo), main.us, [TC.DEFAULT], fraction=fraction,
                                       seed=seed, sum_order=o, device=DEV)
            assert grid.q_cuts == [64] and grid.u_cuts == [64] and np.array_equal(grid.totals[0, 0, 0], totals[0, 0, 0])
            assert grid.rmse[0, 0, 0] == ev.rmse and grid.mae[0, 0, 0] == ev.mae and grid.bias[0, 0, 0] == ev.bias
            assert grid.coverage[0, 0, 0] == ev.coverage


# ------------------------------------------------------------------------------------------------ 2. row forms
def test_one_wide_rating_sends_that_row_to_memory(main):
    ratings = main.ratings.copy()
    ratings[1, 1000] = 300
    keep = EC.keep_of(0.1)
    cells, values = EC.evaluated_cells(ratings, 9, keep)
    assert (cells[:, 0] == 1).sum() > 50
    qs, reads = dict(main.qs), 0
    for j in cells[cells[:, 0] == 1][:40, 1].tolist():     # evaluated cells of that row whose lists read the 300
        if j in qs and j != 1000:
            qs[j] = {"indexes": np.concatenate(([1000], qs[j]["indexes"][1:])), "values": qs[j]["values"]}
            reads += 1
    assert reads > 10
    want = TC.grid_ref(ratings, qs, main.us, cells, values, Q_CUTS, U_CUTS, main.weights[:3])
    assert_grid(Abi(ratings, None, EC.coo_of(qs), main.us, 9)(Q_CUTS, U_CUTS, main.weights[:3], seed=9, keep=keep), want,
                "wide row")


def test_a_row_longer_than_the_lds_holds():
    nq = 131073
    ratings, coo, qs, us = EC.random_case(nq, 2, nq, 4, 2)
    keep = EC.keep_of(1500 / (0.5 * 2 * nq))
    cells, values = EC.evaluated_cells(ratings, 4, keep)
    assert 1000 < len(cells) < 2000 and cells[:, 1].max() > 131000
    weights = TC.weight_grid(3, seed=1)
    for o, s in ORDERS.items():
        want = TC.grid_ref(ratings, qs, us, cells, values, [2, 64], [1, 64], weights, summation=s)
        assert_grid(Abi(ratings, None, coo, us, 2)([2, 64], [1, 64], weights, order=o, seed=4, keep=keep), want,
                    "nq=131073 " + o)


# ------------------------------------------------------------------------------------------------ 3. knife edges
def test_knife_edge_cells_under_weights_that_keep_them_on_the_half():
    """default_mean = 60 + 10 m moves the query-only blend by 2 m and the user-only blend by 3 m, and the both-sides
    blend not at all: every knife-edge cell stays on k + 1/2 under each triple.  Cuts 8 / 9 / 64 change the pairwise
    shape of the lists; the held-out values sit on the knife cells only."""
    c = PC.build_case(16, nu=60, nq=700, tu=6, tq=60, user_longest=32)
    rng = np.random.default_rng(160)
    truth = np.zeros_like(c.ratings)
    truth[c.knife[:, 0], c.knife[:, 1]] = rng.integers(1, 101, size=len(c.knife))
    order = np.lexsort((c.knife[:, 1], c.knife[:, 0]))
    cells = c.knife[order]
    values = truth[cells[:, 0], cells[:, 1]]
    weights = [(0.6, 0.4, 60.0 + 10.0 * m) for m in (0, 1, -2, 4)]
    cuts = [8, 9, 64]
    ku = max(len(v["indexes"]) for v in c.us.values())
    abi = Abi(c.ratings, truth, [t.numpy() for t in c.coo()], c.us, ku)
    want = {o: TC.grid_ref(c.ratings, c.qs, c.us, cells, values, cuts, cuts, weights, summation=s)
            for o, s in ORDERS.items()}
    assert len(cells) > 100 and not np.array_equal(want["pairwise"][2], want["sequential"][2])
    assert not np.array_equal(want["pairwise"][2][0, 2], want["pairwise"][2][1, 2])
    for o in ORDERS:
        assert_grid(abi(cuts, cuts, weights, order=o), want[o], "knife " + o)
        ev = qrlsh.evaluate_grid(c.ratings, *c.coo(), c.us, weights, q_cuts=cuts, u_cuts=cuts, truth=truth, sum_order=o,
                                 device=DEV)
        assert np.array_equal(ev.totals, want[o][2])


# ------------------------------------------------------------------------------------------------ 4. weights, hold-out
def test_zero_weights_miss_every_covered_cell(main):
    keep = EC.keep_of(main.thin)
    weights = [(0.0, 0.0, 0.0), TC.DEFAULT]
    rc, totals, per, flags = main.abi([64], [9], weights, seed=main.seed, keep=keep)
    assert rc == 0 and flags == 0
    assert not totals[0, 0, 0, :4].any() and not totals[0, 0, 0, 6:].any()
    assert totals[0, 0, 0, 4] == totals[0, 0, 0, 5] == len(main.thin_cells) and totals[0, 0, 1, 0] > 0
    want = TC.grid_ref(main.ratings, main.qs, main.us, main.thin_cells, main.thin_values, [64], [9], weights)
    assert_grid((rc, totals, per, flags), want, "zero weights")


def test_a_holdout_evaluates_the_cells_it_zeroed(main):
    seed, fraction = 1234567890123, 0.08
    keep = EC.keep_of(fraction)
    train, count = EC.holdout_ref(main.ratings, seed, keep)
    cells, values = EC.evaluated_cells(main.ratings, seed, keep)
    assert len(cells) == count > 100 and not train[cells[:, 0], cells[:, 1]].any()
    weights = main.weights[:4]
    want = TC.grid_ref(train, main.qs, main.us, cells, values, [8, 64], [1, 9], weights)
    assert_grid(Abi(train, main.ratings, main.coo, main.us, 9)([8, 64], [1, 9], weights, seed=seed, keep=keep), want,
                "hold-out")
    dev_train, n = qrlsh.holdout(main.ratings, fraction, seed=seed, device=DEV)
    ev = qrlsh.evaluate_grid(dev_train, *tensors(main.coo), main.us, weights, q_cuts=[8, 64], u_cuts=[1, 9],
                             truth=main.ratings, fraction=fraction, seed=seed, device=DEV)
    assert n == count and np.array_equal(ev.totals, want[2])


def test_forty_weight_triples_take_two_calls(main):
    weights = TC.weight_grid(40, seed=9)
    want = TC.grid_ref(main.ratings, main.qs, main.us, main.thin_cells, main.thin_values, [7, 64], [1, 9], weights)
    ev = qrlsh.evaluate_grid(main.ratings, *tensors(main.coo), main.us, weights, q_cuts=[7, 64], u_cuts=[1, 9],
                             fraction=main.thin, seed=main.seed, want_per_user=True, device=DEV)
    assert ev.totals.shape == (2, 2, 40, 8) and np.array_equal(ev.totals, want[2])
    assert np.array_equal(ev.per_user.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------ 5. flags, limits
def test_flags_limits_and_empty_shapes(main):
    nu, nq = main.ratings.shape
    src, dst, mil = (np.asarray(x) for x in main.coo)
    w = [TC.DEFAULT]
    # a 65-entry list: bit 0, whatever the cuts
    keep = src != 600
    long_ = [np.concatenate([a[keep], b]) for a, b in ((src, np.full(65, 600)), (dst, np.arange(65)), (mil, np.full(65, 500)))]
    order = np.argsort(long_[0], kind="stable")
    long_ = [a[order] for a in long_]
    rc, _, _, flags = Abi(main.ratings, None, long_, main.us, 9)([1], [1], w)
    assert rc == 0 and flags == 1
    # an index >= nq: bit 1, whatever the cuts (the entry lies past every cut here)
    outside = dst.copy()
    at = int(np.flatnonzero(src == 2048)[-1])
    outside[at] = nq
    rc, _, _, flags = Abi(main.ratings, None, (src, outside, mil), main.us, 9)([1], [1], w)
    assert rc == 0 and flags == 2
    # a negative cut: bit 3
    for cuts in (([-1], [9]), ([64], [3, -2]), ([0, 1, 2, -5], [9])):
        rc, _, _, flags = main.abi(cuts[0], cuts[1], w, keep=EC.keep_of(0.01))
        assert rc == 0 and flags == 8
    with pytest.raises(ValueError, match="more than 64"):
        qrlsh.evaluate_grid(main.ratings, *tensors(long_), main.us, w, device=DEV)
    with pytest.raises(ValueError, match="neighbour index"):
        qrlsh.evaluate_grid(main.ratings, *tensors((src, outside, mil)), main.us, w, device=DEV)
    # limits: refused before any device work (the outputs keep their fill)
    abi = main.abi
    for kw in (dict(nw=129), dict(ncq=5), dict(nw=0), dict(ncu=0), dict(ncq=4, ncu=4, nw=9)):
        rc, _, _, flags = abi([64], [64], w, **kw)
        assert rc == _lib.QRLSH_EINVAL and flags == 0x55, kw
    rc, _, _, flags = abi(Q_CUTS, U_CUTS, main.weights, workspace=int(
        abi.lib.qrlsh_evaluate_grid_workspace_bytes(nu, nq, 128)) - 8)
    assert rc == _lib.QRLSH_EWORKSPACE and flags == 0x55
    assert abi.lib.qrlsh_evaluate_grid_workspace_bytes(nu, nq, 128) == 128 * abi.lib.qrlsh_evaluate_grid_workspace_bytes(nu, nq, 1)
    # no users: zeros
    rc, totals, per, flags = Abi(main.ratings[:0], None, main.coo, {}, 0)(Q_CUTS, [0, 1], main.weights[:2])
    assert rc == 0 and flags == 0 and totals.shape == (4, 2, 2, 8) and not totals.any() and per.size == 0
    # and the device is still sound
    assert_grid(abi(Q_CUTS, U_CUTS, main.weights, seed=main.seed, keep=EC.keep_of(main.thin)), main.want_thin, "afterwards")


# ------------------------------------------------------------------------------------------------ 6. Recommender
def _index_lists(ui):
    idx, milli, n = (t.cpu().numpy() for t in (ui.idx, ui.milli, ui.len))
    return {u: {"indexes": idx[u, :n[u]].astype(np.int64), "values": milli[u, :n[u]] / 1000.0} for u in range(ui.nu)}


def test_recommender_tunes_and_serves_the_chosen_blend():
    import recommender as R
    from test_gpu_recommend import _recommender_on
    from qrlsh import users
    rec, g = _recommender_on("cfg1")
    nu, nq = rec.ratings.shape
    rec.compute_querySimilarities()
    rec.live_user_similarities(labels=users.cluster_labels(rec.ratings))
    ui = rec.user_index
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == (R.QUERY_WEIGHT, R.USER_WEIGHT, R.DEFAULT_MEAN)
    before = rec.ratings.copy()
    held = [t.clone() for t in (ui.ratings, ui.idx, ui.milli, ui.len)]
    lists = [np.asarray(qrlsh.ops.to_host(x)).copy() for x in rec._live_lists()]
    # the single default setting: evaluate(holdout=True)'s totals
    one = rec.tune([(R.QUERY_WEIGHT, R.USER_WEIGHT, R.DEFAULT_MEAN)], fraction=0.2, seed=3)
    ev = rec.evaluate(holdout=True, fraction=0.2, seed=3)
    assert one.totals.shape == (1, 1, 1, 8) and np.array_equal(one.totals[0, 0, 0], TC.words8(ev.totals)) and ev.n > 300
    loo = rec.tune([(R.QUERY_WEIGHT, R.USER_WEIGHT, R.DEFAULT_MEAN)], fraction=1.0, holdout=False)
    assert np.array_equal(loo.totals[0, 0, 0], TC.words8(rec.evaluate().totals))
    # a grid whose best setting is not the default; cuts are reported, not applied
    weights = [(R.QUERY_WEIGHT, R.USER_WEIGHT, R.DEFAULT_MEAN)] + [(qw, 1.0 - qw, dm) for qw in (0.2, 0.5, 0.8)
                                                                   for dm in (30.0, 45.0, 75.0)]
    grid = rec.tune(weights, q_cuts=[4, 64], u_cuts=[0, 64], fraction=0.2, seed=3, apply=True)
    q_cut, u_cut, triple, index = grid.best()
    print("best setting %d: cuts %d / %d, weights %s, rmse %.4f (default %.4f)" % (
        index, q_cut, u_cut, triple, grid.rmse.reshape(-1)[index], grid.rmse[1, 1, 0]))
    assert triple != weights[0] and np.array_equal(grid.totals[1, 1, 0], one.totals[0, 0, 0])
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == triple
    assert (R.Recommender.query_weight, R.Recommender.user_weight, R.Recommender.default_mean) == (0.6, 0.4, 60)
    assert np.array_equal(rec.ratings, before) and rec.user_index is ui
    assert all(torch.equal(a, b) for a, b in zip(held, (ui.ratings, ui.idx, ui.milli, ui.len)))
    assert all(np.array_equal(a, np.asarray(qrlsh.ops.to_host(b))) for a, b in zip(lists, rec._live_lists()))
    # serving uses the chosen triple
    qs, us = rec.current_query_similarities(), _index_lists(ui)
    summation = ORDERS[rec.sum_order]
    serve = [0, 5, nu - 1]
    cells = np.array([(u, j) for u in serve for j in range(nq)])
    want = O.predict_cells(rec.ratings, qs, us, cells, summation=summation, query_weight=triple[0], user_weight=triple[1],
                           default_mean=triple[2]).reshape(len(serve), nq)
    default = O.predict_cells(rec.ratings, qs, us, cells, summation=summation).reshape(len(serve), nq)
    assert not np.array_equal(want, default)
    assert np.array_equal(rec.predict_users(serve).to_numpy(), want)
    out = rec.recommend_users(serve, 10)
    for row, u in enumerate(serve):
        cand = np.flatnonzero((rec.ratings[u] == 0) & (want[row] != 0))
        top = cand[np.lexsort((cand, -want[row][cand]))][:10]
        assert np.array_equal(out[u]["indexes"], top) and np.array_equal(out[u]["values"], want[row][top])
        assert out[u]["available"] == len(cand)
    # evaluate() reports that setting's figures (the whole lists: the cuts are not applied)
    w = weights.index(triple)
    assert np.array_equal(TC.words8(rec.evaluate(holdout=True, fraction=0.2, seed=3).totals), grid.totals[1, 1, w])
    with pytest.raises(ValueError, match="no setting"):
        rec.tune(weights, fraction=0.2, seed=3, min_coverage=1.5, apply=True)
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == triple


def test_a_fresh_recommender_still_reproduces_the_golden_predictions():
    from test_gpu_recommend import _recommender_on
    rec, g = _recommender_on("cfg1")
    assert np.array_equal(rec.compute_scores()[1].to_numpy(), g["final"])
