"""The ranking grid on the device (qrlsh_evaluate_ranking_grid, qrlsh.evaluate_ranking_grid, Recommender.tune_ranking).
Expected values come from the numpy restatement of tests/rank_grid_cases.py (tune_cases' sides and blend handed to
rank_eval_cases.rank_eval_ref, candidates="heldout"), never from the code under test; every comparison is integer
equality.  Every test calls qrlsh.evaluate_ranking_grid or the library entry behind it."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
import evaluate_cases as EC
import predict_cases as PC
import rank_eval_cases as REC
import rank_grid_cases as RGC
import tune_cases as TC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib, recommend  # noqa: E402
from qrlsh.ops import _ptr, _stream  # noqa: E402

DEV = "cuda"
ORDERS = {"pairwise": O.np_sum_order, "sequential": PC.sequential_sum}
ORDER_WORD = {"pairwise": _lib.SUM_PAIRWISE, "sequential": _lib.SUM_SEQUENTIAL}


def tensors(coo):
    return tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo)


def run(train, truth, coo, us, k, relevant, weights, **kw):
    kw.setdefault("want_per_request", True)
    return qrlsh.evaluate_ranking_grid(train, truth, *tensors(coo), us, k, relevant, weights, device=DEV, **kw)


def assert_grid(ev, want, what):
    """ev: a RankingGridEvaluation with per_request; want: rank_grid_ref's (per, totals, idx)"""
    assert ev.totals.dtype == np.int64 and ev.totals.shape == want[1].shape, what
    bad = np.argwhere(ev.totals != want[1])
    assert len(bad) == 0, "%s: totals differ at (cq, cu, w, word) %s: %s != %s" % (
        what, bad[:5].tolist(), ev.totals[tuple(bad[0])], want[1][tuple(bad[0])])
    per = ev.per_request.cpu().numpy()
    assert per.shape == want[0].shape and per.dtype == np.int64, what
    bad = np.argwhere(per != want[0])
    assert len(bad) == 0, "%s: lines differ at (request, cq, cu, w, word) %s: %s != %s" % (
        what, bad[:5].tolist(), per[tuple(bad[0])], want[0][tuple(bad[0])])
    assert (per[..., 2] == per[..., 0]).all()                                    # known == listed in this mode


class Abi:
    """qrlsh_evaluate_ranking_grid called directly: the inputs on the device once, one call per grid"""

    def __init__(self, train, truth, coo, us, ku):
        self.nu, self.nq = train.shape
        src, dst, mil = (np.asarray(x) for x in coo)
        off = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=self.nq)))).astype(np.int64)
        ui = np.full((self.nu, max(ku, 1)), -1, dtype=np.int32)
        uv = np.zeros((self.nu, max(ku, 1)), dtype=np.float64)
        for u, v in us.items():
            ui[u, :len(v["indexes"])] = v["indexes"]
            uv[u, :len(v["indexes"])] = v["values"]
        self.ku = ku
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
        self.r, self.t = up(train.astype(np.int32)), up(truth.astype(np.int32))
        self.off, self.idx, self.mil = up(off), up(dst.astype(np.int32)), up(mil.astype(np.int32))
        self.ui, self.uv = up(ui), up(uv)
        self.cells = int(((train == 0) & (truth != 0)).sum())
        self.lib = _lib.load()

    def __call__(self, q_cuts, u_cuts, weights, k=5, relevant=50, users=None, gains=None, cells=None, workspace=None,
                 ncq=None, ncu=None, nw=None, order="pairwise"):
        """-> (return code, totals [CQ][CU][W][16], lines [m][CQ][CU][W][8], flags, cells counted)"""
        w = np.asarray(weights, dtype=np.float64).reshape(-1, 3)
        ncq = len(q_cuts) if ncq is None else ncq
        ncu = len(u_cuts) if ncu is None else ncu
        nw = len(w) if nw is None else nw
        s = max(ncq * ncu * nw, 1)
        m = self.nu if users is None else len(users)
        kk = max(1, min(k, 1024))
        g = np.array(REC.dcg_gains_ref(kk) if gains is None else gains, dtype=np.int64)
        dg = torch.from_numpy(g).to(DEV)
        dp = torch.from_numpy(np.concatenate(([0], np.cumsum(g)))).to(DEV)
        dq = torch.tensor(list(q_cuts) + [0] * 8, dtype=torch.int32, device=DEV)
        du = torch.tensor(list(u_cuts) + [0] * 8, dtype=torch.int32, device=DEV)
        dw = torch.from_numpy(np.concatenate([w, np.zeros((1, 3))])).to(DEV)
        ut = None if users is None else torch.tensor(list(users) + [0], dtype=torch.int32, device=DEV)
        totals = torch.full((s * 16,), -1, dtype=torch.int64, device=DEV)
        lines = torch.full((max(m, 1) * s * 8,), -7, dtype=torch.int64, device=DEV)
        flags = torch.full((1,), 0x55, dtype=torch.int32, device=DEV)
        counted = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        cells = (self.cells * 4 if users is not None else self.cells) if cells is None else cells
        need = int(self.lib.qrlsh_evaluate_ranking_grid_workspace_bytes(m, self.nq, min(ncq, 4), min(ncu, 4),
                                                                        min(s, 128), cells))
        ws = torch.empty((max(need if workspace is None else workspace, 16),), dtype=torch.uint8, device=DEV)
        rc = self.lib.qrlsh_evaluate_ranking_grid(
            _ptr(self.r), _ptr(self.t), self.nu, self.nq, _ptr(self.off), _ptr(self.idx), _ptr(self.mil), _ptr(self.ui),
            _ptr(self.uv), self.ku, _ptr(dq), ncq, _ptr(du), ncu, _ptr(dw), nw, ORDER_WORD[order], _ptr(ut), m, k,
            relevant, _ptr(dg), _ptr(dp), cells, _ptr(lines), _ptr(totals), _ptr(counted), _ptr(flags), _ptr(ws),
            need if workspace is None else workspace, _stream())
        torch.cuda.synchronize()
        if rc != 0:
            return rc, None, None, int(flags.item()), int(counted.item())
        return (rc, totals.cpu().numpy().reshape(ncq, ncu, nw, 16),
                lines.cpu().numpy()[:m * s * 8].reshape(m, ncq, ncu, nw, 8), int(flags.item()), int(counted.item()))


# ------------------------------------------------------------------------------------------------ 1. the main case
class Main:
    """24 x 700, planted list lengths at both ends, user lists of 9, 27 requests (three users named twice); 4 x 4 cuts x
    8 weight triples = 128 settings, the limit of a call; k = 10.  The references are computed once per sum order."""

    def __init__(self):
        self.case = RGC.main_case()
        self.train, self.truth, self.coo, self.qs, self.us, self.users = self.case
        self.weights = RGC.main_weights()
        self.want = {o: RGC.main_expected(self.case, s) for o, s in ORDERS.items()}
        self._abi = None

    @property
    def abi(self):
        if self._abi is None:
            self._abi = Abi(self.train, self.truth, self.coo, self.us, 9)
        return self._abi


@pytest.fixture(scope="module")
def main():
    return Main()


def test_main_case_at_the_limit_of_128_settings_in_both_orders(main):
    t = main.want["pairwise"][1]
    print("test cells %d relevant %d; hits per query cut %s, per user cut %s" % (
        t[3, 3, 0, 6], t[3, 3, 0, 5], t[:, 3, 0, 1].tolist(), t[3, :, 0, 1].tolist()))
    # the restatement alone: the cuts and the weights show in the expected words; the counts do not move
    assert len({tuple(x) for x in t.reshape(128, 16)[:, :5].tolist()}) > 60
    assert not t[0, 0, :, :5].any() and (t[..., 6] == t[0, 0, 0, 6]).all() and (t[..., 8] == len(main.users)).all()
    assert t[3, 3, 0, 1] > 20 and t[3, 3, 0, 6] > 1500
    for o in ORDERS:
        ev = run(main.train, main.truth, main.coo, main.us, RGC.MAIN_K, RGC.MAIN_RELEVANT, main.weights,
                 q_cuts=RGC.MAIN_Q_CUTS, u_cuts=RGC.MAIN_U_CUTS, users=main.users, sum_order=o)
        assert_grid(ev, main.want[o], "main " + o)
        assert ev.q_cuts == RGC.MAIN_Q_CUTS and ev.u_cuts == RGC.MAIN_U_CUTS and np.array_equal(ev.weights, main.weights)
    # the two one-sided triples rank the same cells differently (asserted on the expected lists in the case module)
    assert not np.array_equal(ev.totals[3, 3, 1, :5], ev.totals[3, 3, 2, :5])
    tt = ev.totals.astype(np.float64)
    assert np.array_equal(ev.ndcg[1:, 1:], tt[1:, 1:, :, 4] / tt[1:, 1:, :, 11]) and np.isnan(ev.precision[0, 0]).all()
    q, u, w, index = ev.best()
    assert ev.ndcg.reshape(-1)[index] == np.nanmax(ev.ndcg) and ev.setting(index) == (q, u, w)
    # no lines asked for: the totals alone
    plain = run(main.train, main.truth, main.coo, main.us, RGC.MAIN_K, RGC.MAIN_RELEVANT, main.weights[:3],
                users=main.users, want_per_request=False)
    assert plain.per_request is None and np.array_equal(plain.totals[0, 0], main.want["pairwise"][1][3, 3, :3])


def test_four_settings_agree_with_evaluate_ranking_over_host_cut_lists(main):
    per = run(main.train, main.truth, main.coo, main.us, RGC.MAIN_K, RGC.MAIN_RELEVANT, main.weights,
              q_cuts=RGC.MAIN_Q_CUTS, u_cuts=RGC.MAIN_U_CUTS, users=main.users)
    lines = per.per_request.cpu().numpy()
    for a, b, w in ((3, 3, 0), (1, 2, 1), (2, 1, 2), (3, 0, 5)):
        cqs, cus = RGC.host_cut_lists(main.qs, main.us, RGC.MAIN_Q_CUTS[a], RGC.MAIN_U_CUTS[b])
        qw, uw, dm = main.weights[w]
        one = qrlsh.evaluate_ranking(main.train, main.truth, *tensors(EC.coo_of(cqs)), cus, RGC.MAIN_K, RGC.MAIN_RELEVANT,
                                     users=main.users, candidates="heldout", query_weight=qw, user_weight=uw,
                                     default_mean=dm, device=DEV)
        assert np.array_equal(one.per_user.cpu().numpy(), lines[:, a, b, w]), (a, b, w)
        assert np.array_equal(one.totals, per.totals[a, b, w])
        assert one.ndcg == per.ndcg[a, b, w] and one.precision == per.precision[a, b, w]
        assert one.recall == per.recall[a, b, w] and one.hit_rate == per.hit_rate[a, b, w]


# ------------------------------------------------------------------------------------------------ 2. queue and tiles
@pytest.fixture(scope="module")
def queue():
    train, truth, coo, qs, us = REC.queue_case()
    sides = RGC.sides_of_test_cells(train, truth, qs, us, range(train.shape[0]), [64], [64])
    return train, truth, coo, qs, us, sides


@pytest.mark.parametrize("k", [1, 100, 1024])
def test_queue_and_tile_edges(queue, k):
    """test cells per user 0, 1, 1023, 1024, 1025, 2047, 2048, 4100 (and 2048 in runs) at nq = 8192: the sweep's queue
    fills, overflows and drains, the rank kernel's 256-record tiles end everywhere, and avail lies on both sides of k"""
    train, truth, coo, qs, us, sides = queue
    weights = [TC.DEFAULT, RGC.USER_ONLY]
    want = RGC.rank_grid_ref(train, truth, qs, us, None, k, 60, REC.dcg_gains_ref(k), [64], [64], weights, sides=sides)
    counts = list(REC.QUEUE_COUNTS) + [2048]
    avail = want[0][:, 0, 0, 0, 7]
    assert want[0][:, 0, 0, 0, 6].tolist() == counts and (avail <= counts).all() and avail[2] == 1023 and avail[7] == 4100
    assert_grid(run(train, truth, coo, us, k, 60, weights), want, "queue k=%d" % k)


@pytest.mark.parametrize("k", [1, 2, 257, 1024])
def test_avail_just_below_at_and_just_above_k(k):
    train, truth, coo, qs, us = RGC.avail_case(k)
    weights = [TC.DEFAULT, (0.2, 1.0, 35.0)]
    want = RGC.rank_grid_ref(train, truth, qs, us, None, k, 50, REC.primes(k), [64], [64], weights)
    assert want[0][:, 0, 0, 0, 7].tolist() == [k - 1, k, k + 1] and want[0][:, 0, 0, 0, 0].tolist() == [k - 1, k, k]
    assert_grid(run(train, truth, coo, us, k, 50, weights, gains=np.array(REC.primes(k))), want, "avail around k=%d" % k)


# ------------------------------------------------------------------------------------------------ 3. ties and the cut
@pytest.mark.parametrize("k", [1, 64, 1024])
def test_ties_across_the_cut(k):
    """cut_case's users under the default blend, under one where only default_mean survives (every prediction equal: the
    list is the first k candidate columns) and under zero weights (nothing is listed)"""
    train, truth, coo, qs, us, rows = REC.cut_case(k)
    weights = [TC.DEFAULT, (-0.5, 1.0, 60.0), (0.0, 0.0, 60.0), (0.3, 1.0, 20.0)]
    gains = REC.primes(k)
    want = RGC.rank_grid_ref(train, truth, qs, us, None, k, REC.CUT_RELEVANT, gains, [64], [64], weights)
    per = want[0][:, 0, 0]
    assert per[rows["first"], 0, 3] == 1 and per[rows["nothing"], 0].tolist() == [0, 0, 0, 0, 0, 2, 2, 0]
    assert per[rows["ties"], 0, 5] > per[rows["ties"], 0, 1] and per[rows["no_relevant"], 0, 5] == 0
    assert not per[:, 2, :5].any() and not per[:, 2, 7].any()                      # zero weights: no candidates
    u = rows["no_relevant"]                                                        # all equal: the first k columns
    cand = np.flatnonzero((train[u, :REC.CUT_TARGETS] == 0) & (truth[u, :REC.CUT_TARGETS] != 0)
                          & (train[u, REC.CUT_TARGETS:] != 0))
    assert want[2][u, 0, 0, 1, :min(k, len(cand))].tolist() == cand[:k].tolist()
    ev = run(train, truth, coo, us, k, REC.CUT_RELEVANT, weights, gains=np.array(gains))
    assert_grid(ev, want, "cut k=%d" % k)


def test_zero_weights_and_equal_predictions_on_two_sided_cells(main):
    weights = [(0.0, 0.0, 60.0), (-0.5, 1.0, 60.0), (1.0, -0.5, 40.0)]
    want = RGC.rank_grid_ref(main.train, main.truth, main.qs, main.us, main.users, 10, 60, REC.dcg_gains_ref(10),
                             [64], [0, 9], weights)
    assert not want[1][0, 1, 0, :5].any() and want[1][0, 0, 1, 0] > 100
    assert_grid(run(main.train, main.truth, main.coo, main.us, 10, 60, weights, u_cuts=[0, 9], users=main.users), want,
                "zero and constant")


# ------------------------------------------------------------------------------------------------ 4. any int32 value
def test_predictions_outside_any_window_in_one_call(main):
    weights = [(-0.6, 0.4, 60.0), (0.6, 0.4, 1e6), (0.6, 0.4, -1e6), (-1.5, -2.0, 7.0), (300.0, 200.0, 60.0), TC.DEFAULT]
    want = RGC.rank_grid_ref(main.train, main.truth, main.qs, main.us, main.users, 10, 60, REC.primes(10), [8, 64],
                             [1, 9], weights)
    sides = RGC.sides_of_test_cells(main.train, main.truth, main.qs, main.us, [0], [64], [9])
    pred = np.array([[RGC.setting_predictions(sides, [0], 700, 0, 0, tuple(w))[0]] for w in weights])
    assert pred.min() < -100000 and pred.max() > 100000 and (pred[3] < 0).sum() > 20
    assert_grid(run(main.train, main.truth, main.coo, main.us, 10, 60, weights, q_cuts=[8, 64], u_cuts=[1, 9],
                    users=main.users, gains=REC.primes(10)), want, "far apart")


# ------------------------------------------------------------------------------------------------ 5. knife edges
def test_knife_edge_cells_under_weights_that_keep_them_on_the_half():
    """default_mean = 60 + 10 m moves the one-sided blends by whole numbers and the two-sided blend not at all: every
    knife-edge cell stays on k + 1/2, and the sum order decides which way it falls"""
    train, truth, coo, qs, us = REC.knife_split(11, 37, 700, held=0.3)
    weights = [(0.6, 0.4, 60.0 + 10.0 * m) for m in (0, 1, -2, 4)]
    users = list(range(REC.KNIFE_USERS)) + [20, 36]
    want = {o: RGC.rank_grid_ref(train, truth, qs, us, users, 12, 50, REC.dcg_gains_ref(12), [8, 64], [8, 64], weights,
                                 summation=s) for o, s in ORDERS.items()}
    assert not np.array_equal(want["pairwise"][2], want["sequential"][2])
    for o in ORDERS:
        assert_grid(run(train, truth, coo, us, 12, 50, weights, q_cuts=[8, 64], u_cuts=[8, 64], users=users,
                        sum_order=o), want[o], "knife " + o)


# ------------------------------------------------------------------------------------------------ 6. row routes
def test_one_wide_rating_sends_that_row_to_memory(main):
    train, truth = main.train.copy(), main.truth.copy()
    col = int(np.flatnonzero(train[1] != 0)[5])
    train[1, col] = truth[1, col] = 300
    qs, reads = dict(main.qs), 0
    for j in np.flatnonzero((train[1] == 0) & (truth[1] != 0))[:40].tolist():   # test cells whose lists read the 300
        if j in qs:
            qs[j] = {"indexes": np.concatenate(([col], qs[j]["indexes"][1:])), "values": qs[j]["values"]}
            reads += 1
    assert reads > 10
    weights = main.weights[:3]
    want = RGC.rank_grid_ref(train, truth, qs, main.us, [0, 1, 2], 10, 60, REC.dcg_gains_ref(10), [7, 64], [9], weights)
    plain = RGC.rank_grid_ref(main.train, main.truth, qs, main.us, [1], 10, 60, REC.dcg_gains_ref(10), [7, 64], [9],
                              weights)
    assert not np.array_equal(want[2][1], plain[2][0])                          # the 300 moves user 1's lists
    assert_grid(run(train, truth, EC.coo_of(qs), main.us, 10, 60, weights, q_cuts=[7, 64], u_cuts=[9], users=[0, 1, 2]),
                want, "wide row")


def test_a_row_longer_than_the_lds_holds():
    nq = 131073
    train, truth, coo, qs, us = REC.split_case(nq, 3, nq, fill=0.05, held=0.1, longest_q=4, ku=2)
    cells = int(((train == 0) & (truth != 0)).sum())
    assert 1000 < cells < 3000 and np.flatnonzero((train == 0) & (truth != 0))[-1] % nq > 131000
    weights = [TC.DEFAULT, RGC.QUERY_ONLY]
    want = RGC.rank_grid_ref(train, truth, qs, us, None, 28, 60, REC.dcg_gains_ref(28), [2, 64], [64], weights)
    assert want[1][1, 0, 0, 1] > 0
    assert_grid(run(train, truth, coo, us, 28, 60, weights, q_cuts=[2, 64]), want, "nq=131073")


# ------------------------------------------------------------------------------------------------ 7. calls and blocks
def test_forty_triples_take_two_calls_and_request_blocks_add_up(main, monkeypatch):
    weights = TC.weight_grid(40, seed=9)
    users = [5, 0, 23, 5, 11, 2, 17, 9]
    args = dict(q_cuts=[7, 64], u_cuts=[1, 9], users=users)
    want = RGC.rank_grid_ref(main.train, main.truth, main.qs, main.us, users, 10, 60, REC.dcg_gains_ref(10), [7, 64],
                             [1, 9], weights)
    ev = run(main.train, main.truth, main.coo, main.us, 10, 60, weights, **args)
    assert ev.totals.shape == (2, 2, 40, 16) and tuple(ev.per_request.shape) == (8, 2, 2, 40, 8)
    assert_grid(ev, want, "two calls")
    for lo, hi in ((0, 32), (32, 40)):                                          # the one-call slices
        part = run(main.train, main.truth, main.coo, main.us, 10, 60, weights[lo:hi], **args)
        assert np.array_equal(part.totals, ev.totals[:, :, lo:hi])
        assert torch.equal(part.per_request, ev.per_request[:, :, :, lo:hi])
    lib = _lib.load()
    cells = ((main.train == 0) & (main.truth != 0)).sum(axis=1)[users]
    budget = int(lib.qrlsh_evaluate_ranking_grid_workspace_bytes(3, 700, 2, 2, 128, int(cells.max()) * 3))
    assert budget < int(lib.qrlsh_evaluate_ranking_grid_workspace_bytes(8, 700, 2, 2, 128, int(cells.sum())))
    monkeypatch.setattr(recommend, "WORKSPACE_BUDGET", budget)                  # 8 -> 4 -> 2 requests per block
    assert_grid(run(main.train, main.truth, main.coo, main.us, 10, 60, weights, **args), want, "blocks")
    dev = [torch.from_numpy(x).to(DEV) for x in (main.train, main.truth)]      # device matrices: counted on the device
    assert_grid(run(dev[0], dev[1], main.coo, main.us, 10, 60, weights, q_cuts=[7, 64], u_cuts=[1, 9],
                    users=torch.tensor(users, device=DEV)), want, "blocks, device inputs")


# ------------------------------------------------------------------------------------------------ 8. flags, limits
def test_flags_limits_and_empty_shapes(main):
    nu, nq = main.train.shape
    src, dst, mil = (np.asarray(x) for x in main.coo)
    w = [TC.DEFAULT]
    abi = main.abi
    want = RGC.rank_grid_ref(main.train, main.truth, main.qs, main.us, [4, 4, 0], 5, 50, REC.dcg_gains_ref(5), [64], [9], w)
    rc, totals, lines, flags, counted = abi([64], [9], w, users=[4, 4, 0])
    assert rc == 0 and flags == 0 and np.array_equal(totals, want[1]) and np.array_equal(lines, want[0])
    assert counted == want[1][0, 0, 0, 6]
    # a 65-entry list: bit 0; an index of nq: bit 1 -- whatever the cuts
    keep = src != 600
    long_ = [np.concatenate([a[keep], b]) for a, b in ((src, np.full(65, 600)), (dst, np.arange(65)), (mil, np.full(65, 500)))]
    order = np.argsort(long_[0], kind="stable")
    long_ = [a[order] for a in long_]
    assert Abi(main.train, main.truth, long_, main.us, 9)([1], [1], w)[3] == 1
    outside = dst.copy()
    outside[int(np.flatnonzero(src == 699)[-1])] = nq
    assert Abi(main.train, main.truth, (src, outside, mil), main.us, 9)([1], [1], w)[3] == 2
    with pytest.raises(ValueError, match="more than 64"):
        run(main.train, main.truth, long_, main.us, 5, 50, w)
    with pytest.raises(ValueError, match="neighbour index"):
        run(main.train, main.truth, (src, outside, mil), main.us, 5, 50, w)
    # a user id of nu: a zero line with avail -1, nothing in the totals, bit 2; ValueError from the host layer
    rc, totals, lines, flags, _ = abi([64], [9], w, users=[4, nu, 0])
    assert rc == 0 and flags == 4 and lines[1, 0, 0, 0].tolist() == [0] * 7 + [-1]
    assert np.array_equal(lines[[0, 2]], want[0][[0, 2]]) and totals[0, 0, 0, 8] == 2
    assert np.array_equal(totals[0, 0, 0, :8], want[0][[0, 2], 0, 0, 0].sum(axis=0))
    with pytest.raises(ValueError, match="user id"):
        run(main.train, main.truth, main.coo, main.us, 5, 50, w, users=torch.tensor([3, nu], device=DEV))
    # a negative gain, a negative cut: bit 3
    assert abi([64], [9], w, gains=[5, 4, -3, 2, 1])[3] == 8
    for cuts in (([-1], [9]), ([64], [3, -2]), ([0, 1, 2, -5], [9])):
        assert abi(cuts[0], cuts[1], w)[3] == 8
    # fewer record slots than test cells: bit 4, nothing written past them
    rc, totals, lines, flags, counted = abi([64], [9], w, users=[4, 4, 0], cells=int(want[1][0, 0, 0, 6]) - 1)
    assert rc == 0 and flags == 16 and counted == want[1][0, 0, 0, 6]
    # limits: refused before any device work (the outputs keep their fill)
    for kw in (dict(ncq=5), dict(ncu=5), dict(nw=129), dict(nw=0), dict(ncq=4, ncu=4, nw=9), dict(k=0), dict(k=1025),
               dict(relevant=0), dict(cells=-1)):
        rc, _, _, flags, counted = abi([64], [9], w, **kw)
        assert rc == _lib.QRLSH_EINVAL and flags == 0x55 and counted == -1, kw
    need = int(abi.lib.qrlsh_evaluate_ranking_grid_workspace_bytes(nu, nq, 1, 1, 1, abi.cells))
    rc, _, _, flags, _ = abi([64], [9], w, workspace=need - 16)
    assert rc == _lib.QRLSH_EWORKSPACE and flags == 0x55
    assert abi.lib.qrlsh_evaluate_ranking_grid_workspace_bytes(nu, nq, 1, 1, 129, 10) == 0
    grow = [int(abi.lib.qrlsh_evaluate_ranking_grid_workspace_bytes(nu, nq, 2, 2, 8, c)) for c in (0, 1000, 2000)]
    assert grow[2] - grow[1] == grow[1] - grow[0] == 1000 * (8 + 8 * 4)              # it follows the test cells
    # m = 0, nq = 0, a user without a test cell
    rc, totals, lines, flags, counted = abi([64], [9], w, users=[])
    assert rc == 0 and flags == 0 and not totals.any() and counted == 0
    ev = run(main.train, main.truth, main.coo, main.us, 5, 50, w, users=[])
    assert not ev.totals.any() and tuple(ev.per_request.shape) == (0, 1, 1, 1, 8) and np.isnan(ev.ndcg).all()
    none = np.zeros((4, 0), dtype=np.int32)
    empty = tuple(np.zeros(0, dtype=np.int32) for _ in range(3))
    ev = run(none, none, empty, {}, 3, 50, w, users=[3, 0])
    assert ev.per_request.cpu().numpy().reshape(2, 8).tolist() == [[0] * 8] * 2
    assert ev.totals.reshape(16).tolist() == [0] * 8 + [2] + [0] * 7
    train = main.train.copy()
    train[7] = main.truth[7]                                                        # user 7 holds nothing out
    ev = run(train, main.truth, main.coo, main.us, 5, 50, w, users=[7, 4])
    assert ev.per_request.cpu().numpy()[0].reshape(8).tolist() == [0] * 8 and ev.totals[0, 0, 0, 8] == 2
    # and the device is still sound
    rc, totals, lines, flags, _ = abi([64], [9], w, users=[4, 4, 0])
    assert rc == 0 and flags == 0 and np.array_equal(lines, want[0])


# ------------------------------------------------------------------------------------------------ 9. Recommender
def test_recommender_tunes_for_the_order_of_its_lists():
    import recommender as R
    from test_gpu_recommend import _recommender_on
    from qrlsh import users
    rec, g = _recommender_on("cfg1")
    with pytest.raises(ValueError, match="no live lists"):
        rec.tune_ranking(5, 60, [TC.DEFAULT])
    rec.compute_querySimilarities()
    rec.live_user_similarities(labels=users.cluster_labels(rec.ratings))
    ui = rec.user_index
    before = rec.ratings.copy()
    held = [t.clone() for t in (ui.ratings, ui.idx, ui.milli, ui.len)]
    triples = [(R.QUERY_WEIGHT, R.USER_WEIGHT, float(R.DEFAULT_MEAN)), (1.0, 0.0, 50.0), (0.1, 0.9, 30.0)]
    k, relevant, fraction, seed = 7, 60, 0.3, 11
    grid = rec.tune_ranking(k, relevant, triples, fraction=fraction, seed=seed)
    assert grid.totals.shape == (1, 1, 3, 16) and grid.totals[0, 0, 0, 1] > 0
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == (R.QUERY_WEIGHT, R.USER_WEIGHT, R.DEFAULT_MEAN)
    for w, triple in enumerate(triples):                      # the existing route with the attributes set by hand
        rec.query_weight, rec.user_weight, rec.default_mean = triple
        one = rec.evaluate_ranking(k, relevant, fraction=fraction, seed=seed, candidates="heldout")
        assert np.array_equal(one.totals, grid.totals[0, 0, w]), triple
        assert one.ndcg == grid.ndcg[0, 0, w] and one.recall == grid.recall[0, 0, w]
    del rec.query_weight, rec.user_weight, rec.default_mean
    assert len({tuple(t) for t in grid.totals[0, 0, :, :5].tolist()}) >= 2
    some = rec.tune_ranking(k, relevant, triples, fraction=fraction, seed=seed, users=[0, 5, 5], q_cuts=[4, 64])
    assert some.totals.shape == (2, 1, 3, 16) and (some.totals[..., 8] == 3).all()
    best = rec.tune_ranking(k, relevant, triples, fraction=fraction, seed=seed, metric="precision", apply=True)
    q_cut, u_cut, triple, index = best.best("precision")
    assert np.array_equal(best.totals, grid.totals) and triple == triples[index]
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == triple
    assert (R.Recommender.query_weight, R.Recommender.user_weight, R.Recommender.default_mean) == (0.6, 0.4, 60)
    with pytest.raises(ValueError, match="no setting"):
        rec.tune_ranking(k, relevant, triples, fraction=fraction, seed=seed, min_recall=1.5, apply=True)
    with pytest.raises(ValueError, match="metric"):
        rec.tune_ranking(k, relevant, triples, metric="rmse")
    assert (rec.query_weight, rec.user_weight, rec.default_mean) == triple
    assert np.array_equal(rec.ratings, before) and rec.user_index is ui
    assert all(torch.equal(a, b) for a, b in zip(held, (ui.ratings, ui.idx, ui.milli, ui.len)))


def test_a_fresh_recommender_still_reproduces_the_golden_predictions():
    from test_gpu_recommend import _recommender_on
    rec, g = _recommender_on("cfg1")
    assert qrlsh.evaluate_ranking_grid is not None and hasattr(rec, "tune_ranking")
    assert np.array_equal(rec.compute_scores()[1].to_numpy(), g["final"])
