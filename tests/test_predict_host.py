"""The knife-edge prediction cases (tests/predict_cases.py) checked with the oracle alone: the builder really
builds cells whose float64 prediction depends on the summation order, on half-to-even rounding and on FMA
contraction, in every branch of the blend and on both sides -- so that tests/test_gpu_predict.py, which holds
the kernel to oracle.predict_cells on them, would notice a kernel that got any of these wrong.  And
predict_cells, which those tests use on samples of large matrices, equals the whole-matrix predict_scores."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import GENERATOR_SETS, load
from oracle import oracle as O
import predict_cases as PC

N = 20   # every "at least N cells" threshold below


@pytest.fixture(scope="module")
def case():
    return PC.build_case(2024, nu=1500, nq=6000, tu=24, tq=120)


def _sides(case, i, j, sum_q, sum_u):
    """(qp, up) of cell (i, j) with the given summation on each side (oracle.weighted_average)"""
    ql = case.qs.get(int(j))
    qp = 0.0 if ql is None else O.weighted_average(case.ratings[i], ql["indexes"], ql["values"], sum_q)
    ul = case.us[int(i)]
    up = O.weighted_average(case.ratings[:, j], ul["indexes"], ul["values"], sum_u)
    return qp, up


def _blend(qp, up, fma=None):
    """recommender.py:324-331 in float64; fma: evaluate the final multiply-add as one fused operation, on the
    first ('a') or the second ('b') product of the both-sides sum"""
    def mul_add(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c)) if fma else a * b + c
    if up == 0 and qp == 0:
        return 0.0
    if up == 0:
        return mul_add(qp, O.QUERY_WEIGHT + (O.USER_WEIGHT * 0.5), O.DEFAULT_MEAN * (O.USER_WEIGHT * 0.5))
    if qp == 0:
        return mul_add(up, O.USER_WEIGHT + (O.QUERY_WEIGHT * 0.5), O.DEFAULT_MEAN * (O.QUERY_WEIGHT * 0.5))
    if fma == "b":
        return mul_add(up, O.USER_WEIGHT, qp * O.QUERY_WEIGHT)
    return mul_add(qp, O.QUERY_WEIGHT, up * O.USER_WEIGHT)


def _real_side(vec, lst):
    """the weighted average in exact arithmetic (weights = milli / 1000, so the ratio of milli sums)"""
    r = np.asarray(vec)[lst["indexes"]].astype(np.int64)
    w = np.rint(lst["values"] * 1000).astype(np.int64)
    nz = r != 0
    if not nz.any() or w[nz].sum() == 0:
        return Fraction(0)
    return Fraction(int((r * w).sum()), int(w[nz].sum()))


def test_builder_layout_lengths_and_interleaving(case):
    """targets are zero; private blocks are disjoint; the spare query is in no list; list lengths cover 1-7,
    8-32 (n % 8 != 0 and == 0) and 33-64 on both sides; unrated neighbours are interleaved (m < n, m < 8 <= n)"""
    tu, tq = 24, 120
    assert len(case.knife) >= 0.9 * tu * tq
    assert (case.ratings[case.knife[:, 0], case.knife[:, 1]] == 0).all()
    qblocks = np.concatenate([case.qs[j]["indexes"] for j in range(tq) if j in case.qs])
    ublocks = np.concatenate([case.us[i]["indexes"] for i in range(tu)])
    assert len(np.unique(qblocks)) == len(qblocks) and qblocks.min() >= tq
    assert len(np.unique(ublocks)) == len(ublocks) and ublocks.min() >= tu
    assert all(case.spare not in v["indexes"] for v in case.qs.values())
    for lens in ([len(case.qs[j]["indexes"]) for j in range(tq) if j in case.qs],
                 [len(case.us[i]["indexes"]) for i in range(tu)]):
        lens = np.array(lens)
        assert ((lens >= 1) & (lens <= 7)).any() and ((lens > 32) & (lens <= 64)).any()
        assert ((lens >= 8) & (lens <= 32) & (lens % 8 == 0)).any()
        assert ((lens > 8) & (lens < 32) & (lens % 8 != 0)).any()
    for side in ("q", "u"):
        n_m = []
        for (i, j), b in zip(case.knife, case.branch):
            if b in (side, "b"):   # the sides the cell's branch reads
                lst = case.qs[int(j)] if side == "q" else case.us[int(i)]
                vec = case.ratings[i] if side == "q" else case.ratings[:, j]
                n_m.append((len(lst["indexes"]), int((vec[lst["indexes"]] != 0).sum())))
        n_m = np.array(n_m)
        assert (n_m[:, 1] < n_m[:, 0]).sum() >= N, side
        assert ((n_m[:, 1] < 8) & (n_m[:, 0] >= 8)).sum() >= N, side
        assert ((n_m[:, 1] >= 8) & (n_m[:, 1] % 8 != 0)).sum() >= N, side


def test_knife_cells_are_exactly_half_in_real_arithmetic(case):
    """every knife cell takes the branch it was built for, and its blend in exact arithmetic is k + 1/2"""
    assert set(case.branch.tolist()) == set(PC.BRANCHES)
    for (i, j), b in zip(case.knife, case.branch):
        qp = _real_side(case.ratings[i], case.qs[int(j)]) if int(j) in case.qs else Fraction(0)
        up = _real_side(case.ratings[:, j], case.us[int(i)])
        assert (qp != 0) == (b in ("q", "b")) and (up != 0) == (b in ("u", "b")), (i, j, b)
        v = PC.blend_real(b, qp, up)
        assert v - (v.numerator // v.denominator) == Fraction(1, 2), (i, j, b)


def test_knife_cells_tell_summation_orders_rounding_and_fma_apart(case):
    """with the oracle only: at least N cells round differently under numpy's pairwise and a sequential sum in
    each branch, and when only the query side's or only the user side's order changes; at least N cells are
    exactly on .5 in float64 with an even and with an odd floor (half-to-even vs half-up); at least N cells
    change when the blend's final multiply-add is one FMA"""
    pw, sq = O.np_sum_order, PC.sequential_sum
    flips = {b: 0 for b in PC.BRANCHES}
    side = {"q": 0, "u": 0}
    half = {0: 0, 1: 0}
    fma = 0
    for (i, j), b in zip(case.knife, case.branch):
        p = _sides(case, i, j, pw, pw)
        r = round(_blend(*p))
        if round(_blend(*_sides(case, i, j, sq, sq))) != r:
            flips[b] += 1
        if round(_blend(*_sides(case, i, j, sq, pw))) != r:
            side["q"] += 1
        if round(_blend(*_sides(case, i, j, pw, sq))) != r:
            side["u"] += 1
        x = _blend(*p)
        if x - np.floor(x) == 0.5:
            half[int(np.floor(x)) % 2] += 1
        if round(_blend(*p, fma="a")) != r or round(_blend(*p, fma="b")) != r:
            fma += 1
    assert min(flips.values()) >= N, flips
    assert min(side.values()) >= N, side
    assert min(half.values()) >= N, half
    assert fma >= N, fma


def test_predict_cells_equals_predict_scores_on_a_knife_case():
    c = PC.build_case(7, nu=160, nq=400, tu=6, tq=12)
    assert len(c.knife) >= 50
    for summation in (O.np_sum_order, PC.sequential_sum):
        full = O.predict_scores(c.ratings, c.qs, c.us, summation=summation)
        cells = np.argwhere(np.ones_like(c.ratings, dtype=bool))
        got = O.predict_cells(c.ratings, c.qs, c.us, cells, summation=summation)
        assert np.array_equal(got.reshape(full.shape), full)
    # the weights are parameters: the defaults reproduce the constants; other values move knife cells
    k = c.knife
    a = O.predict_cells(c.ratings, c.qs, c.us, k)
    assert np.array_equal(a, O.predict_cells(c.ratings, c.qs, c.us, k, query_weight=0.6, user_weight=0.4,
                                             default_mean=60))
    assert not np.array_equal(a, O.predict_cells(c.ratings, c.qs, c.us, k, query_weight=0.7, user_weight=0.3,
                                                 default_mean=55))


@pytest.mark.parametrize("sub", GENERATOR_SETS)
def test_predict_cells_equals_predict_scores_on_golden_sets(sub):
    """on the reference's own lists and finalPredictions (tests/golden/<sub>_scores.npz)"""
    g, h = load(sub + "_scores"), load(sub + "_hotpath")
    qs = {int(q): {"indexes": h["qs_idx"][h["qs_off"][k]:h["qs_off"][k + 1]].astype(np.int64),
                   "values": h["qs_val"][h["qs_off"][k]:h["qs_off"][k + 1]]} for k, q in enumerate(h["qs_q"])}
    us = {}
    for u in range(len(g["ratings"])):
        n = int((g["us_idx"][u] >= 0).sum())
        us[u] = {"indexes": g["us_idx"][u][:n].astype(np.int64), "values": g["us_val"][u][:n]}
    full = O.predict_scores(g["ratings"], qs, us)
    cells = np.argwhere(np.ones_like(g["ratings"], dtype=bool))
    got = O.predict_cells(g["ratings"], qs, us, cells).reshape(full.shape)
    assert np.array_equal(got, full) and np.array_equal(got, g["final"])
