"""The claim the list update rests on, checked on the CPU: the stored rows plus the scored new pairs, cut at K
(lists_update_cases.restate_update), are element for element the oracle's lists over all rows -- for every hold-out
fixture and for crowded shapes where nearly every row is cut at K and ties at the cut are common."""
import numpy as np
import pytest

import lists_update_cases as LC
import query_index_cases as QC
from helpers import FULL, check_topk_tie_aware, pairs_u64


def _check(sig, b, K, bounds, what):
    n = bounds[0]
    want = LC.full_lists(sig[:bounds[-1]], b, K)
    got = LC.restate_batches(LC.full_lists(sig[:n], b, K), sig, n, bounds[1:], b, K)
    assert LC.same(got, want), what
    return got


@pytest.mark.parametrize("name", QC.HOLDOUT_SETS)
def test_restatement_equals_the_oracle_on_every_fixture(name):
    from oracle import oracle as O
    g, sig, b, K = next((g, sig, b, K) for nm, g, sig, b, K in QC.golden_sets() if nm == name)
    N = sig.shape[0]
    for h in LC.holdouts(N):
        got = _check(sig, b, K, [N - h, N], (name, h))
    if name in FULL:      # the reference's own lists, through the tie-aware comparison
        pairs = O.candidates_from_sig(sig, b)
        assert np.array_equal(pairs, pairs_u64(g["pairs"]))
        check_topk_tie_aware(g, pairs, O.score_pairs(sig, pairs), got[0], got[1], got[2], K)


def test_only_the_ties_fixture_has_rows_the_cut_shortens():
    cutting = [nm for nm, g, sig, b, K in QC.golden_sets() if LC.rows_cut(sig, b, K)[0]]
    assert cutting == ["full_p160_ties"]


@pytest.mark.parametrize("hi", [3, 40])
def test_crowded_and_sparse_shapes_in_one_batch_and_in_three(hi):
    c = LC.CROWDED
    sig = LC.crowded(hi)
    N, b, K = c["N"], c["b"], c["K"]
    ncut, npairs = LC.rows_cut(sig, b, K)
    if hi == 3:
        assert ncut > 300 and npairs > 20000          # nearly every row is cut, ties at the cut everywhere
    else:
        assert 0 < ncut < 40                          # sparse: most rows shorter than K
        first = LC.full_lists(sig[:300], b, K)[0]
        assert set(np.unique(LC.full_lists(sig, b, K)[0])[:].tolist()) - set(range(300, N)) > set(np.unique(first).tolist())
    for n in (0, 40, 300, 339):
        _check(sig, b, K, [n, N], (hi, n))
    _check(sig, b, K, [300, 313, 326, N], (hi, "three batches"))
    _check(sig, b, K, [0, 1, 2, N], (hi, "from nothing in three"))


def test_wide_bands_and_the_popular_key():
    c = LC.WIDE
    _check(LC.wide(), c["b"], c["K"], [c["n"], c["N"]], "wide")
    p = LC.POPULAR
    sig = LC.popular()
    _check(sig, p["b"], p["K"], [p["n"], p["n"] + p["m"]], "popular")
