"""The rules behind set_list_length, pinned on the host against the oracle (no GPU): the cut as a predicate on src, the
prefix property it rests on, the regrow from the rows of exactly K_old entries, both again for the dense user lists, and
the counts the GPU tests take for granted."""
import numpy as np
import pytest

import list_length_cases as LL
import lists_update_cases as LC
import user_lists_cases as UC

B = LC.CROWDED["b"]


@pytest.fixture(scope="module")
def crowded_full():
    """(hi, K) -> the oracle's lists, computed once per setting"""
    memo = {}

    def get(hi, K):
        if (hi, K) not in memo:
            memo[(hi, K)] = LC.full_lists(LC.crowded(hi), B, K)
        return memo[(hi, K)]
    return get


@pytest.mark.parametrize("hi", [3, 40])
def test_cut_predicate_is_the_cut_and_a_prefix_is_the_shorter_list(crowded_full, hi):
    for K_old in (4, 64):
        stored = crowded_full(hi, K_old)
        for K2 in (K_old, K_old - 1, 3, 2, 1):
            got = LL.restate_cut(stored, K2)
            assert LC.same(got, LC.cut(*stored, K2)), (hi, K_old, K2)
            assert LC.same(got, crowded_full(hi, K2)), (hi, K_old, K2, "prefix property")
    # i < K2 at the first row, K2 beyond the whole list
    short = tuple(a[:3] for a in crowded_full(hi, 4))
    assert LL.cut_mask(short[0], 5).all() and LL.cut_mask(np.empty(0, dtype=np.int32), 2).size == 0


def test_cut_counts(crowded_full):
    for K, entries in LL.CUT_ENTRIES_40.items():
        assert len(LL.restate_cut(crowded_full(40, 4), K)[0]) == entries == len(crowded_full(40, K)[0])
    for K in (1, 5, 63, 64):
        assert len(LL.restate_cut(crowded_full(3, 64), K)[0]) == K * 323


@pytest.mark.parametrize("case", sorted(LL.REGROWS))
def test_regrow_from_the_full_rows(crowded_full, case):
    hi, K_old, K2 = case
    picked_n, before, after = LL.REGROWS[case]
    stored = crowded_full(hi, K_old)
    got, picked = LL.restate_regrow(stored, LC.crowded(hi), B, K_old, K2)
    assert LC.same(got, crowded_full(hi, K2)), case
    assert (len(picked), len(stored[0]), len(got[0])) == (picked_n, before, after), case
    # the mark's rule is the rows' lengths
    rows, counts = np.unique(stored[0], return_counts=True)
    assert np.array_equal(picked, rows[counts == K_old]) and counts.max() <= K_old
    if case == (3, 4, 256):
        assert np.unique(got[0], return_counts=True)[1].max() == 219
    if case == (40, 4, 6):
        assert (counts < K_old).sum() == 236


def test_round_trip(crowded_full):
    for hi in (3, 40):
        cut = LL.restate_cut(crowded_full(hi, 4), 2)
        assert LC.same(LL.restate_regrow(cut, LC.crowded(hi), B, 2, 4)[0], crowded_full(hi, 4))


# ---- the user side ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def user_cases():
    return UC.build_cases()


def test_user_cut_and_regrow_are_the_reference_at_the_new_length(user_cases):
    for name, c in user_cases.items():
        K = c["K"]
        stored = UC.reference_lists(c["ratings"], c["labels"], K)
        cuts, grows = LL.user_targets(K)
        for K2 in cuts:
            assert UC.same(LL.user_cut(stored, K2), UC.reference_lists(c["ratings"], c["labels"], K2)), (name, K2)
        for K2 in grows:
            got, full = LL.user_regrow(stored, c["ratings"], c["labels"], K, K2)
            assert UC.same(got, UC.reference_lists(c["ratings"], c["labels"], K2)), (name, K2)
            assert len(full) == (stored[2] == K).sum()


def test_user_counts(user_cases):
    for name, (full, short) in LL.USER_FULL.items():
        c = user_cases[name]
        ln = UC.reference_lists(c["ratings"], c["labels"], c["K"])[2]
        assert ((ln == c["K"]).sum(), ((ln > 0) & (ln < c["K"])).sum()) == (full, short), name
    c = user_cases["ties_at_the_cut"]
    assert UC.reference_lists(c["ratings"], c["labels"], 64)[2].max() == 8
    c = user_cases["mixed_K19"]
    for K2 in (22, 64):
        assert len(LL.user_regrow(UC.reference_lists(c["ratings"], c["labels"], 19), c["ratings"], c["labels"], 19, K2)[1]) == 80
    c = user_cases["cluster_smaller_than_K"]      # a regrow that rescores nothing: the lists as they were, restrided
    stored = UC.reference_lists(c["ratings"], c["labels"], c["K"])
    got, full = LL.user_regrow(stored, c["ratings"], c["labels"], c["K"], c["K"] + 3)
    assert len(full) == 0 and np.array_equal(got[0][:, :c["K"]], stored[0]) and (got[0][:, c["K"]:] == -1).all()
    assert user_cases["mixed_K64"]["K"] == 64 and LL.user_targets(64) == ([1, 63], [])


def test_library_declares_the_entry_points():
    from qrlsh import _lib
    for name in ("qrlsh_lists_cut_workspace_bytes", "qrlsh_lists_cut_count", "qrlsh_lists_cut_fill",
                 "qrlsh_lists_regrow_mark", "qrlsh_index_pick_keys"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["qrlsh_lists_cut_fill"][1]) == 14
