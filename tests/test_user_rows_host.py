"""The rules of the user-row operations, on the host (tests/user_rows_cases.py): for every case the restated rule gives
the numpy lists of the new matrix, each named case shows the property it is named for, and the nearest rule equals a
brute-force loop.  No GPU."""
import numpy as np
import pytest

import user_lists_cases as UC
import user_rows_cases as RC

CASES = RC.build_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_rule_equals_the_lists_of_the_new_matrix(name):
    c = CASES[name]
    before, after, picked = RC.restated(c)
    want = UC.reference_lists(c["new"], c["all_labels"], c["K"])
    assert UC.same(after, want), name
    assert c["new"].shape[0] == len(c["all_labels"]) == want[2].size
    if c["op"] == "add":
        assert picked == [], name             # no stored entry names a new id
        assert np.array_equal(c["new"][:c["ratings"].shape[0]], c["ratings"])
    else:
        keep = c["new_pos"] >= 0
        assert np.array_equal(c["new_pos"][keep], np.arange(keep.sum())) and np.array_equal(c["new"], c["ratings"][keep])
        if name in RC.PICKS:
            assert picked, name
        if name in RC.NO_PICKS:
            assert picked == [], name


def _old_rows(c, lists):
    nu = c["ratings"].shape[0]
    return tuple(a[:nu] for a in lists)


def test_add_cases_show_what_they_are_named_for():
    def parts(name):
        c = CASES[name]
        before, after, _ = RC.restated(c)
        return c, before, after, c["ratings"].shape[0]

    c, before, after, nu = parts("into_short_rows")
    assert (before[2][:4] < c["K"]).all() and all(nu in after[0][v] for v in range(4))
    assert np.array_equal(after[2][:4], before[2][:4] + 1) and after[2][nu] == 4

    c, before, after, nu = parts("outranks_full_rows")
    K = c["K"]
    assert (before[2] == K).all()
    pushed = [v for v in range(nu) if nu in after[0][v] and before[0][v, K - 1] not in after[0][v]]
    assert pushed and all(after[2][v] == K for v in pushed)

    c, before, after, nu = parts("ranks_below_full_rows")
    assert (before[2] == c["K"]).all() and UC.same(_old_rows(c, after), before) and after[2][nu] > 0

    c, before, after, nu = parts("ties_the_Kth_entry")
    K = c["K"]
    assert UC.same(_old_rows(c, after), before)
    mm = RC.cross_milli(c["ratings"], c["rows"])[0]
    tied = [v for v in range(nu) if before[2][v] == K and mm[v] == before[1][v, K - 1]]
    assert tied and all(nu > before[0][v, K - 1] for v in tied)      # equal value, larger id: the newcomer loses

    c, before, after, nu = parts("two_newcomers_one_cluster")
    assert nu + 1 in after[0][nu] and nu in after[0][nu + 1]

    c, before, after, nu = parts("two_clusters_and_a_new_label")
    assert after[0][nu + 1, :after[2][nu + 1]].tolist() in ([nu + 3], []) and set(after[0][nu + 1][:1]) <= {nu + 3, -1}
    assert set(after[0][nu, :after[2][nu]]) <= set(range(5)) and set(after[0][nu + 2, :after[2][nu + 2]]) <= set(range(5, 9))
    assert after[2][nu] > 0 and after[2][nu + 2] > 0
    assert not any(x in after[0][:nu] for x in (nu + 1, nu + 3))

    c, before, after, nu = parts("unrated_newcomer")
    assert after[2][nu] == 0 and UC.same(_old_rows(c, after), before)

    c, before, after, nu = parts("nu_crosses_an_id_map_word")
    assert nu == 31 and after[2].size == 33 and after[2][31] > 0 and after[2][32] > 0


def test_assignment_cases_show_what_they_are_named_for():
    c = CASES["copy_of_an_existing_user"]
    user, milli, _ = RC.nearest_rule(c["ratings"], c["rows"])
    assert (user.tolist(), milli.tolist(), c["returned"].tolist()) == ([7], [1000], [8])
    c = CASES["identical_users_lowest_id_wins"]
    user, milli, mm = RC.nearest_rule(c["ratings"], c["rows"])
    assert mm[0, 2] == mm[0, 7] == 1000 and user.tolist() == [2] and c["returned"].tolist() == [3]
    c = CASES["nothing_positive_own_cluster"]
    user, milli, mm = RC.nearest_rule(c["ratings"], c["rows"])
    assert (mm <= 0).all() and (mm < 0).any() and (user.tolist(), milli.tolist()) == ([-1], [0])
    assert c["returned"].tolist() == [4]
    c = CASES["two_own_clusters_in_one_batch"]
    assert c["returned"].tolist() == [4, 3, 5]
    # the rule does not look at the other rows of the batch: any order gives every row the same nearest user
    user, milli, _ = RC.nearest_rule(c["ratings"], c["rows"])
    u2, m2, _ = RC.nearest_rule(c["ratings"], c["rows"][::-1])
    assert np.array_equal(user, u2[::-1]) and np.array_equal(milli, m2[::-1])


def test_remove_cases_show_what_they_are_named_for():
    c = CASES["nobody_names_the_user"]
    before, after, picked = RC.restated(c)
    assert not (before[0] == 9).any() and UC.same(after, tuple(a[:9] for a in before))
    c = CASES["named_by_short_rows_only"]
    before, after, picked = RC.restated(c)
    assert (before[0] == 1).any() and (before[2] < c["K"]).all() and not picked
    c = CASES["named_by_full_rows"]
    before, after, picked = RC.restated(c)
    assert (before[2] == c["K"]).all() and picked and (after[2] == c["K"]).all()      # six survivors: five neighbours each
    c = CASES["whole_cluster_removed"]
    assert sorted(set(c["all_labels"].tolist())) == [0, 2]
    c = CASES["first_and_last_user"]
    assert c["new_pos"][0] == c["new_pos"][9] == -1 and c["new_pos"][1] == 0
    c = CASES["duplicates_in_the_ids"]
    assert (c["new_pos"] < 0).sum() == 2 and c["new"].shape[0] == 8
    c = CASES["all_users_but_one"]
    _, after, _ = RC.restated(c)
    assert c["new"].shape[0] == 1 and after[2].tolist() == [0]
    c = CASES["cluster_left_with_one_member"]
    before, after, _ = RC.restated(c)
    assert before[2][6] > 0 and after[2][c["new_pos"][6]] == 0
    c = CASES["ties_at_the_cut"]
    before, after, picked = RC.restated(c)
    assert picked and any(before[1][v, c["K"] - 1] == 1000 for v in picked)


def test_mixed_matrix_spans_five_id_map_words():
    for K in (1, 19, 64):
        a, n, r = CASES["mixed_K%d_add" % K], CASES["mixed_K%d_add_nearest" % K], CASES["mixed_K%d_remove" % K]
        assert a["ratings"].shape[0] == 150 and a["new"].shape[0] == 156 and r["new"].shape[0] == 136
        assert int(r["users"].max()) >= 128
        assert len(set(n["returned"].tolist())) >= 2


def test_nearest_rule_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    r = np.vstack((UC._like_minded(rng, 9, 23), UC._random(rng, 6, 23), np.zeros((1, 23), dtype=np.int64)))
    r[3] = r[1]
    rows = np.vstack((r[1], UC._random(rng, 4, 23), np.zeros((1, 23), dtype=np.int64), np.where(r[0] > 0, 101 - r[0], 0)))
    user, milli, mm = RC.nearest_rule(r, rows)
    nu = r.shape[0]
    for k in range(rows.shape[0]):
        scores = UC.pair_milli(np.vstack((r, rows[k:k + 1])), [(nu, u) for u in range(nu)])
        assert np.array_equal(mm[k], scores), k
        best_u, best = -1, 0
        for u in range(nu):
            if scores[u] > best:
                best_u, best = u, int(scores[u])
        assert (user[k], milli[k]) == (best_u, best), k
    assert user[0] == 1 and milli[0] == 1000 and (user[5], milli[5]) == (-1, 0)
