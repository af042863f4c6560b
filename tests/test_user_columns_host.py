"""The numpy side of the live user lists' column operations (tests/user_columns_cases.py), without a GPU: with R taken
by the changed-values rule the restated update gives the lists of a full recompute over the new matrix, the rows outside
R keep their mean and norm, each case has the property it is named for, and the new entry points of the library refuse
bad sizes and return at once on empty batches."""
import ctypes

import numpy as np
import pytest

import user_columns_cases as CC
import user_lists_cases as UC


@pytest.fixture(scope="module")
def cases():
    return CC.build_cases()


@pytest.fixture(scope="module")
def lists(cases):
    """per case: (the lists before, the lists of the new matrix, (restated lists, picked)) -- computed once"""
    out = {}
    for name, c in cases.items():
        old = UC.reference_lists(c["ratings"], c["labels"], c["K"])
        out[name] = (old, UC.reference_lists(c["new"], c["labels"], c["K"]),
                     UC.restated_update(old, c["new"], c["labels"], c["K"], c["R"]))
    return out


def test_restated_update_over_the_new_columns_equals_full_recompute(cases, lists):
    for name in cases:
        _, fresh, (got, _) = lists[name]
        assert UC.same(got, fresh), name


def _stats(r):
    c = UC.centred(r)
    nz = r != 0
    mean = np.where(nz.any(axis=1), r.sum(axis=1) / np.maximum(nz.sum(axis=1), 1), 0.0)
    return mean, (c * c).sum(axis=1)


def test_rows_outside_R_keep_mean_and_norm(cases):
    for name, c in cases.items():
        out = np.setdiff1d(np.arange(c["ratings"].shape[0]), c["R"])
        (m0, n0), (m1, n1) = _stats(c["ratings"]), _stats(c["new"])
        assert np.array_equal(m0[out], m1[out]) and np.array_equal(n0[out], n1[out]), name
        # and their dots with each other: the affected columns hold equal values on both sides
        c0, c1 = UC.centred(c["ratings"])[out], UC.centred(c["new"])[out]
        assert np.array_equal(c0 @ c0.T, c1 @ c1.T), name


def test_cases_have_the_properties_they_are_named_for(cases, lists):
    for name, c in cases.items():
        assert (len(c["R"]) == 0) == (name in CC.R_EMPTY), name
    for name in CC.PICKS:
        assert len(lists[name][2][1]) > 0, name
    nq = 37
    c = cases["unrated_columns_appended"]
    assert c["new"].shape[1] == nq + 3 and not c["new"][:, nq:].any()
    assert cases["block_appended_two_users_rated"]["R"].tolist() == [1, 7]
    c = cases["never_rated_column_removed"]
    assert not c["ratings"][:, 5].any() and c["new"].shape[1] == nq - 1
    c = cases["rated_column_removed"]
    assert 0 < len(c["R"]) and c["R"].tolist() == np.flatnonzero(c["ratings"][:, 7]).tolist()
    c = cases["first_and_last_column_removed"]
    assert np.array_equal(c["new"], c["ratings"][:, 1:nq - 1])
    c = cases["duplicates_in_cols"]
    assert len(c["cols"]) > len(set(c["cols"].tolist())) == 3 and c["new"].shape[1] == nq - 3
    c = cases["every_column_but_one_removed"]
    assert np.array_equal(c["new"], c["ratings"][:, 11:12])
    c = cases["every_column_removed"]
    assert c["new"].shape == (11, 0) and (lists["every_column_removed"][1][2] == 0).all()
    c = cases["equal_values_overwritten"]
    assert np.array_equal(c["new"], c["ratings"])
    c = cases["overwrites_to_zero_from_zero_and_between"]
    o, n = c["ratings"], c["new"]
    assert o[1, 4] and not n[1, 4] and not o[2, 30] and n[2, 30] and o[3, 17] and n[3, 17] and o[3, 17] != n[3, 17]
    assert c["R"].tolist() == [1, 2, 3]
    c = cases["agreed_columns_removed"]
    assert c["R"].tolist() == [0, 1] and lists["agreed_columns_removed"][0][2][2:].max() == c["K"]
    c = cases["R_is_a_whole_cluster"]
    assert set(c["R"]) == set(np.flatnonzero(c["labels"] == 0))
    c = cases["two_clusters_at_once"]
    assert len(set(c["labels"][c["R"]])) >= 3
    c = cases["ties_at_the_cut"]
    assert not UC.no_tie_straddles_the_cut(c["ratings"], c["labels"], c["K"])
    assert not UC.no_tie_straddles_the_cut(c["new"], c["labels"], c["K"])
    for K in (1, 19, 64):
        for op in ("add", "remove", "set"):
            c = cases["mixed_K%d_%s" % (K, op)]
            assert c["K"] == K and c["op"] == op and c["ratings"].shape == (150, 37) and 0 < len(c["R"]) < 150
            lab = c["labels"]
            assert (np.diff(lab) != 0).sum() > 50            # clusters interleaved in id order
    assert (lists["mixed_K64_set"][0][2] == 64).any()


def test_new_entry_points_check_sizes_without_a_gpu():
    from qrlsh import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: the arguments are refused first
    big = 1 << 31
    for nu, nq, m in ((-1, 4, 1), (big, 4, 1), (4, -1, 1), (4, big, 1), (4, 4, -1)):
        rc = lib.qrlsh_ratings_columns_changed(one, nu, nq, one, one, m, one, one, None)
        assert rc == _lib.QRLSH_EINVAL and b"columns_changed" in lib.qrlsh_last_error(), (nu, nq, m)
    for nu, nq, nq2, m in ((-1, 4, 4, 1), (big, 4, 4, 1), (4, -1, 4, 1), (4, big, 4, 1), (4, 4, -1, 1), (4, 4, big, 1),
                           (4, 4, 4, -1)):
        rc = lib.qrlsh_ratings_columns_move(one, nu, nq, one, nq2, one, m, one, one, None)
        assert rc == _lib.QRLSH_EINVAL and b"columns_move" in lib.qrlsh_last_error(), (nu, nq, nq2, m)
    # an output that is not 16-byte aligned is refused
    assert lib.qrlsh_ratings_columns_move(one, 4, 4, one, 4, one, 1, ctypes.c_void_p(20), one, None) == _lib.QRLSH_EINVAL
    # empty batches return at once, whatever the pointers
    assert lib.qrlsh_ratings_columns_changed(None, 4, 4, None, None, 0, None, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_ratings_columns_changed(None, 0, 4, None, None, 3, None, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_ratings_columns_move(None, 4, 4, None, 4, None, 0, None, None, None) == _lib.QRLSH_OK
    assert lib.qrlsh_ratings_columns_move(None, 0, 4, None, 5, None, 1, None, None, None) == _lib.QRLSH_OK
