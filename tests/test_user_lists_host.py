"""The numpy side of the live user lists (tests/user_lists_cases.py), without a GPU: the restated update rule gives
the lists of a full recompute on every case, each case has the property it is named for, and the restated lists are
the reference's (oracle.user_similarities_from_labels) wherever the reference's arbitrary tie order cannot show."""
import os

import numpy as np
import pytest

import user_lists_cases as UC
from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    c = UC.build_cases()
    c["big_cluster"] = UC.big_cluster_case()
    return c


def test_restated_update_equals_full_recompute(cases):
    for name, c in cases.items():
        old = UC.reference_lists(c["ratings"], c["labels"], c["K"])
        got, _ = UC.restated_update(old, c["new"], c["labels"], c["K"], c["R"])
        assert UC.same(got, UC.reference_lists(c["new"], c["labels"], c["K"])), name


def test_cases_have_the_properties_they_are_named_for(cases):
    def lists(name, which):
        c = cases[name]
        return UC.reference_lists(c[which], c["labels"], c["K"])

    def picked(name):
        c = cases[name]
        return UC.restated_update(lists(name, "ratings"), c["new"], c["labels"], c["K"], c["R"])[1]

    assert cases["one_user"]["ratings"].shape[0] == 1
    c = cases["cluster_smaller_than_K"]
    assert np.bincount(c["labels"]).max() < c["K"]
    c = cases["cluster_of_K_plus_1"]
    assert (c["labels"] == 3).sum() == c["K"] + 1 and (lists("cluster_of_K_plus_1", "ratings")[2][:c["K"] + 1] == c["K"]).all()
    c = cases["ties_at_the_cut"]
    assert not UC.no_tie_straddles_the_cut(c["ratings"], c["labels"], c["K"])
    assert not UC.no_tie_straddles_the_cut(c["new"], c["labels"], c["K"]) and len(picked("ties_at_the_cut")) > 0
    assert len(picked("full_row_loses_an_entry")) > 0
    c = cases["similarity_turns_zero_or_negative"]
    before, after = lists("similarity_turns_zero_or_negative", "ratings"), lists("similarity_turns_zero_or_negative", "new")
    assert before[2][0] > 0 and after[2][0] == 0 and before[2][4] > 0 and after[2][4] == 0
    cand = UC.milli_matrix(UC.centred(c["new"]))
    assert (cand[0, 1:3] < 0).all() and (cand[4] == 0).all()
    c = cases["row_unrated_to_zeros"]
    assert not c["new"][3].any() and c["ratings"][3].any()
    c = cases["R_is_a_whole_cluster"]
    assert set(c["R"]) == set(np.flatnonzero(c["labels"] == 0))
    c = cases["R_is_all_users"]
    assert len(c["R"]) == c["ratings"].shape[0]
    c = cases["two_clusters_at_once"]
    assert len(set(c["labels"][c["R"]])) >= 3
    c = cases["big_cluster"]
    assert c["ratings"].shape == (1500, 64) and len(set(c["labels"])) == 1 and len(c["R"]) > 64
    assert {cases["mixed_K%d" % k]["K"] for k in (1, 19, 64)} == {1, 19, 64}
    assert (lists("mixed_K64", "ratings")[2] == 64).any() and len(picked("mixed_K19")) > 0
    for name, c in cases.items():   # a batch's cells are distinct, and every batch changes something
        u, q, _ = c["edits"]
        assert len(set(zip(u.tolist(), q.tolist()))) == len(u) and not np.array_equal(c["new"], c["ratings"]), name


def _oracle_inputs():
    from qrlsh import users
    out = []
    for sub in ("cfg1", "cfg1b", "cfg2"):
        r = np.load(os.path.join(GOLDEN, sub + "_scores.npz"))["ratings"]
        out.append((sub, r, users.cluster_labels(r)))
    for seed, nu, nq in ((3, 60, 41), (5, 90, 23)):
        rng = np.random.default_rng(seed)
        r = (rng.integers(1, 101, size=(nu, nq)) * (rng.random((nu, nq)) < 0.6)).astype(np.int64)
        r[1] = 0
        out.append(("synthetic%d" % seed, r, rng.integers(0, 7, size=nu)))
    return out


def test_reference_lists_are_the_oracles_positive_entries():
    """cfg1 and cfg1b hold users (5 and 4 of 100) whose K-th and (K+1)-th candidates are equal at the oracle's K: there the
    oracle's np.argsort keeps an arbitrary one of the tied users.  Every other input is held to the precondition that no
    tie straddles the cut, and compared entry for entry; on those two, the users with such a tie are compared entry for
    entry above the tied value and by count and membership at it, all other users entry for entry."""
    tied_inputs = {}
    for name, r, labels in _oracle_inputs():
        nu = r.shape[0]
        K = round(np.log(nu) / np.log(1.5))
        cand = UC.ranked_candidates(r, labels)
        tied = {u for u, c in cand.items() if len(c) > K and c[K - 1][0] == c[K][0]}
        if name not in ("cfg1", "cfg1b"):
            assert UC.no_tie_straddles_the_cut(r, labels, K) and not tied, name
        tied_inputs[name] = len(tied)
        idx, mil, ln = UC.reference_lists(r, labels, K)
        ref = O.user_similarities_from_labels(r, labels)
        for u in range(nu):
            want = {(int(i), int(np.rint(v * 1000.0))) for i, v in zip(ref[u]["indexes"], ref[u]["values"]) if v > 0}
            got = {(int(idx[u, k]), int(mil[u, k])) for k in range(ln[u])}
            if u not in tied:
                assert want == got, (name, u)
                continue
            cut = cand[u][K - 1][0]
            assert {e for e in want if e[1] > cut} == {e for e in got if e[1] > cut}, (name, u)
            at_cut = {e for e in want if e[1] == cut}
            assert len(at_cut) == len({e for e in got if e[1] == cut}) and len(want) == len(got) == K, (name, u)
            assert at_cut <= {(i, m) for m, i in cand[u] if m == cut}, (name, u)
    assert tied_inputs == {"cfg1": 5, "cfg1b": 4, "cfg2": 0, "synthetic3": 0, "synthetic5": 0}
