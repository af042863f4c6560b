"""The two claims qrlsh_index_remove / qrlsh_lists_remove_* rest on, in numpy (tests/index_remove_cases.py): the filtered
and renumbered layout IS the fresh layout of the survivors' keys, and the lists of a run over the survivors ARE the
stored lists with removed entries dropped, re-probing only full rows that lose an entry.  No GPU."""
import numpy as np
import pytest

import index_append_cases as AC
import index_remove_cases as RC
import lists_update_cases as LC


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def crowded():
    c = LC.CROWDED
    out = {}
    for hi in (3, 40):
        sig = LC.crowded(hi)
        out[hi] = (sig, AC.restate_layout(AC.np_band_keys(sig, c["b"])), LC.full_lists(sig, c["b"], c["K"]))
    return out


@pytest.mark.parametrize("hi", [3, 40])
def test_filtered_layout_is_the_fresh_layout_of_the_survivors(crowded, hi):
    c = LC.CROWDED
    sig, layout, _ = crowded[hi]
    keys = AC.np_band_keys(sig, c["b"])
    for name, given in RC.removal_sets(c["N"]).items():
        stay = RC.new_positions(c["N"], given) >= 0
        got = RC.restate_remove_layout(layout, given)
        assert _same(got, AC.restate_layout(np.ascontiguousarray(keys[:, stay]))), (hi, name)
    # "every even id" takes the directory from 6 to 5 bits
    assert AC.dir_bits(c["N"]) == 6 and AC.dir_bits(c["N"] // 2) == 5


@pytest.mark.parametrize("hi", [3, 40])
def test_lists_after_a_removal_come_from_the_stored_lists_and_the_full_rows(crowded, hi):
    c = LC.CROWDED
    sig, _, stored = crowded[hi]
    for name, given in RC.removal_sets(c["N"]).items():
        stay = RC.new_positions(c["N"], given) >= 0
        got, picked = RC.restate_remove_lists(stored, sig, given, c["b"], c["K"])
        assert LC.same(got, LC.full_lists(sig[stay], c["b"], c["K"])), (hi, name)
        if (hi, name) in RC.PICKED:
            assert len(picked) == RC.PICKED[(hi, name)], (hi, name, len(picked))
        if (hi, name) in RC.SHORT_LOST:
            assert RC.short_rows_that_lose(stored, c["N"], given, c["K"]) == RC.SHORT_LOST[(hi, name)], (hi, name)


def test_wide_bands_and_a_popular_key():
    w = LC.WIDE
    sig = LC.wide()
    given = np.random.default_rng(5).choice(w["N"], 60, replace=False)
    stay = RC.new_positions(w["N"], given) >= 0
    got, picked = RC.restate_remove_lists(LC.full_lists(sig, w["b"], w["K"]), sig, given, w["b"], w["K"])
    assert len(picked) > 0 and LC.same(got, LC.full_lists(sig[stay], w["b"], w["K"]))
    keys = AC.np_band_keys(sig, w["b"])
    assert _same(RC.restate_remove_layout(AC.restate_layout(keys), given),
                 AC.restate_layout(np.ascontiguousarray(keys[:, stay])))


def test_the_abi_names_the_remove_entry_points():
    import os
    import re
    from qrlsh import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "qrlsh.h")).read()
    for name in ("qrlsh_idmap_build", "qrlsh_idmap_list", "qrlsh_rows_remove", "qrlsh_index_remove",
                 "qrlsh_index_remove_workspace_bytes", "qrlsh_index_probe_finish_rows", "qrlsh_lists_remove_mark",
                 "qrlsh_lists_remove_count", "qrlsh_lists_remove_fill", "qrlsh_lists_remove_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, hdr)
    assert len(_lib.SIGNATURES["qrlsh_index_remove"][1]) == 15
