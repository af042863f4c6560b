"""The claims qrlsh_index_replace / qrlsh_lists_replace_* rest on, in numpy (tests/index_replace_cases.py): the band
without the replaced records, merged with the batch by (mix bits, id), IS the fresh layout of the new key matrix, and the
lists of a run over the new rows ARE the stored lists with the entries of replaced queries dropped, the replaced queries'
probes merged in with ties by id, and only full rows that lose an entry probed again.  No GPU."""
import numpy as np
import pytest

import index_append_cases as AC
import index_remove_cases as RC
import index_replace_cases as PC
import lists_update_cases as LC
import query_index_cases as QC


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
def test_lists_after_a_replacement_come_from_the_stored_lists_and_the_probed_rows(crowded, hi):
    c = LC.CROWDED
    sig, _, stored = crowded[hi]
    for name, case in PC.replacement_sets(c["N"]).items():
        rows_new = PC.new_rows(sig, case)
        got, picked = PC.restate_replace_lists(stored, sig, case[0], rows_new, c["b"], c["K"])
        assert LC.same(got, LC.full_lists(PC.overwritten(sig, case[0], rows_new), c["b"], c["K"])), (hi, name)
        counts = PC.branch_counts(stored, sig, case[0], rows_new, c["b"], c["K"])
        assert counts[0] == len(picked) == PC.PICKED[(hi, name)], (hi, name, counts)
        assert counts[1] == PC.SHORT_LOST.get((hi, name), 0) and counts[2] == PC.TIE_GAINED.get((hi, name), 0), (hi, name, counts)
        if case[1] == "self":
            assert LC.same(got, stored), (hi, name)
    # every branch is taken somewhere
    assert all(any(v > 0 for v in d.values()) for d in (PC.PICKED, PC.SHORT_LOST, PC.TIE_GAINED))


@pytest.mark.parametrize("hi", [3, 40])
def test_merged_layout_is_the_fresh_layout_of_the_new_keys(crowded, hi):
    c = LC.CROWDED
    sig, layout, _ = crowded[hi]
    for name, case in PC.replacement_sets(c["N"]).items():
        rows_new = PC.new_rows(sig, case)
        got = PC.restate_replace_layout(layout, case[0], AC.np_band_keys(rows_new, c["b"]))
        assert _same(got, AC.restate_layout(AC.np_band_keys(PC.overwritten(sig, case[0], rows_new), c["b"]))), (hi, name)
        if case[1] == "self":
            assert _same(got, layout)
        if case[1] == "copy" and hi == 3:       # new records sit inside runs of equal keys, ids on both sides of them
            top = AC.np_band_keys(PC.overwritten(sig, case[0], rows_new), c["b"])[0]
            inside = [(top[:r] == top[r]).any() and (top[r + 1:] == top[r]).any() for r in case[0].tolist()]
            assert sum(inside) >= 20, (hi, sum(inside))


def test_hashed_wide_bands():
    w = LC.WIDE
    sig = LC.wide()
    rng = np.random.default_rng(6)
    ids = rng.choice(w["N"], 60, replace=False)
    rows_new = np.concatenate((rng.integers(0, 2, size=(40, w["P"])).astype(np.int32), sig[rng.choice(w["N"], 20)]))
    rows = PC.overwritten(sig, ids, rows_new)
    got, picked = PC.restate_replace_lists(LC.full_lists(sig, w["b"], w["K"]), sig, ids, rows_new, w["b"], w["K"])
    assert len(picked) > 0 and LC.same(got, LC.full_lists(rows, w["b"], w["K"]))
    assert _same(PC.restate_replace_layout(AC.restate_layout(AC.np_band_keys(sig, w["b"])), ids, AC.np_band_keys(rows_new, w["b"])),
                 AC.restate_layout(AC.np_band_keys(rows, w["b"])))


def test_golden_signature_sets():
    for name, g, sig, b, K in QC.golden_sets():
        n = sig.shape[0]
        rng = np.random.default_rng(n)
        m = min(12, n)
        ids = rng.choice(n, m, replace=False)
        rows_new = sig[rng.choice(n, m)].copy()                  # rows of the set's own kind, at other ids
        rows_new[0] = np.roll(rows_new[0], 1)
        rows = PC.overwritten(sig, ids, rows_new)
        got, _ = PC.restate_replace_lists(LC.full_lists(sig, b, K), sig, ids, rows_new, b, K)
        assert LC.same(got, LC.full_lists(rows, b, K)), name
        assert _same(PC.restate_replace_layout(AC.restate_layout(AC.np_band_keys(sig, b)), ids, AC.np_band_keys(rows_new, b)),
                     AC.restate_layout(AC.np_band_keys(rows, b))), name


@pytest.mark.parametrize("hi", [3, 40])
def test_equals_remove_then_append_with_the_ids_mapped_back(crowded, hi):
    c = LC.CROWDED
    N, b, K = c["N"], c["b"], c["K"]
    sig, _, stored = crowded[hi]
    for name in ("random40", "copy", "first"):
        case = PC.replacement_sets(N)[name]
        ids = np.sort(case[0])
        rows_new = PC.new_rows(sig, case)[np.argsort(case[0], kind="stable")]
        want, _ = PC.restate_replace_lists(stored, sig, ids, rows_new, b, K)
        pos = RC.new_positions(N, ids)
        shrunk, _ = RC.restate_remove_lists(stored, sig, ids, b, K)
        left = N - len(ids)
        grown = LC.restate_update(shrunk, np.concatenate((sig[pos >= 0], rows_new)), left, len(ids), b, K)
        back = np.concatenate((np.nonzero(pos >= 0)[0], ids))    # id after remove + append -> position it stands for
        got = LC.cut(back[grown[0]], back[grown[1]], grown[2], K)
        # the chain cuts every row while the replaced queries carry the largest ids and lose ties there, so a row may
        # end on another member of the tie at its cut: the values agree everywhere, the neighbours above the cut value
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (hi, name)
        last = np.zeros(N, dtype=np.int64)
        last[want[0]] = want[2]                                   # a row's last, smallest value
        above = want[2] > last[want[0]]
        assert np.array_equal(got[1][above], want[1][above]), (hi, name)
        differ = int((got[1] != want[1]).sum())
        assert differ > 0 if (hi, name) == (3, "random40") else True      # the difference is real: ties go by id


@pytest.mark.parametrize("hi", [3, 40])
def test_any_split_of_a_batch_gives_the_same_result(crowded, hi):
    c = LC.CROWDED
    N, b, K = c["N"], c["b"], c["K"]
    sig, layout, stored = crowded[hi]
    for name in ("random40", "copy"):
        case = PC.replacement_sets(N)[name]
        ids, rows_new = case[0], PC.new_rows(sig, case)
        one, _ = PC.restate_replace_lists(stored, sig, ids, rows_new, b, K)
        one_layout = PC.restate_replace_layout(layout, ids, AC.np_band_keys(rows_new, b))
        for bounds in ((1, len(ids)), (7, 8, 20, len(ids))):
            lists, rows, lay, lo = stored, sig, layout, 0
            for hi_ in bounds:
                part, part_rows = ids[lo:hi_], rows_new[lo:hi_]
                lists, _ = PC.restate_replace_lists(lists, rows, part, part_rows, b, K)
                lay = PC.restate_replace_layout(lay, part, AC.np_band_keys(part_rows, b))
                rows, lo = PC.overwritten(rows, part, part_rows), hi_
            assert LC.same(lists, one) and _same(lay, one_layout), (hi, name, bounds)


def test_the_abi_names_the_replace_entry_points():
    import os
    import re
    from qrlsh import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "qrlsh.h")).read()
    for name in ("qrlsh_rows_replace", "qrlsh_index_replace", "qrlsh_index_replace_workspace_bytes",
                 "qrlsh_lists_replace_count", "qrlsh_lists_replace_fill", "qrlsh_lists_replace_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, hdr)
    assert len(_lib.SIGNATURES["qrlsh_index_replace"][1]) == 18
    from qrlsh.index import QueryIndex
    assert callable(QueryIndex.replace) and callable(QueryIndex.set)
