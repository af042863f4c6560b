"""Dataset rows under a live index, the part that needs no device: the numpy restatements of tests/table_rows_cases.py
against the oracle (oracle.answer_sets + oracle.minhash over the edited table), and the host side of qrlsh.LiveTable -- the
dictionary that covers the values of the table and of the queries, and the live column."""
import numpy as np
import pytest

import table_rows_cases as TC


@pytest.fixture(scope="module")
def cases():
    return TC.host_cases()


def test_brute_answer_sets_and_minhash_equal_the_oracle(cases):
    for c in cases:
        live = np.zeros(c.D + c.m, dtype=bool)
        live[:c.D] = True
        for lv, want in ((live, c.sig), (None, c.sig_after)):
            sig, off, rows = TC.oracle_signatures(c.cells, c.qrows, c.perms, lv)
            boff, brows = TC.brute_answer_sets(c.cells, c.qrows, lv)
            assert np.array_equal(off, boff) and np.array_equal(rows, brows)
            assert np.array_equal(sig, want)


def test_restate_add_is_the_difference_of_two_oracle_runs(cases):
    for c in cases:
        cells, slots, tab_rows = c.batch()
        ids, rows = TC.restate_add(c.sig, c.qrows, cells, tab_rows)
        after, _, _ = TC.oracle_signatures(c.cells, c.qrows, c.perms)
        want = np.nonzero((after != c.sig).any(axis=1))[0]
        assert np.array_equal(ids, want) and np.array_equal(rows, after[want])
        assert np.all(np.diff(ids) > 0)
        # the specials: the empty set is filled, the all-unconstrained query is among the matched, the quiet one matches
        # and is not listed
        assert c.EMPTY in ids and (c.sig[c.EMPTY] == -1).all() and (after[c.EMPTY] >= 0).all()
        m = TC.matches(c.qrows, cells)
        assert m[c.ALL].all()
        if c.quiet:
            assert m[c.QUIET].any() and c.QUIET not in ids
        assert TC.matched_count(c.qrows, cells) >= len(ids)


@pytest.mark.parametrize("keep_slot0", [True, False])
def test_restate_remove_is_exactly_the_queries_whose_minimum_sat_there(cases, keep_slot0):
    for c in cases:
        gone = c.removal(keep_slot0)
        live = np.ones(c.D + c.m, dtype=bool)
        live[gone] = False
        ids = TC.restate_remove(c.sig_after, c.qrows, c.cells[gone], c.tab[gone])
        after, _, _ = TC.oracle_signatures(c.cells, c.qrows, c.perms, live)
        # the columns of the table hold distinct values: marked <=> the row really changes
        assert np.array_equal(ids, np.nonzero((after != c.sig_after).any(axis=1))[0])
        if c.quiet:
            assert TC.matches(c.qrows, c.cells[gone])[c.QUIET].any()
            assert (c.QUIET in ids) == (not keep_slot0)          # its minimum sits on slot 0, not on the hand-made row


def test_dictionary_covers_table_and_queries():
    from qrlsh.table import TableDictionary, with_live_column, LIVE_ROW
    d = TableDictionary(2)
    cells = d.encode_cells(np.array([["a", "x"], ["b", "x"], ["a", "y"]], dtype=object))
    assert cells.dtype == np.int32 and cells.shape == (3, 2)
    assert cells.min() >= 1 and LIVE_ROW == 0                    # row 0 is the live row
    assert cells[0, 0] == cells[2, 0] != cells[1, 0] and cells[0, 1] == cells[1, 1] != cells[2, 1]
    assert len(set(cells.reshape(-1).tolist())) == 4 == d.nrows - 1      # features do not share rows
    # a value named only by a query gets a row of its own -- not a shared zero row -- and an unconstrained cell is -1
    q = d.encode_queries(np.array([["a", ""], ["c", "y"], ["", "z"]], dtype=object))
    assert q[0].tolist() == [cells[0, 0], -1] and q[1, 1] == cells[2, 1] and q[2, 0] == -1
    assert q[1, 0] >= 5 and q[2, 1] >= 5 and q[1, 0] != q[2, 1] and d.nrows == 7
    # a later row with that value is matched: it takes the query's id
    later = d.encode_cells(np.array([["c", "z"]], dtype=object))
    assert later[0].tolist() == [q[1, 0], q[2, 1]] and d.nrows == 7
    # a value new to both gets the next row; numbers and strings compare as strings, as the dataset's cells do
    assert d.encode_cells(np.array([["d", 5]], dtype=object))[0].tolist() == [7, 8]
    assert d.encode_queries(np.array([["", "5"]], dtype=object))[0].tolist() == [-1, 8]
    # looking up without adding
    assert d.encode_queries(np.array([["nope", ""]], dtype=object), add=False)[0].tolist() == [-2, -1] and d.nrows == 9
    # the live column
    w = with_live_column(q)
    assert w.dtype == np.int32 and w.shape == (3, 3) and (w[:, 2] == LIVE_ROW).all() and np.array_equal(w[:, :2], q)
    for bad in (np.zeros((2, 3), dtype=object), np.zeros(4, dtype=object)):
        with pytest.raises(ValueError):
            d.encode_cells(bad)
        with pytest.raises(ValueError):
            d.encode_queries(bad)
    for nfeat in (0, 64):
        with pytest.raises(ValueError):
            TableDictionary(nfeat)
    TableDictionary(63)


def test_library_refuses_bad_table_row_arguments_without_a_gpu():
    import ctypes
    from qrlsh import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    ok = dict(n=10, nfeat=3, m=5, pd=_lib.PERM_U16, P=16, ps=16, sd=_lib.SIG_I32, mode=_lib.ROWS_ADD)

    def mark(**kw):
        a = dict(ok, **kw)
        return lib.qrlsh_table_rows_mark(one, a["n"], a["nfeat"], one, one, a["m"], one, a["pd"], a["P"], a["ps"], one, a["sd"],
                                         a["mode"], one, one, None)

    def fill(**kw):
        a = dict(ok, **kw)
        return lib.qrlsh_table_rows_fill(one, a["n"], a["nfeat"], one, one, a["m"], one, a["pd"], a["P"], a["ps"], one, a["sd"],
                                         one, a.get("c", 1), one, one, None)

    for f in (mark, fill):
        for bad in (dict(nfeat=0), dict(nfeat=64), dict(m=65537), dict(m=-1), dict(n=2**32 - 1), dict(P=0), dict(ps=15),
                    dict(pd=2), dict(sd=2), dict(pd=_lib.PERM_I32, sd=_lib.SIG_U16)):
            assert f(**bad) == _lib.QRLSH_EINVAL, (f.__name__, bad)
    assert mark(mode=2) == _lib.QRLSH_EINVAL and b"mode" in lib.qrlsh_last_error()
    assert fill(c=11) == _lib.QRLSH_EINVAL
    assert fill(c=0) == _lib.QRLSH_OK                           # nothing changed: nothing is launched
    for bad in (dict(wpr=0), dict(nfeat=64), dict(live=-1), dict(on=2)):
        a = dict(dict(wpr=4, m=3, nfeat=3, live=0, on=1), **bad)
        assert lib.qrlsh_bitmaps_set_rows(one, a["wpr"], one, one, a["m"], a["nfeat"], a["live"], a["on"], None) == _lib.QRLSH_EINVAL
    assert lib.qrlsh_bitmaps_set_rows(None, 4, None, None, 0, 3, 0, 1, None) == _lib.QRLSH_OK
