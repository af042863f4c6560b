"""qrlsh._inputs: the one copy of the wrappers' argument checks, request blocks and flag reading, and the import order
of the package.  No device, no library."""
import ast
import glob
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from qrlsh import _inputs as I

PKG = os.path.dirname(os.path.abspath(I.__file__))
MODULES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(PKG, "*.py")) if not p.endswith("__init__.py"))


# ------------------------------------------------------------------------------------------------ request blocks
def _plan(m, need, budget, **kw):
    blk, _ = I.request_blocks(m, need, budget, **kw)
    return blk, [(i0, i1) for _, i0, i1 in I.blocks(m, blk)]


def test_blocks_of_nothing_and_of_one():
    assert _plan(0, lambda b: 1 << 40, 100) == (1, [])
    assert _plan(0, lambda b: 1 << 40, 100, group=4) == (4, [])
    assert _plan(1, lambda b: 1 << 40, 100) == (1, [(0, 1)])


def test_a_need_equal_to_the_budget_is_not_split_and_one_byte_more_is():
    assert _plan(8, lambda b: b * 16, 128) == (8, [(0, 8)])
    assert _plan(8, lambda b: b * 16 + 1, 128) == (4, [(0, 4), (4, 8)])


def test_a_need_that_never_fits_ends_at_one_request_or_one_group():
    asked = []

    def need(b):
        asked.append(b)
        return 1 << 40
    assert _plan(5, need, 100) == (1, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])
    assert asked == [5, 3, 2]                      # (blk + 1) // 2 each time; one request is not asked about
    assert _plan(10, lambda b: 1 << 40, 100, group=4) == (4, [(0, 4), (4, 8), (8, 10)])


def test_blocks_are_whole_groups_with_a_short_last_one():
    # 10 -> 5 fits; 5 rounds up to two groups of 4
    assert _plan(10, lambda b: b * 10, 50, group=4) == (8, [(0, 8), (8, 10)])


def test_a_cap_below_m():
    assert _plan(10, lambda b: 0, 100, cap=4) == (4, [(0, 4), (4, 8), (8, 10)])
    assert _plan(10, lambda b: 0, 100, group=4, cap=6) == (8, [(0, 8), (8, 10)])


def test_37_requests_under_a_budget_that_admits_10():
    asked = []

    def need(b):
        asked.append(b)
        return b
    assert _plan(37, need, 10) == (10, [(0, 10), (10, 20), (20, 30), (30, 37)])
    assert asked == [37, 19, 10]
    assert [b for b, _, _ in I.blocks(37, 10)] == [0, 1, 2, 3]


def test_the_unnamed_full_set_gets_its_ids_once_it_is_split():
    blk, ids = I.request_blocks(6, lambda b: b, 6, None, 6, "cpu")
    assert blk == 6 and ids is None
    blk, ids = I.request_blocks(6, lambda b: b, 3, None, 6, "cpu")
    assert blk == 3 and ids.dtype == torch.int32 and ids.tolist() == [0, 1, 2, 3, 4, 5]
    given = torch.tensor([4, 4, 1, 0, 2, 2], dtype=torch.int32)
    assert I.request_blocks(6, lambda b: b, 3, given, 6, "cpu")[1] is given
    assert I.request_blocks(6, lambda b: b, 3)[1] is None          # a caller whose requests carry no ids


# ------------------------------------------------------------------------------------------------------ the ids
def test_host_ids_outside_the_bound_raise_before_any_upload(monkeypatch):
    def no_device(*a, **kw):
        raise AssertionError("touched the device")
    monkeypatch.setattr(I, "ids32", no_device)
    monkeypatch.setattr(I, "on_device", no_device)
    for bad in ([-1], [7], [0, 3, 7], np.array([2**40])):
        with pytest.raises(ValueError, match=r"user id outside \[0, 7\)"):
            I.select_ids(bad, 7, "user", "users")
    r = np.zeros((7, 3), dtype=np.int32)
    e = np.zeros(0, dtype=np.int64)
    with pytest.raises(ValueError, match=r"user id outside \[0, 7\)"):
        I.ServeInputs(r, e, e, e, {}, [7], "pairwise")
    with pytest.raises(ValueError, match=r"query id outside \[0, 3\)"):
        I.ServeInputs(r, e, e, e, {}, [-1], "pairwise", ids="queries")


def test_id_selections():
    assert I.select_ids(None, 7, "user", "users") == (7, None, False)
    m, ids, vouch = I.select_ids([], 7, "user", "users")
    assert (m, ids.dtype, ids.tolist(), vouch) == (0, np.int64, [], False)
    m, ids, vouch = I.select_ids([6, 0, 6], 7, "user", "users")
    assert (m, ids.dtype, ids.tolist(), vouch) == (3, np.int64, [6, 0, 6], False)
    t = torch.tensor([9, -4])                                           # a tensor: the library's flag vouches
    m, ids, vouch = I.select_ids(t, 7, "user", "users")
    assert m == 2 and ids is t and vouch is True
    with pytest.raises(ValueError, match=r"query id outside \[0, 7\)"):    # unless CPU tensors count as host data
        I.select_ids(t, 7, "query", "queries", host_tensors=True)
    for bad in ([0.5], [[0, 1]], [True], torch.tensor([0.5]), torch.tensor([[0, 1]]), torch.tensor([True])):
        with pytest.raises(ValueError, match="users must be a 1-D"):
            I.select_ids(bad, 7, "user", "users")


def test_ids_past_int32_stay_out_of_range():
    bound = 1000
    t = torch.tensor([2**31, 2**32 + 3, -2**40, 0, bound - 1, -1, bound], dtype=torch.int64)
    got = I.ids32(t, bound, "cpu")
    assert got.dtype == torch.int32 and got.is_contiguous()
    assert got.tolist() == [bound, bound, -1, 0, bound - 1, -1, bound]
    assert I.ids32(np.array([2**32 + 3, 5], dtype=np.int64), bound, "cpu").tolist() == [bound, 5]


def test_integer_arrays():
    assert I.int_array([], 1, "x").dtype == torch.int64 and I.int_array([], 1, "x").shape == (0,)
    assert I.int_array([[1, 2]], 2, "x").shape == (1, 2)
    assert I.int_array(np.zeros((2, 3, 4), dtype=np.int16), None, "x").shape == (2, 3, 4)
    for bad, ndim in (([0.5], 1), ([[0, 1]], 1), ([True], 1), ([1, 2], 2), (torch.tensor([1.0]), 1), ([0.5], None)):
        with pytest.raises(ValueError, match="x must be an? .*integer array"):
            I.int_array(bad, ndim, "x")
    assert [t.tolist() for t in I.coo_triple([0, 0], (1, 2), np.array([900, 800]))] == [[0, 0], [1, 2], [900, 800]]
    with pytest.raises(ValueError, match="differ in length"):
        I.coo_triple([0, 0], [1, 2], [900])
    with pytest.raises(ValueError, match="q_dst must be a 1-D integer array"):
        I.coo_triple([0], [0.5], [900])


def test_sum_order_and_matrix_shape():
    from qrlsh import _lib
    assert I.sum_order_code("pairwise") == _lib.SUM_PAIRWISE and I.sum_order_code("sequential") == _lib.SUM_SEQUENTIAL
    for bad in ("numpy", None, 0):
        with pytest.raises(ValueError, match="sum_order must be 'pairwise' or 'sequential'"):
            I.sum_order_code(bad)
    t = np.zeros((4, 5), dtype=np.int64)
    assert I.like_matrix(t, "truth", (4, 5), "ratings") is not None
    with pytest.raises(ValueError, match=r"truth has shape \(4, 5\), ratings \(5, 4\)"):
        I.like_matrix(t, "truth", (5, 4), "ratings")
    with pytest.raises(ValueError, match="truth must hold integers"):
        I.like_matrix(t.astype(np.float32), "truth", (4, 5), "ratings")


# -------------------------------------------------------------------------------------------------------- flags
def test_flag_words_are_ored():
    assert I.or_flags([0, 2, 0, 4]) == 6
    assert I.or_flags(np.array([0, 2, 0, 4], dtype=np.int64)) == 6
    assert I.or_flags(torch.tensor([0, 2, 0, 4], dtype=torch.int32)) == 6
    assert I.or_flags([]) == 0
    words = torch.tensor([[0], [2], [0], [6]], dtype=torch.int64)       # the form that stays on the device
    got = I.or_flags(words, device_bits=3)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.tolist() == [6]


def test_the_first_entry_of_the_table_whose_bit_is_set_is_raised():
    table = ((1, "one of %(n)d"), (2, "two of %(n)d"), (4, "four"))
    I.raise_flags(0, table, n=3)                                        # a zero word raises nothing
    I.raise_flags(8, table, n=3)                                        # nor does a bit the table does not name
    with pytest.raises(ValueError, match="^two of 3$"):
        I.raise_flags(6, table, n=3)
    with pytest.raises(ValueError, match="^four$"):
        I.raise_flags(6, ((4, "four"), (2, "two of %(n)d")), n=3)       # the table's order, not the bit's


def test_every_table_raises_its_lowest_bit_first():
    tables = [importlib.import_module("qrlsh." + name)._FLAG_TEXT for name in ("diversify", "fidelity", "exactlists")]
    for table in [I.LIST_FLAGS] + tables:
        bits = [bit for bit, _ in table]
        assert bits == sorted(bits) and all(b & (b - 1) == 0 for b in bits)
    r = np.zeros((3, 2), dtype=np.int32)
    e = np.zeros(0, dtype=np.int64)
    a = I.ServeInputs(r, e, e, e, {}, None, "pairwise")
    a.raise_flags(np.array([0, 0], dtype=np.int64))
    with pytest.raises(ValueError, match="more than 64 neighbours"):
        a.raise_flags(torch.tensor([2, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"neighbour index is outside \[0, 2\)"):
        a.raise_flags([2, 4])


# ------------------------------------------------------------------------------------------------- import order
def test_no_import_of_the_package_inside_a_function():
    found = []
    for name in MODULES + ["__init__"]:
        path = os.path.join(PKG, name + ".py")
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                found += ["%s.py:%d" % (name, n.lineno) for n in ast.walk(fn)
                          if isinstance(n, ast.ImportFrom) and n.level > 0]
    assert not found, "intra-package imports inside a function body: %s" % found


def test_every_submodule_imports_on_its_own():
    """each in a fresh interpreter in which the package is an empty shell, so that nothing but the module's own imports
    has run before it: a cycle, or an import that leans on qrlsh/__init__'s order, fails here"""
    code = ("import importlib, sys, types\n"
            "pkg = types.ModuleType('qrlsh'); pkg.__path__ = [%r]; sys.modules['qrlsh'] = pkg\n"
            "importlib.import_module('qrlsh.' + sys.argv[1])\n" % PKG)
    failed = {}
    for first in range(0, len(MODULES), 8):                # eight interpreters at a time: each imports torch
        procs = [(name, subprocess.Popen([sys.executable, "-c", code, name], stdout=subprocess.PIPE,
                                         stderr=subprocess.STDOUT, text=True)) for name in MODULES[first:first + 8]]
        for name, p in procs:
            out = p.communicate()[0]
            if p.returncode:
                failed[name] = out
    assert not failed, failed
