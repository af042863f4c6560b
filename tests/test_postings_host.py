"""The postings and the exact lists served from them (qrlsh.answer_postings, exact_neighbours(postings=...),
Recommender.answer_postings): what needs no device.  The numpy transpose the GPU tests compare bytes with is held to a
dict-of-lists restatement, the vectorised list reference to exactlists_cases.exact_ref, the cases to what makes them worth
running; then Python's argument checks, the size exports and the C surface; last the window rule of csrc/postingsplan.h,
run on the CPU by its own program under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import exactlists_cases as XC
import postings_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "query-recommendation-system_amd", "csrc")


# ---- the restatements ---------------------------------------------------------------------------------------------------
def test_numpy_transpose_against_dict_of_lists():
    for case in (XC.sizes_case(), XC.planted_case(31), XC.planted_case(33), PC.every_query_case(), PC.empty_rows_case(),
                 XC.Case([{0}, set(), {0}], 1, "D=1"), XC.Case([set(), set()], 7, "nnz=0"), XC.Case([], 7, "nq=0")):
        p_off, p_qry = PC.postings_ref(case.offsets, case.rows, case.D)
        assert p_off.dtype == np.int64 and p_qry.dtype == np.int32 and p_off.shape == (case.D + 1,), case.name
        assert p_off[0] == 0 and p_off[-1] == len(case.rows) == len(p_qry) and (np.diff(p_off) >= 0).all(), case.name
        held = PC.postings_lists(case.offsets, case.rows, case.D)
        for d in (range(case.D) if case.D <= 4096 else sorted(set(case.rows.tolist()) | {0, case.D - 1, case.D // 2 - 1})):
            assert p_qry[p_off[d]:p_off[d + 1]].tolist() == held[d], (case.name, d)
            assert held[d] == sorted(held[d])                        # ascending: the CSR holds a row once per query
        assert sum(len(v) for v in held.values()) == len(p_qry)


def test_fast_reference_against_the_set_restatement():
    for case, K, chosen in ((XC.sizes_case(), 5, None), (XC.sizes_case(), 64, None), (XC.planted_case(200), 3, None),
                            (XC.tie_case(), 10, [0, 3, 50]), (XC.positives_case(2), 2, range(4)),
                            (XC.positives_case(64), 64, range(4)), (PC.every_query_case(), 7, [0, 1, 6, 299]),
                            (XC.planted_case(33), 4, [5, 0, 0, 7, 8])):
        XC.same_lists(PC.fast_ref(case.offsets, case.rows, case.D, K, chosen), case.ref(K, chosen), case.name)
    small = PC.single_row_case(40, C=41)
    XC.same_lists(small.ref(6, small.requests), XC.exact_ref(small.offsets, small.rows, 6, small.requests))


def test_case_builders_assert_their_point():
    C = PC.PASS_ENTRIES
    for others in (C - 2, C - 1, C, C + 1):
        case = PC.single_row_case(others)
        assert case.list_length(0) - 1 == others
    PC.narrow_case(), PC.unpruned_case(), PC.survivors_case(), PC.long_request_case()
    PC.every_query_case(), PC.empty_rows_case()


SMALL = dict(D=40, nq=256, base=100, span=16, per=20)     # long_windows_case under C = 64 and 32 cursors


def _small_cases():
    """the new shapes shrunk (a small C passed in), each with a K that cuts its lists and one that does not"""
    return ((PC.long_windows_case(C=64, cursors=32, **SMALL), 5), (PC.hot_id_case(C=64), 3),
            (PC.probe_chain_case(nq=1 << 15), 64), (PC.late_windows_case(C=128), 8),
            (PC.lanes_case(nq=400, sizes=(1, 2, 3, 5, 8, 9, 16, 17), shared=60, threads=64, cursors=32), 7),
            (PC.mixed_case(C=64, cursors=32, **SMALL), 4))


def test_new_case_builders_assert_their_point():
    """every new builder at the size the GPU tests run: the path assertions through plan_ref / slot_ref hold for the C,
    the queue and the cursor count the library exports"""
    from qrlsh import _lib
    lib = _lib.load()
    assert lib.qrlsh_exact_postings_pass_entries() == PC.PASS_ENTRIES == PC.TABLE_SLOTS // 2
    assert lib.qrlsh_exact_postings_queue() == PC.QUEUE and lib.qrlsh_exact_postings_list_cursors() == PC.LIST_CURSORS
    assert lib.qrlsh_exact_postings_threads() == PC.THREADS
    long = PC.long_windows_case()
    assert long.nq == 4096 and long.D == 600 and 19_000 < len(long.rows) < 21_000
    hot = PC.hot_id_case()
    assert hot.D == PC.PASS_ENTRIES + 8 and hot.requests == [0, 19, 30, 5]
    chain = PC.probe_chain_case()
    assert chain.nq == 1 << 17
    slots = np.array([PC.slot_ref(j) for j in range(chain.nq)])
    assert int((slots >= PC.TABLE_SLOTS - 32).sum()) == 255 and slots.max() == PC.TABLE_SLOTS - 1 and slots.min() == 0
    lanes = PC.lanes_case()
    assert sorted({PC.lanes_ref(a) for a in PC.LANE_SIZES + (513,)}) == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert len(lanes.requests) == len(PC.LANE_SIZES) + 1
    PC.late_windows_case(), PC.mixed_case()
    grid = PC.random_cases(0)
    assert [(c.nq, c.D) for c in grid] == [(nq, D) for nq in (257, 5000) for D in (8, 64, 700)]
    assert all(len(c.requests) == 16 for c in grid) and PC.RANDOM_KS == (1, 7, 63, 64)
    for case in (long, hot, chain, lanes, grid[-1]):
        assert len(case.rows) <= 250_000, case.name


def test_plan_restatement_against_brute_force_counts():
    """plan_ref's windows tile [0, nq) in order, each count is the number of list entries with an id inside it (counted
    entry by entry from the dict-of-lists postings), a pass holds at most C entries or one id, and a window was halved
    only because it was no pass: the window before its last halving holds more than C"""
    for case, C in ((PC.long_windows_case(C=64, cursors=32, **SMALL), 64), (PC.hot_id_case(C=16), 16),
                    (PC.late_windows_case(C=128), 128)):
        held = PC.postings_lists(case.offsets, case.rows, case.D)
        halved = single = 0
        for s in case.requests:
            mine = case.rows[case.offsets[s]:case.offsets[s + 1]].tolist()
            entries = [j for d in mine for j in held[d]]

            def count(lo, hi):
                return sum(1 for j in entries if lo <= j < hi)
            plan = PC.plan_ref(case, s, C)
            if not entries:
                assert plan == []
                continue
            windows = -(-len(entries) // C)
            width = case.nq if windows == 1 else -(-case.nq // windows)
            assert [p[0] for p in plan] == [0] + [p[1] for p in plan[:-1]] and plan[-1][1] == case.nq
            assert sum(p[2] for p in plan) == len(entries)
            for lo, hi, n, h in plan:
                assert n == count(lo, hi) and (n <= C or hi - lo == 1) and hi > lo
                top = min(lo + width, case.nq)
                for _ in range(h):
                    before, top = top, lo + (top - lo) // 2
                assert top == hi
                if h:
                    assert count(lo, before) > C and before - lo >= 2
                halved += h
                single += n > C
        assert halved > 0, case.name
        assert single > 0 or "hot" not in case.name


def test_fast_reference_on_the_new_shapes_shrunk():
    for case, K in _small_cases():
        for k in sorted({1, K}):
            XC.same_lists(case.ref(k, case.requests), XC.exact_ref(case.offsets, case.rows, k, case.requests),
                          "%s K=%d" % (case.name, k))
    for case in PC.random_cases(1, grid=((257, 8), (257, 64), (257, 700))):
        for K in (1, 63):
            XC.same_lists(case.ref(K, case.requests), XC.exact_ref(case.offsets, case.rows, K, case.requests), case.name)


# ---- Python's checks come before the library is loaded -----------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from qrlsh import _lib

    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _postings(nq=2, nnz=2, D=4):
    import qrlsh
    return qrlsh.AnswerPostings(torch.zeros(D + 1, dtype=torch.int64), torch.zeros(nnz, dtype=torch.int32), D, nq, nnz)


def test_argument_checks_precede_the_library(no_library):
    import qrlsh
    ok = dict(offsets=np.array([0, 1, 2]), rows=np.array([0, 1]), D=4)
    for bad in (dict(D=-1), dict(D=(1 << 20) + 1), dict(D=True), dict(D=4.0), dict(offsets=[]), dict(offsets=[[0, 1, 2]]),
                dict(rows=[0.5, 1.0])):
        with pytest.raises(ValueError):
            qrlsh.answer_postings(**dict(ok, **bad))
    ok["K"] = 3
    assert repr(_postings()) == "AnswerPostings(D=4, nq=2, nnz=2)"
    for stale, text in ((_postings(nq=3), "built from"), (_postings(nnz=3), "built from"), (_postings(D=5), "built from"),
                        ((1, 2), "must be an AnswerPostings"), (True, "must be an AnswerPostings")):
        with pytest.raises(ValueError, match=text):
            qrlsh.exact_neighbours(postings=stale, **ok)
    with pytest.raises(ValueError, match="slices"):
        qrlsh.exact_neighbours(postings=_postings(), slices=2, **ok)
    short = _postings()
    short.p_qry = short.p_qry[:1]
    with pytest.raises(ValueError, match="shape"):
        qrlsh.exact_neighbours(postings=short, **ok)
    for bad in (dict(K=0), dict(K=65), dict(queries=[2]), dict(queries=[-1])):      # the other checks stay in front
        with pytest.raises(ValueError):
            qrlsh.exact_neighbours(postings=_postings(), **dict(ok, **bad))


def test_recommender_checks_need_no_device(no_library):
    import recommender as R
    rec = R.Recommender()
    with pytest.raises(ValueError, match="1..64"):
        rec.exact_query_lists(K=65, postings=True)
    with pytest.raises(ValueError, match="no live lists"):
        rec.exact_query_lists(postings=True)
    assert "postings" in R.Recommender.exact_query_lists.__doc__ and callable(R.Recommender.answer_postings)


# ---- the size exports and the C surface --------------------------------------------------------------------------------
def test_scratch_sizes_on_both_sides_of_their_constants():
    from qrlsh import _lib
    lib = _lib.load()
    size, sort = lib.qrlsh_answer_postings_scratch_bytes, lib.qrlsh_sort_workspace_bytes

    def al16(n):
        return (n + 15) // 16 * 16
    # two arrays of nnz 64-bit words, each rounded to 16 bytes, and the sort's own workspace behind them; D does not enter
    for nnz in (1, 2, 3, 5, 2047, 2048, 2049, 4095, 4096, 4097, 16384, 16385, 32768, 32769, 220_000_000, (1 << 32) - 1):
        want = 2 * al16(8 * nnz) + al16(sort(nnz, 1))
        for D in (0, 1, 1 << 20):
            assert size(nnz, D) == want, (nnz, D)
    assert size(1, 0) == 16 + 16 + al16(sort(1, 1))
    assert all(size(0, D) == 0 for D in (0, 1, 5, 1 << 20))                       # nothing to sort
    for bad in ((-1, 5), (1 << 32, 5), (5, -1), (5, (1 << 20) + 1)):
        assert size(*bad) == 0, bad
    assert lib.qrlsh_exact_postings_pass_entries() == PC.PASS_ENTRIES
    assert lib.qrlsh_exact_postings_queue() == PC.QUEUE and lib.qrlsh_exact_postings_list_cursors() == PC.LIST_CURSORS
    assert lib.qrlsh_exact_postings_threads() == PC.THREADS
    for args in ((0, 0, 1), (1, 1, 1), (10_000_000, 1 << 24, 64), (-1, -1, 0), (5, 5, 65)):
        assert lib.qrlsh_exact_postings_scratch_bytes(*args) == 0, args            # everything stays in LDS


def test_c_surface():
    from qrlsh import _lib
    import qrlsh
    hdr = open(os.path.join(ROOT, "include", "qrlsh.h")).read()
    for name, nargs in (("qrlsh_answer_postings", 11), ("qrlsh_answer_postings_scratch_bytes", 2),
                        ("qrlsh_exact_neighbours_postings", 17), ("qrlsh_exact_postings_scratch_bytes", 3)):
        decl = re.search(r"^(?:int|size_t|int32_t) %s\(([^;]*)\);" % name, hdr, re.M)
        assert decl and name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"^int32_t qrlsh_exact_postings_pass_entries\(void\);", hdr, re.M)
    assert _lib.SIGNATURES["qrlsh_exact_postings_pass_entries"][1] == []
    for name in ("qrlsh_exact_postings_list_cursors", "qrlsh_exact_postings_queue", "qrlsh_exact_postings_threads"):
        assert re.search(r"^int32_t %s\(void\);" % name, hdr, re.M) and _lib.SIGNATURES[name][1] == [], name
    assert {"answer_postings", "AnswerPostings", "exact_neighbours"} <= set(qrlsh.__all__)
    # no export of the new file matches the pattern of the recorded workspace sizes
    import importlib.util
    spec = importlib.util.spec_from_file_location("workspace_sizes", os.path.join(ROOT, "tools", "workspace_sizes.py"))
    ws = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ws)
    assert not [n for n in _lib.SIGNATURES if "postings" in n and ws.SIZE_EXPORT.match(n)]
    lib = _lib.load()
    flag = np.zeros(1, dtype=np.uint32).ctypes.data
    some = np.zeros(4, dtype=np.int64).ctypes.data     # a host address: every call below returns before any device work

    def build(nq=5, nnz=0, D=10, flag=flag, off=some, p_off=some, rows=None, p_qry=None, scratch=None, nbytes=0):
        return lib.qrlsh_answer_postings(off, rows, nq, nnz, D, p_off, p_qry, flag, scratch, nbytes, None)
    for bad in (dict(nq=-1), dict(nq=1 << 31), dict(nnz=-1), dict(D=-1), dict(D=(1 << 20) + 1), dict(flag=None),
                dict(off=None), dict(p_off=None), dict(nnz=3), dict(nnz=3, rows=some, p_qry=some, nq=0)):
        assert build(**bad) == _lib.QRLSH_EINVAL, bad
    assert build(nnz=1 << 32, rows=some, p_qry=some) == _lib.QRLSH_EUNSUPPORTED
    need = lib.qrlsh_answer_postings_scratch_bytes(3, 10)
    assert build(nnz=3, rows=some, p_qry=some, scratch=some, nbytes=need - 1) == _lib.QRLSH_EWORKSPACE
    assert build(nnz=3, rows=some, p_qry=some) == _lib.QRLSH_EWORKSPACE              # a null scratch holds nothing

    def serve(nq=5, D=10, m=0, K=3, flag=flag):
        return lib.qrlsh_exact_neighbours_postings(None, None, nq, D, None, None, None, m, K, None, None, None, None, flag,
                                                   None, 0, None)
    assert serve() == _lib.QRLSH_OK and serve(nq=0) == _lib.QRLSH_OK
    for bad in (dict(K=0), dict(K=65), dict(nq=-1), dict(nq=1 << 31), dict(D=-1), dict(D=(1 << 20) + 1), dict(m=-1),
                dict(m=6), dict(flag=None)):
        assert serve(**bad) == _lib.QRLSH_EINVAL, bad
    assert serve(m=(1 << 24) + 1, nq=1 << 30) == _lib.QRLSH_EUNSUPPORTED
    assert serve(m=1) == _lib.QRLSH_EINVAL              # null pointers, still before any device work


# ---- csrc/postingsplan.h on the CPU ------------------------------------------------------------------------------------
def test_window_rule_under_the_host_sanitizers(tmp_path):
    """The even cut, the halving, the pass rule and the lower bound the request kernel uses, in a program of their own
    built with -fsanitize=address,undefined (csrc/Makefile's postingsplan_host): exactly sized lists, one list on both
    sides of C, more lists than C on one id, a narrow range in a wide id space, random shapes -- the windows must tile
    [0, nq), hold at most C entries or one id, and find every multiplicity."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "postingsplan_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "postingsplan_host.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "postingsplan ok" in done.stdout, (done.returncode, done.stdout, done.stderr[-2000:])
    text = open(os.path.join(CSRC, "postingsplan.h")).read()
    assert re.search(r"PP_TABLE_SLOTS = (\d+);", text).group(1) == str(2 * PC.PASS_ENTRIES)
