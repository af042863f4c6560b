"""The claim qrlsh_index_append rests on, in numpy on the golden signature sets: the layout of a fresh build over
all n + m rows IS the stable merge (old records first among equal mix bits) of the old layout and the batch's layout
with its ids offset by n (tests/index_append_cases.py).  No GPU."""
import os
import re

import numpy as np

import index_append_cases as AC
import query_index_cases as QC
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def test_band_keys_restatement_equals_the_oracle():
    seen = 0
    for name, g, sig, b, K in QC.golden_sets():
        if sig.shape[1] // b > 4:
            continue
        assert np.array_equal(AC.np_band_keys(sig, b), O.band_keys(sig, b).T), name
        seen += 1
    assert seen >= 10


def test_dir_bits_rule():
    assert [AC.dir_bits(n) for n in (0, 1, 16, 17, 1024, 1025, 10_000_000, 1 << 40)] == [1, 1, 1, 2, 7, 8, 21, 26]


def test_fresh_layout_is_the_stable_merge_on_the_golden_sets():
    seen = 0
    for name, g, sig, b, K in QC.golden_sets():
        keys = AC.np_band_keys(sig, b)
        n = keys.shape[1]
        whole = AC.restate_layout(keys)
        for cut in sorted({0, 1, n // 2, n - 1, n}):
            old, batch = AC.restate_layout(keys[:, :cut].copy()), AC.restate_layout(keys[:, cut:].copy())
            assert _same(AC.restate_merge(old, batch), whole), (name, cut)
        # in three steps, the directory width changing on the way
        a, c = n // 3, 2 * n // 3
        lay = AC.restate_layout(keys[:, :a].copy())
        lay = AC.restate_merge(lay, AC.restate_layout(keys[:, a:c].copy()))
        lay = AC.restate_merge(lay, AC.restate_layout(keys[:, c:].copy()))
        assert _same(lay, whole), name
        seen += 1
    assert seen >= 12


def test_layout_ties_keep_ids_ascending_and_old_first():
    """equal keys (a popular key, empty bands): ids ascend inside the run, and a batch record goes behind every old one"""
    keys = np.array([[7, 3, 7, 7, 3, 0xFFFF, 7, 0xFFFF]], dtype=np.uint64)
    sk, ids, dirw = AC.restate_layout(keys)
    for v in (3, 7, 0xFFFF):
        run = ids[0][sk[0] == v]
        assert np.array_equal(run, np.sort(run))
    merged = AC.restate_merge(AC.restate_layout(keys[:, :5].copy()), AC.restate_layout(keys[:, 5:].copy()))
    assert _same(merged, (sk, ids, dirw))
    assert dirw[0] == 0 and dirw[-1] == 8 and np.all(np.diff(dirw.astype(np.int64)) >= 0)


def test_the_abi_names_the_append_entry_points():
    from qrlsh import _lib
    hdr = open(os.path.join(ROOT, "include", "qrlsh.h")).read()
    for name in ("qrlsh_index_append", "qrlsh_index_append_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b%s\(" % name, hdr)
    assert len(_lib.SIGNATURES["qrlsh_index_append"][1]) == 13
