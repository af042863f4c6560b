"""No call touches a byte outside the workspace it declares, and no result depends on what a workspace held before.

Every workspace of the Python layer is allocated by qrlsh.ops._ws.  Here it is replaced by one that allocates 4096 guard
bytes on either side of the buffer, fills all of it with 0xA5 and hands out the middle: ordinary allocated memory, so a
layout that walks past the size its *_workspace_bytes export states cannot fault -- it shows as a changed guard byte, or
(a carve that falls short of a region the kernels use) as a result that differs from the unpatched run, whose workspace
holds whatever the allocator left there.  Each case is the smallest shape its case module uses and runs twice, plain and
patched; the last test proves that the cases reach every size export of include/qrlsh.h."""
import collections
import importlib.util
import os

import numpy as np
import pytest
import torch

import diversify_cases as DC
import evaluate_cases as EC
import live_sequence_cases as S
import rank_grid_cases as RGC
import shard_cases as SH
import users_cases as UC

pytestmark = pytest.mark.gpu

import qrlsh  # noqa: E402
from qrlsh import _lib, ops, pipeline, predict, users  # noqa: E402

DEV = "cuda"
GUARD = 4096
FILL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# size exports no path of the Python layer calls, with the reason
NOT_CALLED = {
    "qrlsh_predict_users_workspace_bytes": "the call takes no workspace (the export returns 0): predict_users passes none",
}


def _size_exports():
    spec = importlib.util.spec_from_file_location("workspace_sizes", os.path.join(ROOT, "tools", "workspace_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [name for name, _ in mod.size_exports()]


class Guarded:
    """the replacement of ops._ws, the allocations it made and the size exports called while it was in place"""

    def __init__(self):
        self.made = []
        self.sizes = collections.Counter()

    def ws(self, nbytes, device):
        n = max(int(nbytes), 16)                      # at least 16 bytes, as ops._ws guarantees
        whole = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=device)
        assert whole.data_ptr() % 256 == 0
        self.made.append((whole, n))
        return whole[GUARD:GUARD + n]                 # GUARD is a multiple of 256: the slice keeps the alignment

    def damaged(self):
        """[(allocation number, bytes, which guard, first changed byte)] over every allocation so far; forgets them"""
        torch.cuda.synchronize()
        out = []
        for at, (whole, n) in enumerate(self.made):
            for side, part in (("front", whole[:GUARD]), ("back", whole[GUARD + n:])):
                bad = torch.nonzero(part != FILL)
                if bad.numel():
                    out.append((at, n, side, int(bad[0])))
        self.made.clear()
        return out


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)     # (a copy: some case arrays are read-only)


def _flat(x, out):
    """every array, tensor and number a result holds, in a fixed order"""
    if isinstance(x, torch.Tensor):
        out.append(x.detach().cpu().numpy())
    elif isinstance(x, np.ndarray):
        out.append(x)
    elif isinstance(x, (bool, int, float, str, np.generic)):
        out.append(np.asarray(x))
    elif isinstance(x, dict):
        for k in sorted(x, key=repr):
            _flat(x[k], out)
    elif isinstance(x, (list, tuple)):
        for y in x:
            _flat(y, out)
    elif hasattr(x, "to_numpy"):
        out.append(x.to_numpy())
    elif x is not None and hasattr(x, "__dict__"):
        _flat({k: v for k, v in vars(x).items() if not callable(v)}, out)
    return out


def _same(a, b):
    return len(a) == len(b) and all(
        x.shape == y.shape and x.dtype == y.dtype and (x.tobytes() == y.tobytes() if x.dtype != object else (x == y).all())
        for x, y in zip(a, b))


# ---- the cases: each returns its results ---------------------------------------------------------------------------------
def _hot(topk):
    nq, D, P, b, K = 3000, 4096, 128, 32, 8
    off, rows = qrlsh.synth_csr(nq, D, seed=5, device=DEV)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42), DEV)
    res = pipeline.query_similarities(off, rows, table, b, K, topk=topk)
    return res.pairs, res.milli, res.src, res.dst, res.val


def _general_bucket_path():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 400, size=(2, 1500)).astype(np.int64)
    sk, sid = ops.bucket_sort(dev(keys))
    out = ops.emit_pairs(sk, sid, 2)
    return ops.unique_sorted(ops.sort_pairs(out, 1500))


def _two_level_partition():
    """the bucket partition with part_bits > 8: the second set of cursors and the buffers between the levels"""
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 400, size=(2, 1500)).astype(np.int64)
    out = ops.emit_pairs_fast(dev(keys), 2, part_bits=9)
    assert out is not None
    return torch.sort(out).values          # (the parts reserve their output ranges in no fixed order)


def _words(seed=22):
    """emitted pair words i << 32 | j, i < j < 2^20 spread over the id space (the fixed regions are sized by the mean),
    each three times over, shuffled"""
    rng = np.random.default_rng(seed)
    i = rng.integers(0, (1 << 20) - 64, size=30000).astype(np.uint64)
    j = i + 1 + rng.integers(0, 40, size=30000).astype(np.uint64)
    w = np.repeat((i << np.uint64(32)) | j, 3)
    return w[rng.permutation(len(w))]


DEDUP = {   # dedup_path -> (nq, scatter) that selects it in ops.unique_pairs (tests/test_gpu_parity.py, test_gpu_sort.py)
    "regions-in-lds (scattered)": ((1 << 20) - 1, True),
    "regions-in-lds": ((1 << 20) - 1, False),
    "rows-in-lds": (1 << 31, True),
    "full-sort": (1 << 28, True),           # 28 id bits leave 4 group bits: below ops.REGION_MIN_GROUP_BITS
}


def _dedup(path):
    nq, scatter = DEDUP[path]
    stats = {}
    got = ops.unique_pairs(dev(_words().view(np.int64)), nq, stats, scatter=scatter)
    assert stats["dedup_path"] == path, stats
    return got


def _live_sequence():
    """one committed schedule through the Recommender: index build, append, probe, finish, remove and replace, the lists'
    update, remove, replace and cut, the id maps, user lists, user rows and table rows; then one served answer"""
    from test_gpu_live_sequence import Served
    with pytest.MonkeyPatch.context() as mp:
        s, trace, served = Served(mp), S.run(2), []
        for i, step in enumerate(trace):
            s.do(step)
            if i in S.serve_points(len(trace)) and step.note["longest"] <= S.SERVED_MAX:
                chosen = [0, s.rec.ratings.shape[0] - 1]
                served.append((s.rec.predict_users(chosen), s.rec.recommend_users(chosen, 5)))
        assert served
        return (s.rec._live_lists(), s.rec.current_query_similarities(),
                [getattr(s.ui, f) for f in ("idx", "milli", "len")], served)


def _serving():
    """(ratings, (src, dst, milli) tensors, qs, us): evaluate_cases' small random case, 6 users x 2500 queries"""
    ratings, coo, qs, us = EC.random_case(25, 6, 2500, 12, 4)
    return ratings, tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo), qs, us


def _predict():
    ratings, coo, _, us = _serving()
    return (predict.fill_predictions(ratings, *coo, us, device=DEV),
            predict.fill_predictions(ratings, *coo, us, device=DEV, transpose_lists=False))


def _recommend():
    ratings, coo, _, us = _serving()
    pred = predict.fill_predictions(ratings, *coo, us, device=DEV)
    from qrlsh import recommend
    return (recommend.top_k(ratings, pred, 7, slices=2, device=DEV), recommend.top_k(ratings, pred, 7, device=DEV),
            recommend.for_users(ratings, *coo, us, [5, 0, 3], 7, slices=2, device=DEV),
            recommend.for_users(ratings, *coo, us, [5, 0, 3], 7, device=DEV))


def _evaluate():
    ratings, coo, _, us = _serving()
    return qrlsh.evaluate(ratings, *coo, us, fraction=0.5, seed=3, want_predictions=True, device=DEV)


def _tune_grid():
    ratings, coo, _, us = _serving()
    weights = [(0.5, 0.5, 50.0), (1.0, 0.0, 40.0), (0.25, 0.75, 60.0)]
    return qrlsh.evaluate_grid(ratings, *coo, us, weights, q_cuts=[2, 12], u_cuts=[1, 4], fraction=0.5, seed=3,
                               want_per_user=True, device=DEV)


def _split():
    ratings, coo, _, us = _serving()
    keep = EC.kept_mask(*ratings.shape, 9, EC.keep_of(0.3)) & (ratings != 0)
    return np.where(keep, 0, ratings).astype(np.int32), ratings, coo, us


def _rank_eval():
    train, truth, coo, us = _split()
    return (qrlsh.evaluate_ranking(train, truth, *coo, us, 5, 60, slices=2, device=DEV),
            qrlsh.evaluate_ranking(train, truth, *coo, us, 5, 60, users=[4, 1], candidates="heldout", device=DEV))


def _rank_grid():
    train, truth, coo, _, us, _ = RGC.main_case()
    coo = tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in coo)
    return qrlsh.evaluate_ranking_grid(train, truth, *coo, us, 5, 60, RGC.main_weights()[:3], q_cuts=[2, 6], u_cuts=[1, 3],
                                       want_per_request=True, device=DEV)


def _diversify():
    c = DC.small_case(1)
    idx, val, avail = c.arrays()
    coo = tuple(torch.as_tensor(np.asarray(x), dtype=torch.int32) for x in c.coo())
    settings = [(0, 1001), (30, 1001), (0, 700)]
    return (qrlsh.diversify(idx, val, avail, *coo, c.nq, c.k, penalty=30, max_sim=900, device=DEV),
            qrlsh.list_redundancy(idx[:, :c.k], *coo, c.nq, device=DEV),
            qrlsh.diversify_grid(idx, val, avail, *coo, c.nq, c.k, settings, want_lists=True, device=DEV))


def _users():
    r, labels = UC.label_case()
    K = UC.max_candidates(r.shape[0])
    from qrlsh.userlists import UserLists
    ul = UserLists.build(r, labels, K)
    base, base_labels, rows, row_labels = UC.add_users_case()
    grown = UserLists.build(base, base_labels, K)
    grown.add_users(rows, labels=row_labels)           # the nearest-rows search and the row statistics
    return (users.standardized_gram(dev(r)), users.user_similarities(r, labels, K, DEV), ul.coo(), grown.coo())


def _shard():
    from qrlsh.dist import HipBackend
    H = HipBackend()
    case = SH.idset_case(5003, 5, 2, 100, seed=2)
    p = dev(np.ascontiguousarray(case["pairs"]).view(np.int64))
    rid = H.remote_ids(p, case["q0"], case["nql"], case["nids"], case["world"])
    need = H.remote_id_list(rid, int(rid.bounds[-1].item()))
    offs, rows, _ = SH.shard_sets(5, 61, 65536, seed=5, empty_shard=3)
    return (rid.bounds, need, H.remap_pairs(p, rid), H.gather_sets(dev(SH.set_ids(5, 61, 17, seed=17)), dev(offs), dev(rows), 61))


CASES = {
    "hot-path-select": lambda: _hot("select"),
    "hot-path-sort": lambda: _hot("sort"),
    "general-bucket-path": _general_bucket_path,
    "two-level-partition": _two_level_partition,
    **{"dedup-" + path.replace(" ", "-"): (lambda path=path: _dedup(path)) for path in DEDUP},
    "live-sequence": _live_sequence,
    "predict": _predict,
    "recommend": _recommend,
    "evaluate": _evaluate,
    "tune-grid": _tune_grid,
    "rank-eval": _rank_eval,
    "rank-grid": _rank_grid,
    "diversify": _diversify,
    "users": _users,
    "shard": _shard,
}


@pytest.fixture(scope="module")
def outcome():
    """outcome(name) -> (plain results, patched results, damaged guards) of a case, each case run once per session;
    .sizes counts the size exports called under the patch"""
    lib = _lib.load()
    guarded, done = Guarded(), {}

    def counted(name, fn):
        def call(*args):
            guarded.sizes[name] += 1
            return fn(*args)
        return call

    def run(name):
        if name not in done:
            plain = _flat(CASES[name](), [])
            torch.cuda.synchronize()
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(ops, "_ws", guarded.ws)
                for export in _size_exports():
                    mp.setattr(lib, export, counted(export, getattr(lib, export)))
                patched = _flat(CASES[name](), [])
                made = len(guarded.made)
                done[name] = (plain, patched, guarded.damaged(), made)
        return done[name]

    run.sizes = guarded.sizes
    return run


@pytest.mark.parametrize("name", list(CASES))
def test_guards_stay_intact_and_results_do_not_depend_on_the_workspace(outcome, name):
    plain, patched, damaged, made = outcome(name)
    assert made > 0, "the case allocated no workspace through ops._ws"
    assert not damaged, "bytes outside a declared workspace were written: %s" % damaged[:5]
    assert _same(plain, patched), "the results differ from those of the unpatched run"


def test_every_size_export_is_called_under_the_patch(outcome):
    for name in CASES:
        outcome(name)
    exports = _size_exports()
    assert len(exports) >= 39 and set(NOT_CALLED) <= set(exports)
    missing = [e for e in exports if outcome.sizes[e] == 0 and e not in NOT_CALLED]
    assert not missing, "size exports no case reached: %s" % missing
    assert not [e for e in NOT_CALLED if outcome.sizes[e]], "listed as never called, but called"
