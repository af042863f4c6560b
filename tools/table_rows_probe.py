"""Timing probe of dataset rows that come and go under a live index (qrlsh.LiveTable.add_rows / remove_rows,
qrlsh_table_rows_mark / _fill, qrlsh_bitmaps_set_rows, csrc/tablerows.hip) on one GPU.

Shape: a synthetic table of D = 32768 rows x 16 features of 4 values each in a table of capacity D + 8192, and --nq
queries (default configs[2]'s 10 M) that constrain 5 or 6 random features each (answer sets of 32 and 8 rows on average),
128 permutations / 32 bands, K = round(log_1.5 nq); index and lists from the hot path itself.  Batches of 1, 16, 256 and
4096 rows are added (random cells) and removed (random live rows).  Every batch is first checked in this process: index
arrays and lists against a fresh QueryIndex / pipeline.query_similarities over the edited table's answer sets.  Then, in
the same process,
  * the call time of the operation (table and index copied outside the timed region: a row operation writes the index's
    rows in place) and its per-kernel times (the library's HIP-event profiler);
  * the route it replaces: answer_sets over all queries + the hot path (MinHash included) + the index build;
  * for additions, the fill kernel against recomputing the changed queries with answer_sets + MinHash.

    python tools/table_rows_probe.py [--nq N] [--reps N] [--out DIR] [--budget SECONDS]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/table_rows_probe.json (rewritten after
every result).  --budget: no new batch is started once that many seconds have passed.
"""
import argparse
import copy
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from index_replace_probe import _own  # noqa: E402
from query_index_probe import timed  # noqa: E402

NFEAT, NVALS, D, SPARE, P, BANDS = 16, 4, 32768, 8192, 128, 32


def _own_table(lt):
    """a copy of the table that row operations may write"""
    t = copy.copy(lt)
    t.dictionary = copy.deepcopy(lt.dictionary)
    t.bitmaps, t.cells = lt.bitmaps.clone(), lt.cells.clone()
    t._cells, t.live = lt._cells.copy(), lt.live.copy()
    return t


def _op_ms(op, prepare, reps):
    """(mean call ms, {kernel label: ms per call}) of op(*prepare()), the preparation outside the timed region"""
    from qrlsh import _lib
    op(*prepare())
    total = 0.0
    for _ in range(reps):
        args = prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        op(*args)
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
    held = [prepare() for _ in range(reps)]
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    for args in held:
        op(*args)
    torch.cuda.synchronize()
    rep = _lib.prof_report()
    _lib.prof_enable(False)
    return total / reps, {lab: round(ms / reps, 4) for lab, (cnt, ms) in sorted(rep.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nq", type=int, default=10_000_000)
    ap.add_argument("--batches", default="1,16,256,4096")
    ap.add_argument("--budget", type=float, default=1e9)
    a = ap.parse_args()
    from qrlsh import ops, pipeline
    from qrlsh.index import QueryIndex
    from qrlsh.table import LiveTable
    if not torch.cuda.is_available():
        raise SystemExit("table_rows_probe needs a GPU")
    t0 = time.time()
    nq = a.nq
    K = pipeline.max_candidates(nq)
    rng = np.random.default_rng(1)
    base_id = 1 + np.arange(NFEAT) * NVALS
    lt = LiveTable(NFEAT, D + SPARE, "cuda")
    for f in range(NFEAT):
        lt.dictionary.maps[f] = {str(v): int(base_id[f] + v) for v in range(NVALS)}
    lt.dictionary.nrows = 1 + NFEAT * NVALS
    lt._place((rng.integers(0, NVALS, size=(D, NFEAT)) + base_id).astype(np.int32), np.arange(D, dtype=np.int64))
    g = torch.Generator(device="cuda").manual_seed(2)
    rank = torch.rand((nq, NFEAT), generator=g, device="cuda").argsort(dim=1).argsort(dim=1)
    k = 5 + torch.randint(0, 2, (nq, 1), generator=g, device="cuda")
    vals = torch.randint(0, NVALS, (nq, NFEAT), generator=g, device="cuda") + torch.from_numpy(base_id).cuda()
    lt.qrows = torch.where(rank < k, vals, torch.full_like(vals, -1)).to(torch.int32).contiguous()
    del rank, vals, k
    table = ops.perm_table(ops.legacy_permutations(P, D + SPARE, seed=42))
    off, rows = lt.answer_sets()
    res = pipeline.query_similarities(off, rows, table, BANDS, K)
    base = QueryIndex.from_result(res, table, lists=True)
    mean_set = rows.numel() / nq
    del off, rows
    out = []

    def save():
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "table_rows_probe.json"), "w") as fh:
                json.dump(out, fh, indent=1)

    for kind in ("add", "remove"):
        for m in (int(x) for x in a.batches.split(",")):
            if time.time() - t0 > a.budget:
                continue
            er = np.random.default_rng(10 * m + len(kind))
            if kind == "add":
                given = er.integers(0, NVALS, size=(m, NFEAT)).astype(str).astype(object)
                op = lambda t, q: t.add_rows(given, q, update_lists=True)
            else:
                given = np.sort(er.choice(D, m, replace=False))
                op = lambda t, q: t.remove_rows(given, q, update_lists=True)
            prepare = lambda: (_own_table(lt), _own(base))
            t, qi = prepare()
            op(t, qi)
            matched, changed, picked = t.last_matched, t.last_changed, qi.last_picked
            off2, rows2 = t.answer_sets()
            full = pipeline.query_similarities(off2, rows2, table, BANDS, K)
            fresh = QueryIndex.from_result(full, table)
            for name, x, y in zip(("src", "dst", "val"), qi.lists, (full.src, full.dst, full.val)):
                if x.shape != y.shape or not torch.equal(x, y):
                    raise SystemExit("%s m=%d: %s differs from the full run over the edited table" % (kind, m, name))
            for name in ("keys", "ids", "dir", "sig", "norm2"):
                x, y = getattr(qi, name), getattr(fresh, name)
                if x.shape != y.shape or not torch.equal(x, y):
                    raise SystemExit("%s m=%d: %s differs from a fresh index over the edited table" % (kind, m, name))
            del full, fresh, qi
            call_ms, kern = _op_ms(op, prepare, a.reps)
            extra = {}
            if kind == "add" and changed:
                # the fill kernel against the recompute of the changed queries (the table `t` holds the batch)
                batch = ops.RowBatch(t._cells[D:D + m], np.arange(D, D + m), "cuda")
                ids = ops.table_rows_mark(lt.qrows, batch, table, base.sig)[0].members()
                fill_ms, _ = timed(lambda: ops.table_rows_fill(lt.qrows, batch, table, base.sig, ids), a.reps)

                def recompute():
                    o, r = t.answer_sets(lt.qrows[ids.to(torch.int64)])
                    return base.signatures(o, r)
                rec_ms, rec_kern = timed(recompute, a.reps)
                extra = {"fill_call_ms": round(fill_ms, 4), "recompute_changed_call_ms": round(rec_ms, 4),
                         "recompute_changed_kernels_ms": rec_kern, "recompute_over_fill": round(rec_ms / fill_ms, 2)}

            def rerun():
                o, r = t.answer_sets()
                QueryIndex.from_result(pipeline.query_similarities(o, r, table, BANDS, K), table)
            full_ms, full_kern = timed(rerun, max(1, a.reps - 1))
            del off2, rows2, t
            torch.cuda.empty_cache()
            rec = {"shape": "%d queries x %d/%d over %d rows x %d features, K=%d, %s %d rows" % (nq, P, BANDS, D, NFEAT, K, kind, m),
                   "date": datetime.date.today().isoformat(), "n": nq, "operation": kind, "rows": m, "K": K,
                   "mean_answer_set": round(mean_set, 2), "matched_queries": int(matched), "changed_queries": int(changed),
                   "picked_rows": int(picked) if picked is not None else None,
                   "checked_against_fresh_index_and_full_run_same_process": True,
                   "call_ms": round(call_ms, 4), "kernels_ms": kern, "kernels_total_ms": round(sum(kern.values()), 4),
                   "table_rows_kernels_ms": round(sum(v for k_, v in kern.items() if k_.startswith(("table_rows", "bitmaps_set"))), 4),
                   "full_route_call_ms": round(full_ms, 3), "full_route_kernels_total_ms": round(sum(full_kern.values()), 3),
                   "full_route_over_call": round(full_ms / call_ms, 2)}
            rec.update(extra)
            out.append(rec)
            print(json.dumps(rec), flush=True)
            save()
    print("total %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
