"""Timing probe of removing queries from a built index with its top-K lists kept exact (qrlsh_idmap_*, qrlsh_rows_remove,
qrlsh_index_remove, qrlsh_lists_remove_*, qrlsh_index_probe_finish_rows, csrc/remove.hip) on one GPU.

Shapes: index and lists of configs[2] (10 M queries x 128 / 32 bands, D = 32768, bench.py's synthetic recipe) from the
hot path itself (pipeline.query_similarities), then seeded random sets of m = 1, 1024, 16 384 and 1 M queries removed.
Every shape is first checked in this process: QueryIndex.remove(update_lists=True) leaves band arrays, rows and norms
that equal a fresh QueryIndex over the surviving queries, and lists that equal, element for element, a full
pipeline.query_similarities over them with the same K.  Then
  * per-kernel times (the library's HIP-event profiler, mean of --reps after a warm-up) and the call time of
    QueryIndex.remove(update_lists=True) on a shallow copy of the index (the removal writes out of place),
  * the call time of what it replaces: the full run over the survivors plus the index build from its result,
  * the removal's algorithmic bytes -- bands: keys read once, ids twice, keys and ids written once, the new keys read
    once more by the directory kernel; rows: read and written once; lists: src / dst read by the mark and the count,
    src / dst / val read and written by the fill -- against the 6.29 TB/s streaming-copy rate DESIGN section 4 records.

    python tools/index_remove_probe.py [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/index_remove_probe.json.
"""
import argparse
import copy
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd"), os.path.join(ROOT, "tests"),
          os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from query_index_probe import HBM_PEAK, timed  # noqa: E402

COPY_RATE = 6.29e12      # streaming copy, DESIGN section 4
BANDS = ("index_remove_count", "index_remove_fill", "index_dir")
ROWS = ("rows_remove",)
LISTS = ("lists_remove_mark", "lists_remove_count", "lists_remove_fill", "lists_fill_probed", "lists_remove_total")
REPROBE = ("index_probe_count", "index_probe_fill", "index_score", "index_select", "index_compact")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nq", type=int, default=10_000_000)
    ap.add_argument("--batches", default="1,1024,16384,1048576")
    a = ap.parse_args()
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    if not torch.cuda.is_available():
        raise SystemExit("index_remove_probe needs a GPU")
    t0 = time.time()
    batches = [int(x) for x in a.batches.split(",")]
    nq, D, P, b = a.nq, 32768, 128, 32
    K = pipeline.max_candidates(nq)
    offsets, rows = synth.synth_csr(nq, D, seed=0)
    sizes = offsets[1:] - offsets[:-1]
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42))
    res = pipeline.query_similarities(offsets, rows, table, b, K)
    base = QueryIndex.from_result(res, table, lists=True)
    n_edges = res.src.numel()
    row_bytes = P * base.sig.element_size()
    out = []
    for m in batches:
        given = torch.from_numpy(np.random.default_rng(m).choice(nq, m, replace=False)).cuda()
        keep = torch.ones((nq,), dtype=torch.bool, device="cuda")
        keep[given] = False
        off2 = torch.cat((torch.zeros((1,), dtype=offsets.dtype, device="cuda"),
                          torch.cumsum(sizes[keep], 0).to(offsets.dtype))).contiguous()
        rows2 = rows[torch.repeat_interleave(keep, sizes)].contiguous()
        full = pipeline.query_similarities(off2, rows2, table, b, K)
        fresh = QueryIndex.from_result(full, table)
        qi = copy.copy(base)
        qi.remove(given, update_lists=True)
        for name, g, f in zip(("src", "dst", "val"), qi.lists, (full.src, full.dst, full.val)):
            if g.shape != f.shape or not torch.equal(g, f):
                raise SystemExit("remove m=%d: %s differs from the full run over the %d survivors" % (m, name, nq - m))
        for name in ("keys", "ids", "dir", "sig", "norm2"):
            g, f = getattr(qi, name), getattr(fresh, name)
            if g.shape != f.shape or not torch.equal(g, f):
                raise SystemExit("remove m=%d: %s differs from a fresh index over the %d survivors" % (m, name, nq - m))
        total, picked = int(full.src.numel()), qi.last_picked
        del qi, fresh, full

        def remove():
            copy.copy(base).remove(given, update_lists=True)
        call_ms, kern = timed(remove, a.reps)

        def rerun():
            QueryIndex.from_result(pipeline.query_similarities(off2, rows2, table, b, K), table)
        rcall_ms, rkern = timed(rerun, a.reps)
        del off2, rows2
        torch.cuda.empty_cache()
        left = nq - m
        band_by = b * (nq * (8 + 4 + 4) + left * (8 + 4) + left * 8)
        rows_by = (row_bytes + 8) * (nq + left)
        list_by = 8 * n_edges + 8 * n_edges + 12 * n_edges + 12 * total
        parts = {}
        for name, labels, by in (("bands", BANDS, band_by), ("rows", ROWS, rows_by), ("lists", LISTS, list_by)):
            ms = sum(kern.get(k, 0.0) for k in labels)
            parts[name] = {"kernels_ms": round(ms, 4), "algorithmic_bytes": by,
                           "byte_floor_ms_at_6.29TBps": round(by / COPY_RATE * 1e3, 4),
                           "share_of_copy_rate": round(by / COPY_RATE / (ms * 1e-3), 3) if ms else None,
                           "hbm_peak_fraction": round(by / HBM_PEAK / (ms * 1e-3), 3) if ms else None}
        parts["reprobe"] = {"kernels_ms": round(sum(kern.get(k, 0.0) for k in REPROBE), 4), "rows": picked}
        rec = {"shape": "index and lists of 10M x 128/32, K=%d, m=%d removed" % (K, m),
               "date": datetime.date.today().isoformat(), "n": nq, "m": m, "K": K, "stored_entries": n_edges,
               "output_entries": total, "picked_rows": picked, "checked_against_fresh_build_and_full_run_same_process": True,
               "remove_update_lists": {"call_ms": round(call_ms, 4), "kernels_ms": kern,
                                       "kernels_total_ms": round(sum(kern.values()), 4)},
               "full_run_plus_index_build_over_survivors": {"call_ms": round(rcall_ms, 4),
                                                            "kernels_total_ms": round(sum(rkern.values()), 4)},
               "rebuild_over_remove_call": round(rcall_ms / call_ms, 2), "remove_over_rebuild_call": round(call_ms / rcall_ms, 3),
               "algorithmic_bytes": band_by + rows_by + list_by, **parts}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "index_remove_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
