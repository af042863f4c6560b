"""Timing probe of replacing queries of a built index in place with its top-K lists kept exact (qrlsh_rows_replace,
qrlsh_index_replace, qrlsh_lists_replace_*, csrc/replace.hip) on one GPU.

Shapes: index and lists of configs[2] (10 M queries x 128 / 32 bands, D = 32768, bench.py's synthetic recipe) from the
hot path itself (pipeline.query_similarities), then seeded random sets of m = 1, 1024, 16 384 and 1 M queries that take
the answer sets of a second synthetic draw.  Every shape is first checked in this process:
QueryIndex.set(update_lists=True) leaves band arrays, rows and norms that equal a fresh QueryIndex over the new queries,
and lists that equal, element for element, a full pipeline.query_similarities over them with the same K.  Then
  * per-kernel times (the library's HIP-event profiler, mean of --reps after a warm-up) and the call time of
    QueryIndex.replace(update_lists=True) on a copy of the index with rows of its own, made outside the timed region,
  * the call time of the two things it stands in for, in the same process:
      (a) remove + append with update_lists=True, plus the permutation of the rows and list ids back to their positions;
      (b) the full run over the new queries plus the index build from its result,
  * the replacement's algorithmic bytes -- bands: keys read once, ids twice, keys and ids written once, the new keys read
    once more by the directory kernel (36 B per record); rows: the m rows; lists: src / dst read by the mark, dst read
    and a word written by the kept pass, src / dst / val and the word read and src / dst / val written by the fill --
    against the 6.29 TB/s streaming-copy rate DESIGN section 4 records.

    python tools/index_replace_probe.py [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/index_replace_probe.json.
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
BANDS = ("index_replace_count", "index_replace_rank", "index_replace_fill", "index_dir")
ROWS = ("rows_replace",)
LISTS = ("lists_remove_mark", "lists_records", "lists_kept", "lists_len", "lists_old_rows", "lists_rev_rows",
         "lists_fill_old", "lists_fill_rev", "lists_fill_probed", "lists_total")
PROBES = ("index_probe_count", "index_probe_fill", "index_score", "index_select", "index_compact")


def _own(base):
    """a copy of the index whose rows are its own (the replacement writes rows in place)"""
    qi = copy.copy(base)
    qi._sig_buf, qi._norm2_buf = base.sig.clone(), base.norm2.clone()
    qi.sig, qi.norm2 = qi._sig_buf[:qi.n], qi._norm2_buf[:qi.n]
    qi._own_rows = True
    return qi


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
        raise SystemExit("index_replace_probe needs a GPU")
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
        boff, brows = synth.synth_csr(m, D, seed=1000 + m)           # the new answer sets, batch row x for given[x]
        bsizes = boff[1:] - boff[:-1]
        sizes2 = sizes.clone()
        sizes2[given] = bsizes
        off2 = torch.cat((torch.zeros((1,), dtype=offsets.dtype, device="cuda"),
                          torch.cumsum(sizes2, 0).to(offsets.dtype))).contiguous()
        rows2 = torch.empty((int(off2[-1].item()),), dtype=rows.dtype, device="cuda")
        keep = torch.ones((nq,), dtype=torch.bool, device="cuda")
        keep[given] = False
        own = torch.repeat_interleave(keep, sizes)                   # entries of the old CSR that stay
        dest = torch.repeat_interleave(keep, sizes2)
        rows2[dest] = rows[own]
        start = off2[:-1][given]
        rows2[torch.repeat_interleave(start - boff[:-1], bsizes) + torch.arange(brows.numel(), device="cuda")] = brows
        del own, dest
        full = pipeline.query_similarities(off2, rows2, table, b, K)
        fresh = QueryIndex.from_result(full, table)
        qi = _own(base)
        bsig, bnorm2, bkeys = qi.signatures(boff, brows)
        qi.replace(given, bsig, bnorm2, bkeys, update_lists=True)
        for name, g, f in zip(("src", "dst", "val"), qi.lists, (full.src, full.dst, full.val)):
            if g.shape != f.shape or not torch.equal(g, f):
                raise SystemExit("replace m=%d: %s differs from the full run over the new queries" % (m, name))
        for name in ("keys", "ids", "dir", "sig", "norm2"):
            g, f = getattr(qi, name), getattr(fresh, name)
            if g.shape != f.shape or not torch.equal(g, f):
                raise SystemExit("replace m=%d: %s differs from a fresh index over the new queries" % (m, name))
        total, picked = int(full.src.numel()), qi.last_picked
        del qi, fresh, full

        work = _own(base)      # rows of its own, made once outside the timed region: every rep writes the same m rows

        def replace():
            copy.copy(work).replace(given, bsig, bnorm2, bkeys, update_lists=True)
        call_ms, kern = timed(replace, a.reps)
        del work

        order = torch.argsort(given)

        def remove_append():
            q = copy.copy(base)      # the removal writes out of place
            new_pos = q.remove(given, update_lists=True)
            q.append(bsig[order], bnorm2[order].contiguous(), bkeys[:, order].contiguous(), update_lists=True)
            back = torch.cat((torch.nonzero(new_pos >= 0).flatten(), given[order]))     # id now -> position it stands for
            inv = torch.empty_like(back)
            inv[back] = torch.arange(nq, device="cuda")
            sig, norm2 = q.sig[inv], q.norm2[inv]                                       # rows back at their positions
            s, d = back[q.lists[0].to(torch.int64)], back[q.lists[1].to(torch.int64)]
            by_src = torch.argsort(s, stable=True)
            return sig, norm2, s[by_src], d[by_src], q.lists[2][by_src]
        ra_ms, ra_kern = timed(remove_append, a.reps)

        def rerun():
            QueryIndex.from_result(pipeline.query_similarities(off2, rows2, table, b, K), table)
        rcall_ms, rkern = timed(rerun, a.reps)
        del off2, rows2
        torch.cuda.empty_cache()
        band_by = b * nq * (8 + 4 + 4 + 8 + 4 + 8)
        rows_by = 2 * (row_bytes + 8) * m
        list_by = 8 * n_edges + (4 + 8 + 16) * n_edges + (12 + 8) * n_edges + 12 * total
        parts = {}
        for name, labels, by in (("bands", BANDS, band_by), ("rows", ROWS, rows_by), ("lists", LISTS, list_by)):
            ms = sum(kern.get(k, 0.0) for k in labels)
            parts[name] = {"kernels_ms": round(ms, 4), "algorithmic_bytes": by,
                           "byte_floor_ms_at_6.29TBps": round(by / COPY_RATE * 1e3, 4),
                           "share_of_copy_rate": round(by / COPY_RATE / (ms * 1e-3), 3) if ms else None,
                           "hbm_peak_fraction": round(by / HBM_PEAK / (ms * 1e-3), 3) if ms else None}
        parts["probes"] = {"kernels_ms": round(sum(kern.get(k, 0.0) for k in PROBES), 4), "rows": m + picked}
        rec = {"shape": "index and lists of 10M x 128/32, K=%d, m=%d replaced" % (K, m),
               "date": datetime.date.today().isoformat(), "n": nq, "m": m, "K": K, "stored_entries": n_edges,
               "output_entries": total, "picked_rows": picked, "checked_against_fresh_build_and_full_run_same_process": True,
               "replace_update_lists": {"call_ms": round(call_ms, 4), "kernels_ms": kern,
                                        "kernels_total_ms": round(sum(kern.values()), 4)},
               "remove_plus_append_plus_permutation": {"call_ms": round(ra_ms, 4),
                                                       "kernels_total_ms": round(sum(ra_kern.values()), 4)},
               "full_run_plus_index_build": {"call_ms": round(rcall_ms, 4), "kernels_total_ms": round(sum(rkern.values()), 4)},
               "remove_append_over_replace_call": round(ra_ms / call_ms, 2),
               "rebuild_over_replace_call": round(rcall_ms / call_ms, 2),
               "algorithmic_bytes": band_by + rows_by + list_by, **parts}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "index_replace_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
