"""Timing probe of keeping the top-K lists current when queries are appended (qrlsh_index_probe_finish_indexed,
qrlsh_lists_update_*, csrc/lists.hip) on one GPU.

Shapes: index and lists of configs[2] (10 M queries x 128 / 32 bands, D = 32768, bench.py's synthetic recipe) from the
hot path itself (pipeline.query_similarities), then batches of m = 1, 1024, 16 384 and 1 M further queries of the same
recipe.  Every shape is first checked: QueryIndex.add(update_lists=True) leaves lists that equal, element for element,
a full pipeline.query_similarities over all n + m queries with the same K, in this process.  Then
  * per-kernel times (the library's HIP-event profiler, mean of --reps after a warm-up) and the call time of
    append + probe + finish + update (the batch's keys are restored by a copy of [b][m] words before every call),
  * the call and kernel time of the full run over the n + m queries it replaces,
  * the update's algorithmic bytes -- fill: 12 B read per stored entry and 12 B written per output entry; bookkeeping:
    the zeroed row extents, src / dst read once more, the lengths and their scan -- against the 6.29 TB/s
    streaming-copy rate DESIGN section 4 records.

    python tools/lists_update_probe.py [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/lists_update_probe.json.
"""
import argparse
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

import torch  # noqa: E402

from query_index_probe import HBM_PEAK, timed  # noqa: E402

COPY_RATE = 6.29e12      # streaming copy, DESIGN section 4
FILL = ("lists_fill_old", "lists_fill_rev", "lists_fill_probed")
BOOK = ("lists_records", "lists_rev_rows", "lists_old_rows", "lists_len", "lists_total")


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
        raise SystemExit("lists_update_probe needs a GPU")
    t0 = time.time()
    batches = [int(x) for x in a.batches.split(",")]
    nq, extra, D, P, b = a.nq, max(batches), 32768, 128, 32
    K = pipeline.max_candidates(nq)
    offsets, rows = synth.synth_csr(nq + extra, D, seed=0)
    off_h = offsets.cpu().numpy()
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42))

    def sub(lo, hi):
        return (offsets[lo:hi + 1] - offsets[lo]).contiguous(), rows[int(off_h[lo]):int(off_h[hi])].contiguous()

    res = pipeline.query_similarities(*sub(0, nq), table, b, K)
    src, dst, val = res.src, res.dst, res.val
    n_edges = src.numel()
    base = QueryIndex.from_result(res, table)
    keys, ids, dirw = base.keys, base.ids, base.dir
    out = []
    for m in batches:
        n = nq + m
        allq = sub(0, n)
        full = pipeline.query_similarities(*allq, table, b, K)
        qi = QueryIndex.from_result(res, table, lists=True)
        qi.add(*sub(nq, n), update_lists=True)
        for name, g, f in zip(("src", "dst", "val"), qi.lists, (full.src, full.dst, full.val)):
            if g.shape != f.shape or not torch.equal(g, f):
                raise SystemExit("update m=%d: %s differs from the full run over all %d queries" % (m, name, n))
        total = int(full.src.numel())
        rows_sig, rows_norm = qi.sig, qi.norm2            # the n + m rows of the grown index
        new_sig, new_norm = rows_sig[nq:], rows_norm[nq:].contiguous()
        new_keys = ops.band_keys(ops.sig_to_int32(new_sig), b)
        del qi, full
        work = new_keys.clone()
        n_raw = [0]

        def update():
            work.copy_(new_keys)
            grown = ops.index_append(keys, ids, dirw, work)
            raw, pws = ops.index_probe(*grown, P // b, new_keys)
            off, idx, milli, _, sk = ops.index_finish(rows_sig, rows_norm, new_sig, new_norm, b, pws, raw, K, first_id=nq)
            n_raw[0] = raw.numel()
            return ops.lists_update(src, dst, val, nq, m, b, K, raw, sk, off, idx, milli)
        call_ms, kern = timed(update, a.reps)

        def rerun():
            pipeline.query_similarities(*allq, table, b, K)
        rcall_ms, rkern = timed(rerun, a.reps)
        torch.cuda.empty_cache()
        fill_by = 12 * n_edges + 12 * total
        book_by = 16 * nq + 8 * n_edges + (16 * nq + 8 * n) + 32 * n + 28 * n_raw[0]
        fill_ms = sum(kern.get(k, 0.0) for k in FILL)
        book_ms = sum(kern.get(k, 0.0) for k in BOOK)
        kms, rms = sum(kern.values()), sum(rkern.values())
        rec = {"shape": "lists of 10M x 128/32, K=%d, updated with m=%d" % (K, m), "date": datetime.date.today().isoformat(),
               "n": nq, "m": m, "K": K, "stored_entries": n_edges, "output_entries": total, "raw_words": n_raw[0],
               "checked_against_full_run_same_process": True,
               "append_probe_finish_update": {"call_ms_incl_batch_key_copy": round(call_ms, 4), "kernels_ms": kern,
                                              "kernels_total_ms": round(kms, 4)},
               "full_run_same_queries": {"call_ms": round(rcall_ms, 4), "kernels_total_ms": round(rms, 4)},
               "update_over_full_run_call": round(call_ms / rcall_ms, 3),
               "full_run_over_update_call": round(rcall_ms / call_ms, 2),
               "fill": {"kernels_ms": round(fill_ms, 4), "algorithmic_bytes": fill_by,
                        "byte_floor_ms_at_6.29TBps": round(fill_by / COPY_RATE * 1e3, 4),
                        "over_byte_floor": round(fill_ms / (fill_by / COPY_RATE * 1e3), 2),
                        "hbm_peak_fraction": round(fill_by / HBM_PEAK / (fill_ms * 1e-3), 3)},
               "bookkeeping": {"kernels_ms_without_memset_sort_scan": round(book_ms, 4), "algorithmic_bytes": book_by,
                               "byte_floor_ms_at_6.29TBps": round(book_by / COPY_RATE * 1e3, 4)}}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "lists_update_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
