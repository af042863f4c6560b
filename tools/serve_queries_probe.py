"""Timing probe of serving chosen queries from the live lists (qrlsh.for_queries / predict_queries / query_utility;
qrlsh_recommend_queries, qrlsh_predict_queries) on one GPU.

Shape: the N1 shape of bench.py (2000 users x 100 000 queries, 25 % rated, K = 28 / 19: recommend_users_probe's inputs)
at k = 10 for m = 1, 16, 256 and 4096 chosen queries, and for 16 384 and 65 536 to bracket the m from which the
full matrix is the cheaper route.  Every m is first checked, output for output, against the route
a caller had before -- fill_predictions over all nu x nq cells, the strided slices of the prediction and rating
matrices, their transposes, top_k over them -- and that route is timed in the same process.  Then: the call times, the
per-kernel times (gather, sweep, selection) from the library's HIP-event profiler, and the transaction and byte counts
(nu x n_j scattered reads for the query side, nu strided reads for the gather, the compact column again per slice)
beside a device-to-device copy measured here.  Last, query_utility for all 100 000 columns against fill_predictions plus
torch reductions (words 0 .. 4 compared).  "full_matrix_cheaper_from_m" is the first swept m at which the old route
took no longer than for_queries (null: none did).

    python tools/serve_queries_probe.py [--quick] [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/serve_queries_probe[_quick].json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from recommend_users_probe import inputs, kernels, timed  # noqa: E402

SWEEP_GROUPS, SWEEP_THREADS = 4096, 1024     # PU_AUTO_GROUPS, PU_THREADS of csrc/evalsides.h


def copy_rate(dev, nbytes=1 << 28):
    """GB/s of a device-to-device copy of nbytes (read + write counted)"""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a), 10)
    return 2 * nbytes / (ms * 1e-3) / 1e9


def measure(rt, coo, usims, prepared, full, counts, m, k, reps, dev, out):
    import qrlsh
    from qrlsh import predict
    nu, nq = rt.shape
    rng = np.random.RandomState(m)
    ids = np.sort(rng.choice(nq, size=m, replace=False)).astype(np.int32)
    queries = torch.from_numpy(ids).to(dev)
    q64 = queries.to(torch.int64)

    def slices_and_top(pt):
        cols = pt[:, q64].T.contiguous()
        return cols, qrlsh.top_k(rt[:, q64].T.contiguous(), cols, k, device=dev)

    def old_route():
        return slices_and_top(predict.fill_predictions(rt, *coo, usims, device=dev))

    def serve():
        return qrlsh.for_queries(rt, *coo, prepared, queries, k, device=dev)

    def columns():
        return qrlsh.predict_queries(rt, *coo, prepared, queries, device=dev)

    want_cols, want_top = slices_and_top(full)
    got_top, got_cols = serve(), columns()
    torch.cuda.synchronize()
    if not torch.equal(got_cols, want_cols):
        raise SystemExit("m=%d: the columns differ from fill_predictions" % m)
    for g, w, what in zip(got_top, want_top, ("users", "val", "avail")):
        if not torch.equal(g, w):
            raise SystemExit("m=%d: %s differs from fill_predictions + top_k over the transposes" % (m, what))
    kern = kernels(serve, reps)
    sweep_slices = min(-(-SWEEP_GROUPS // m), -(-nu // SWEEP_THREADS))
    n_j = counts[ids.astype(np.int64)]
    rec = {"shape": "%dx%d (N1)" % (nu, nq), "m": m, "k": k, "sweep_slices": sweep_slices, "kernels_ms": kern,
           "kernels_total_ms": round(sum(kern.values()), 4),
           "for_queries_call_ms": round(timed(serve, reps), 4),
           "predict_queries_call_ms": round(timed(columns, reps), 4),
           "old_route_call_ms": round(timed(old_route, max(2, reps // 3)), 4),
           "old_route_after_the_matrix_ms": round(timed(lambda: slices_and_top(full), reps), 4),
           "query_side_transactions": int(nu * n_j.sum()), "gather_strided_reads": int(nu * m),
           "compact_column_bytes_read": int(m * sweep_slices * nu * 4), "checked_against_old_route": True}
    out.append(rec)
    print(json.dumps(rec), flush=True)
    return rec


def utility_of_every_column(rt, coo, usims, prepared, reps, dev, out):
    import qrlsh
    from qrlsh import predict
    nu, nq = rt.shape

    def new():
        return qrlsh.query_utility(rt, *coo, prepared, None, device=dev)

    def old():
        pt = predict.fill_predictions(rt, *coo, usims, device=dev)
        rated, hit = rt != 0, (rt == 0) & (pt != 0)
        words = torch.stack([rated.sum(0), rt.to(torch.int64).sum(0), hit.sum(0), (pt.to(torch.int64) * hit).sum(0),
                             ((rt == 0) & (pt == 0)).sum(0)], dim=1)
        return words.cpu().numpy()

    if not np.array_equal(new().words[:, :5], old()):
        raise SystemExit("query_utility: the words differ from fill_predictions + torch reductions")
    kern = kernels(new, max(2, reps // 3))
    rec = {"shape": "%dx%d (N1)" % (nu, nq), "m": nq, "what": "query_utility of every column", "kernels_ms": kern,
           "query_utility_call_ms": round(timed(new, max(2, reps // 3)), 4),
           "fill_predictions_plus_reductions_call_ms": round(timed(old, max(2, reps // 3)), 4),
           "checked_against_old_route": True}
    out.append(rec)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="m = 1 and 16 only, no utility sweep")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    import qrlsh  # noqa: F401
    from qrlsh import _lib, predict
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("serve_queries_probe needs a GPU")
    dev = "cuda"
    out = []
    rt, coo, usims, prepared, Ku = inputs(2000, 100_000, 0, dev)
    counts = np.bincount(coo[0].cpu().numpy().astype(np.int64), minlength=rt.shape[1])
    full = predict.fill_predictions(rt, *coo, usims, device=dev)
    rate = {"what": "device-to-device copy", "GBps": round(copy_rate(dev), 1),
            "fill_predictions_call_ms": round(timed(lambda: predict.fill_predictions(rt, *coo, usims, device=dev), 5), 4)}
    out.append(rate)
    print(json.dumps(rate), flush=True)
    cheaper_from = None
    for m in ((1, 16) if a.quick else (1, 16, 256, 4096, 16384, 65536)):
        rec = measure(rt, coo, usims, prepared, full, counts, m, 10, a.reps, dev, out)
        if cheaper_from is None and rec["old_route_call_ms"] <= rec["for_queries_call_ms"]:
            cheaper_from = m
    last = {"full_matrix_cheaper_from_m": cheaper_from}
    out.append(last)
    print(json.dumps(last), flush=True)
    if not a.quick:
        del full
        utility_of_every_column(rt, coo, usims, prepared, a.reps, dev, out)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "serve_queries_probe%s.json" % ("_quick" if a.quick else "")), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
