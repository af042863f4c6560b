"""Timing probe of serving new queries (qrlsh.QueryIndex: csrc/index.hip, qrlsh_predict_columns) on one GPU.

Shapes:
  * index build at configs[2] (10 M queries x 128 / 32 bands, D = 32768, bench.py's synthetic recipe), on the hot
    path's own band keys and compact signature rows;
  * probe batches of 1, 64, 1024 and 16 384 new queries against it: perturbed copies of indexed answer sets (one row
    id replaced), so that lists are non-trivial;
  * column prediction and top users for 1024 new queries at the N1 shape (2000 users x 100 000 queries, bench.py's
    ratings recipe, lists of K = 28).
Every shape is first checked against the restatement (tests/query_index_cases.py, oracle.predict_cells) on a sample;
then per-kernel times from the library's HIP-event profiler, the call time, the algorithmic bytes and the fraction of
the 8 TB/s HBM peak.

    python tools/query_index_probe.py [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/query_index_probe.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, reps):
    """(call ms, {kernel label: ms per call}) of fn()"""
    from qrlsh import _lib
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    call_ms = e0.elapsed_time(e1) / reps
    _lib.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rep = _lib.prof_report()
    _lib.prof_enable(False)
    return call_ms, {lab: round(ms / reps, 4) for lab, (cnt, ms) in sorted(rep.items())}


def emit(out, rec, by, kern):
    kms = sum(kern.values())
    rec.update({"kernels_ms": kern, "kernels_total_ms": round(kms, 4), "algorithmic_bytes": int(by),
                "GBps": round(by / (kms * 1e-3) / 1e9, 1) if kms else None,
                "hbm_peak_fraction": round(by / HBM_PEAK / (kms * 1e-3), 3) if kms else None})
    out.append(rec)
    print(json.dumps(rec), flush=True)


def check_probe(qi, sig_dev, xs, K, sample):
    """the device lists of `sample` probes equal the restatement (candidates by band equality on the device, scores
    and order in numpy)"""
    import query_index_cases as QC
    from qrlsh import ops
    off, idx, milli, avail = (t.cpu().numpy() for t in qi.neighbours(xs, K=K))
    b, r = qi.b, qi.r
    I16 = ops.sig_to_int32(sig_dev).bitwise_and(0xFFFF).view(qi.n, b, r)
    x32 = ops.sig_to_int32(xs)
    for q in sample:
        X = x32[q].bitwise_and(0xFFFF).view(b, r)
        live = ~(X == 0xFFFF).all(dim=1)
        ids = torch.nonzero(((I16 == X[None]).all(dim=2) & live[None]).any(dim=1)).flatten().cpu().numpy()
        rows = ops.sig_to_int32(sig_dev[torch.from_numpy(ids).to(sig_dev.device)]).cpu().numpy()
        mi = QC.restate_scores(rows, np.arange(len(ids)), x32[q].cpu().numpy())
        order = np.lexsort((ids, -mi))[:K]
        lo, hi = off[q], off[q + 1]
        if avail[q] != len(ids) or not np.array_equal(idx[lo:hi], ids[order]) or not np.array_equal(milli[lo:hi], mi[order]):
            raise SystemExit("probe %d differs from the restatement" % q)


def perturbed_sets(offsets, rows, picks, D, rng):
    """CSR answer sets of the picked indexed queries with one row id replaced by a random one"""
    off_h = offsets.cpu().numpy()
    segs = []
    for q in picks:
        s = rows[off_h[q]:off_h[q + 1]].cpu().numpy().copy()
        if len(s):
            s[rng.integers(len(s))] = rng.integers(D)
        segs.append(np.unique(s).astype(np.int32))
    o = np.concatenate(([0], np.cumsum([len(s) for s in segs]))).astype(np.int64)
    return torch.from_numpy(o).cuda(), torch.from_numpy(np.concatenate(segs)).cuda()


def index_shapes(reps, out):
    from qrlsh import ops, pipeline, synth
    from qrlsh.index import QueryIndex
    nq, D, P, b = 10_000_000, 32768, 128, 32
    offsets, rows = synth.synth_csr(nq, D, seed=0)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42))
    K = pipeline.max_candidates(nq)
    sig, norm2, keys = ops.minhash(offsets, rows, table, b=b, want_norm=True, compact=True, validate=False)
    keep = keys.clone()
    qi = QueryIndex(sig, norm2, b, table=table, keys=keys, K=K)
    work = [keep.clone()]

    def build():
        ops.index_build(work[0])
        work[0].copy_(keep)
    call_ms, kern = timed(build, reps)
    kern = {k: v for k, v in kern.items() if k not in ("",)}
    n = nq * b
    # radix sort: 4 passes of (key, id) read + written and a histogram read; directory: keys once + words written
    by = 4 * (2 * n * 12 + n * 8) + n * 8 + ops._lib.load().qrlsh_index_dir_words(nq, b) * 4
    emit(out, {"shape": "index build 10M x 128/32", "call_ms_incl_key_restore_copy": round(call_ms, 4)}, by, kern)
    del keep, work
    rng = np.random.default_rng(3)
    for m in (1, 64, 1024, 16384):
        picks = rng.choice(nq, m, replace=False)
        po, pr = perturbed_sets(offsets, rows, picks, D, rng)
        xs, xn, xk = qi.signatures(po, pr)
        check_probe(qi, sig, xs, K, range(min(m, 4)))
        raw, _ = ops.index_probe(qi.keys, qi.ids, qi.dir, qi.r, xk)
        n_raw = raw.numel()
        call_ms, kern = timed(lambda: qi.neighbours(xs, xn, xk), reps)
        # probe: key + 2 directory words + ~4 run keys per (query, band), twice; score: raw word, both rows, key out;
        # select / compact: keys in, K outputs
        by = 2 * m * b * (8 + 8 + 4 * 8) + n_raw * (8 + 2 * P * 2 + 8) + n_raw * 8 + m * K * 16
        emit(out, {"shape": "probe m=%d (K=%d)" % (m, K), "raw_words": int(n_raw), "call_ms": round(call_ms, 4),
                   "checked_against_restatement": True}, by, kern)


def column_shapes(reps, out):
    import predict_cases as PC  # noqa: F401  (tests on the path)
    from oracle import oracle as O
    from qrlsh.index import QueryIndex
    rng = np.random.RandomState(0)
    nu, nqq, m, K = 2000, 100_000, 1024, 28
    ratings = rng.randint(1, 101, size=(nu, nqq)).astype(np.int32)      # bench.py's N1 recipe
    ratings[rng.rand(nu, nqq) < 0.75] = 0
    deg = rng.randint(1, K + 1, size=m)
    off = np.concatenate(([0], np.cumsum(deg))).astype(np.int64)
    idx = rng.randint(0, nqq, size=off[-1]).astype(np.int32)
    mil = rng.randint(0, 1001, size=off[-1]).astype(np.int32)
    qi = QueryIndex.__new__(QueryIndex)
    qi.n, qi.sig = nqq, torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    rt = torch.from_numpy(ratings).cuda()
    t = [torch.from_numpy(a).cuda() for a in (off, idx, mil)]
    cols = qi.predict_columns(rt, *t)
    got = cols.cpu().numpy()
    srng = np.random.default_rng(5)
    for x in srng.choice(m, 8, replace=False):
        lst = {nqq: {"indexes": idx[off[x]:off[x + 1]], "values": mil[off[x]:off[x + 1]] / 1000.0}}
        us = srng.choice(nu, 64, replace=False)
        app = np.hstack([ratings[us], np.zeros((64, 1), dtype=np.int32)])
        usr = {u: {"indexes": np.zeros(0, dtype=np.int64), "values": np.zeros(0)} for u in range(64)}
        want = O.predict_cells(app, lst, usr, np.array([(u, nqq) for u in range(64)]))
        if not np.array_equal(got[x, us], want):
            raise SystemExit("predict_columns differs from oracle.predict_cells")
    call_ms, kern = timed(lambda: qi.predict_columns(rt, *t), reps)
    by = off[-1] * 8 + int(off[-1]) * nu * 4 + m * nu * 4      # lists, one rating gather per (entry, user), output
    emit(out, {"shape": "predict_columns m=1024 x 2000 users (N1)", "call_ms": round(call_ms, 4),
               "checked_against_oracle": True}, by, kern)
    from test_recommend_host import restate
    u, v, a = (x.cpu().numpy() for x in QueryIndex.top_users(cols, 10))
    wi, wv, wa = restate(np.zeros_like(got), got, 10)
    if not (np.array_equal(u, wi) and np.array_equal(v, wv) and np.array_equal(a, wa)):
        raise SystemExit("top_users differs from the restatement")
    call_ms, kern = timed(lambda: QueryIndex.top_users(cols, 10), reps)
    by = 2 * m * nu * 4 + m * 10 * 8 + m * 4
    emit(out, {"shape": "top_users m=1024 x 2000 users, k=10", "call_ms_incl_zero_matrix": round(call_ms, 4),
               "checked_against_restatement": True}, by, kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    from qrlsh import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("query_index_probe needs a GPU")
    out = []
    t0 = time.time()
    column_shapes(a.reps, out)
    torch.cuda.empty_cache()
    index_shapes(a.reps, out)
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "query_index_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
