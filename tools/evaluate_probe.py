"""Timing probe of the evaluation on one GPU (qrlsh.holdout / qrlsh.evaluate; qrlsh_ratings_holdout, qrlsh_evaluate).

Shape: the N1 shape of bench.py (2000 users x 100 000 queries, 25 % rated, its ratings and list recipes, K = 28 query /
19 user neighbours).  For the fractions 1, 0.1 and 0.01 a hold-out split is made on the device and evaluated two ways in
the same process (at fraction 1 the train matrix is empty and every cell is missed: a check, not a workload; the
leave-one-out sweep over the same sample, predicted from the full matrix, is timed beside each):

  new     qrlsh.evaluate(train, lists, user lists, truth=ratings, fraction, seed): one sweep, 16 integers back;
  before  the route the library offered for a hold-out before it had one: predict.fill_predictions over the whole train
          matrix, then torch's masked gather of the held-out cells and reductions of pred - truth (the mask itself --
          which that route would also have to make -- is handed to it ready-made and not timed).

Each fraction's result is first checked against the `before` route (cells, missed, sum err, sum |err|, sum err^2 must be
equal), then both are timed: the call times, the library's kernels (HIP-event profiler) and, for the `before` route, its
fill_predictions kernels alone (a lower bound of that route).  The hold-out copy is timed against a device-to-device
copy of the same matrix.  Bytes: the copy reads and writes the matrix once; the sweep reads `truth` once, the user's row
once per column slice, and per evaluated cell one rating per neighbour on either side plus its list entries.

    python tools/evaluate_probe.py [--quick] [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/evaluate_probe[_quick].json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
SEED = 20


def inputs(nu, nq, seed, dev):
    """bench.py's N1 recipe: ratings 1..100 with 75 % unrated, 0..K query neighbours (milli values sorted descending
    over the whole array), K_u random user neighbours with similarities rounded to 3 decimals"""
    from qrlsh import pipeline, predict
    rng = np.random.RandomState(seed)
    Kq, Ku = pipeline.max_candidates(nq), pipeline.max_candidates(nu)
    ratings = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    for r0 in range(0, nu, 250):
        ratings[r0:r0 + 250][rng.rand(min(250, nu - r0), nq) < 0.75] = 0
    deg = rng.randint(0, Kq + 1, size=nq)
    q_src = np.repeat(np.arange(nq, dtype=np.int32), deg)
    q_dst = rng.randint(0, nq, size=q_src.size).astype(np.int32)
    q_mil = np.sort(rng.randint(0, 1001, size=q_src.size).astype(np.int32))[::-1].copy()
    usims = {u: {"indexes": rng.randint(0, nu, size=Ku), "values": np.round(rng.rand(Ku), 3)} for u in range(nu)}
    rt = torch.from_numpy(ratings).to(dev)
    coo = tuple(torch.from_numpy(x).to(dev) for x in (q_src, q_dst, q_mil))
    return rt, coo, usims, predict.user_lists(usims, nu, dev), float(deg.mean()), Ku


def num(x, digits=4):
    """a float for JSON: None where nothing was covered (nan)"""
    return None if x != x else round(x, digits)


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps):
    from qrlsh import _lib
    _lib.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rep = _lib.prof_report()
    _lib.prof_enable(False)
    return {lab: round(ms / reps, 4) for lab, (cnt, ms) in sorted(rep.items())}


def before_route(train, truth, mask, coo, usims, dev):
    """-> [covered, sum err, sum |err|, sum err^2, missed, cells] as Python integers"""
    from qrlsh import predict
    pred = predict.fill_predictions(train, *coo, usims, device=dev)
    p, t = pred[mask].to(torch.int64), truth[mask].to(torch.int64)
    hit = p != 0
    e = torch.where(hit, p - t, torch.zeros_like(p))
    back = torch.stack([hit.sum(), e.sum(), e.abs().sum(), (e * e).sum(), (~hit).sum()]).cpu().tolist()
    return [int(x) for x in back] + [int(p.numel())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="200 users x 20 000 queries instead of the N1 shape")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import _lib, predict
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_probe needs a GPU")
    dev = "cuda"
    nu, nq = (200, 20_000) if a.quick else (2000, 100_000)
    rt, coo, usims, prepared, mean_deg, Ku = inputs(nu, nq, 0, dev)
    shape = "%dx%d%s" % (nu, nq, "" if a.quick else " (N1)")
    out = []

    # the hold-out copy against a device-to-device copy
    spare = torch.empty_like(rt)
    kern = kernels(lambda: qrlsh.holdout(rt, 0.1, seed=SEED, device=dev), a.reps)
    by = 2 * nu * nq * 4
    # the library call alone (count memset + kernel, no allocation, no read-back), back to back like the copies
    from qrlsh.ops import _ptr, _stream
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    keep = int(round(0.1 * 2.0**32))
    lib = _lib.load()
    abi_ms = timed(lambda: _lib.check(lib.qrlsh_ratings_holdout(_ptr(rt), nu, nq, SEED, keep, _ptr(spare), _ptr(count),
                                                                _stream())), 4 * a.reps)
    copy_ms = timed(lambda: spare.copy_(rt), 4 * a.reps)
    rec = {"shape": shape, "what": "hold-out copy, fraction 0.1", "ratings_holdout_kernel_ms": kern.get("ratings_holdout"),
           "library_call_ms": round(abi_ms, 4),
           "holdout_call_ms": round(timed(lambda: qrlsh.holdout(rt, 0.1, seed=SEED, device=dev), a.reps), 4),
           "device_copy_ms": round(copy_ms, 4), "bytes": by,
           "library_call_GBps": round(by / (abi_ms * 1e-3) / 1e9, 1),
           "copy_GBps": round(by / (copy_ms * 1e-3) / 1e9, 1),
           "library_call_over_copy": round(abi_ms / copy_ms, 3)}
    del spare
    out.append(rec)
    print(json.dumps(rec), flush=True)

    slices = max(1, min(-(-4096 // nu), -(-nq // 1024)))     # ev_slices of csrc/evaluate.hip
    for fraction in (1.0, 0.1, 0.01):
        train, count = qrlsh.holdout(rt, fraction, seed=SEED, device=dev)
        mask = (train == 0) & (rt != 0)

        def new():
            return qrlsh.evaluate(train, *coo, prepared, truth=rt, fraction=fraction, seed=SEED, device=dev)

        def before():
            return before_route(train, rt, mask, coo, usims, dev)

        ev, want = new(), before()
        t = [int(x) for x in ev.totals]
        got = [t[0] + t[4] + t[8], t[1] + t[5] + t[9], t[2] + t[6] + t[10], t[3] + t[7] + t[11], t[12], t[13]]
        if got != want or ev.n != count:
            raise SystemExit("fraction %g: the sweep gives %s, fill_predictions + torch %s (held out: %d)"
                             % (fraction, got, want, count))
        kern = kernels(new, a.reps)
        new_ms = timed(new, a.reps)

        def loo():      # the same sample, predicted from the full matrix: leave-one-out, the lists held fixed
            return qrlsh.evaluate(rt, *coo, prepared, fraction=fraction, seed=SEED, device=dev)

        lev = loo()
        if lev.n != count:
            raise SystemExit("fraction %g: leave-one-out evaluates %d cells, the hold-out %d" % (fraction, lev.n, count))
        loo_sweep = kernels(loo, a.reps).get("evaluate", 0.0)
        loo_ms = timed(loo, a.reps)
        fill = kernels(lambda: predict.fill_predictions(train, *coo, usims, device=dev), max(2, a.reps // 2))
        before_ms = timed(before, max(2, a.reps // 2))
        by = nu * nq * 4 + nu * slices * nq * 4 + count * ((mean_deg + Ku) * 4 + mean_deg * 8 + 16)
        sweep = kern.get("evaluate", 0.0)
        rec = {"shape": shape, "what": "hold-out evaluation", "fraction": fraction, "cells_evaluated": count,
               "rmse": num(ev.rmse), "mae": num(ev.mae), "coverage": num(ev.coverage),
               "checked_against_before_route": True, "sweep_slices": slices,
               "new_kernels_ms": kern, "new_kernels_total_ms": round(sum(kern.values()), 4), "new_call_ms": round(new_ms, 4),
               "before_call_ms": round(before_ms, 4), "before_fill_predictions_kernels_ms": round(sum(fill.values()), 4),
               "before_call_over_new_call": round(before_ms / new_ms, 2),
               "before_kernels_over_new_call": round(sum(fill.values()) / new_ms, 2),
               "algorithmic_bytes": int(by), "sweep_GBps": round(by / (sweep * 1e-3) / 1e9, 1) if sweep else None,
               "sweep_hbm_peak_fraction": round(by / HBM_PEAK / (sweep * 1e-3), 4) if sweep else None,
               "sweep_cells_per_s": round(count / (sweep * 1e-3), 1) if sweep else None,
               "leave_one_out": {"rmse": num(lev.rmse), "mae": num(lev.mae), "coverage": num(lev.coverage),
                                 "sweep_kernel_ms": loo_sweep, "call_ms": round(loo_ms, 4),
                                 "sweep_GBps": round(by / (loo_sweep * 1e-3) / 1e9, 1) if loo_sweep else None,
                                 "sweep_cells_per_s": round(count / (loo_sweep * 1e-3), 1) if loo_sweep else None}}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del train, mask
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "evaluate_probe%s.json" % ("_quick" if a.quick else "")), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
