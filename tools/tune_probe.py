"""Timing probe of the grid evaluation on one GPU (qrlsh.evaluate_grid; qrlsh_evaluate_grid).

Shape: the N1 shape of bench.py (2000 users x 100 000 queries, 25 % rated, its ratings and list recipes, K = 28 query /
19 user neighbours; tools/evaluate_probe.py's inputs).  For hold-outs of 10 % and 1 % and for S = 1, 16 and 128 settings
-- as weight triples alone (whole lists) and as 2 x 2 list cuts x S / 4 weight triples -- the grid is evaluated two ways
in the same process:

  grid    one qrlsh.evaluate_grid call: one sweep, S x 8 integers back;
  calls   the route the library offered before: one qrlsh.evaluate call per setting, on lists cut on the host side of
          the call (the cut lists are prepared once per cut and not timed).

Every grid is first checked setting for setting against those S calls (the 8 words of each must be equal), then both are
timed: the call times and the library's kernels (HIP-event profiler).

    python tools/tune_probe.py [--quick] [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/tune_probe[_quick].json.
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

SEED = 20
CUTS = ([14, 64], [10, 64])     # the 2 x 2 form: half of K and the whole list, on either side


def weight_triples(n):
    """n triples around the default: query weight 0.1 .. 0.9, user weight = 1 - query weight, mean 40 .. 75"""
    out = [(0.6, 0.4, 60.0)]
    k = 0
    while len(out) < n:
        qw = (1 + k % 9) / 10.0
        out.append((qw, round(1.0 - qw, 1), 40.0 + 5.0 * ((k // 9) % 8) + 0.5 * (k // 72)))
        k += 1
    return np.array(out[:n], dtype=np.float64)


def cut_query_lists(coo, nq, cut):
    """the first `cut` entries of every list of a COO sorted by source (device tensors)"""
    src, dst, mil = coo
    counts = torch.bincount(src.to(torch.int64), minlength=nq)
    start = torch.cumsum(counts, 0) - counts
    rank = torch.arange(src.numel(), device=src.device) - start[src.to(torch.int64)]
    keep = rank < cut
    return tuple(x[keep].contiguous() for x in (src, dst, mil))


def cut_user_lists(prepared, cut):
    u_idx, u_val, ku = prepared
    u_idx, u_val = u_idx.clone(), u_val.clone()
    u_idx[:, cut:] = -1
    u_val[:, cut:] = 0.0
    return u_idx, u_val, ku


def words8(t):
    t = [int(x) for x in t]
    return [t[0] + t[4] + t[8], t[1] + t[5] + t[9], t[2] + t[6] + t[10], t[3] + t[7] + t[11], t[12], t[13], t[0], t[4]]


def main():
    from evaluate_probe import inputs, kernels, num, timed
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="200 users x 20 000 queries instead of the N1 shape")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("tune_probe needs a GPU")
    dev = "cuda"
    nu, nq = (200, 20_000) if a.quick else (2000, 100_000)
    rt, coo, usims, prepared, mean_deg, Ku = inputs(nu, nq, 0, dev)
    shape = "%dx%d%s" % (nu, nq, "" if a.quick else " (N1)")
    q_lists = {c: cut_query_lists(coo, nq, c) for c in CUTS[0]}
    u_lists = {c: cut_user_lists(prepared, c) for c in CUTS[1]}
    out = []
    for fraction in (0.1, 0.01):
        train, count = qrlsh.holdout(rt, fraction, seed=SEED, device=dev)
        for form, (q_cuts, u_cuts) in (("weights only", ([64], [64])), ("2 x 2 cuts x weights", CUTS)):
            for S in (1, 16, 128):
                nw = S // (len(q_cuts) * len(u_cuts))
                if nw < 1:
                    continue
                weights = weight_triples(nw)

                def grid():
                    return qrlsh.evaluate_grid(train, *coo, prepared, weights, q_cuts=q_cuts, u_cuts=u_cuts, truth=rt,
                                               fraction=fraction, seed=SEED, device=dev)

                def calls():
                    res = []
                    for qc in q_cuts:
                        for uc in u_cuts:
                            for qw, uw, dm in weights.tolist():
                                res.append(qrlsh.evaluate(train, *q_lists[qc], u_lists[uc], truth=rt, fraction=fraction,
                                                          seed=SEED, query_weight=qw, user_weight=uw, default_mean=dm,
                                                          device=dev))
                    return res

                g, each = grid(), calls()
                flat = g.totals.reshape(-1, 8)
                for s, ev in enumerate(each):
                    if flat[s].tolist() != words8(ev.totals):
                        raise SystemExit("fraction %g, %s, S=%d: setting %d gives %s, its qrlsh.evaluate call %s"
                                         % (fraction, form, S, s, flat[s].tolist(), words8(ev.totals)))
                if int(flat[0, 5]) != count:
                    raise SystemExit("fraction %g: %d cells evaluated, %d held out" % (fraction, int(flat[0, 5]), count))
                reps = a.reps if S < 128 else max(2, a.reps // 2)
                gk, ck = kernels(grid, a.reps), kernels(calls, reps)
                grid_ms, calls_ms = timed(grid, a.reps), timed(calls, reps)
                q, u, w, index = g.best()
                rec = {"shape": shape, "what": "grid evaluation", "fraction": fraction, "cells_evaluated": count,
                       "form": form, "settings": S, "q_cuts": q_cuts, "u_cuts": u_cuts, "weight_triples": nw,
                       "checked_setting_for_setting": True,
                       "best": {"index": index, "q_cut": q, "u_cut": u, "weights": list(w),
                                "rmse": num(float(g.rmse.reshape(-1)[index])),
                                "coverage": num(float(g.coverage.reshape(-1)[index]))},
                       "default_rmse": num(float(g.rmse[-1, -1, 0])),
                       "grid_kernels_ms": gk, "grid_kernels_total_ms": round(sum(gk.values()), 4),
                       "grid_call_ms": round(grid_ms, 4),
                       "calls_kernels_ms": ck, "calls_kernels_total_ms": round(sum(ck.values()), 4),
                       "calls_ms": round(calls_ms, 4),
                       "calls_over_grid": round(calls_ms / grid_ms, 2),
                       "calls_kernels_over_grid_kernels": round(sum(ck.values()) / sum(gk.values()), 2),
                       "grid_sweep_us_per_setting": round(1e3 * gk.get("evaluate_grid", 0.0) / S, 2)}
                out.append(rec)
                print(json.dumps(rec), flush=True)
        del train
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "tune_probe%s.json" % ("_quick" if a.quick else "")), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
