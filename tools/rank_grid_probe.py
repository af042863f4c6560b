"""Timing probe of the ranking grid on one GPU (qrlsh.evaluate_ranking_grid; qrlsh_evaluate_ranking_grid).

Shape: the N1 shape of bench.py (2000 users x 100 000 queries, 25 % rated, its ratings and list recipes, K = 28 query /
19 user neighbours; tools/evaluate_probe.py's inputs).  For hold-outs of 10 % and 1 %, k = 10 and k = 1024, m = 2000 and
m = 16 requests and S = 1, 16 and 128 settings -- as weight triples alone (whole lists) and as 2 x 2 list cuts x S / 4
weight triples -- the grid is evaluated two ways in the same process:

  grid    one qrlsh.evaluate_ranking_grid call: one count pass, one sweep, one rank workgroup per (request, setting);
  calls   the route the library offered before: one qrlsh.evaluate_ranking(candidates="heldout") call per setting, on
          lists cut on the host side of the call (the cut lists are prepared once per cut and not timed).

Every grid is first checked setting for setting against those S calls (the 16 words of each must be equal), then both
are timed: the call times and the library's kernels (HIP-event profiler).

    python tools/rank_grid_probe.py [--quick] [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/rank_grid_probe[_quick].json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

RELEVANT = 60


def main():
    from evaluate_probe import inputs, kernels, num, timed
    from tune_probe import CUTS, SEED, cut_query_lists, cut_user_lists, weight_triples
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="200 users x 20 000 queries instead of the N1 shape")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("rank_grid_probe needs a GPU")
    dev = "cuda"
    nu, nq = (200, 20_000) if a.quick else (2000, 100_000)
    rt, coo, usims, prepared, mean_deg, Ku = inputs(nu, nq, 0, dev)
    shape = "%dx%d%s" % (nu, nq, "" if a.quick else " (N1)")
    q_lists = {c: cut_query_lists(coo, nq, c) for c in CUTS[0]}
    u_lists = {c: cut_user_lists(prepared, c) for c in CUTS[1]}
    few = torch.arange(0, nu, nu // 16, device=dev)[:16]
    out = []
    for fraction in (0.1, 0.01):
        train, count = qrlsh.holdout(rt, fraction, seed=SEED, device=dev)
        for users in (None, few):
            m = nu if users is None else int(users.numel())
            for k in (10, 1024):
                for form, (q_cuts, u_cuts) in (("weights only", ([64], [64])), ("2 x 2 cuts x weights", CUTS)):
                    for S in (1, 16, 128):
                        nw = S // (len(q_cuts) * len(u_cuts))
                        if nw < 1:
                            continue
                        weights = weight_triples(nw)

                        def grid():
                            return qrlsh.evaluate_ranking_grid(train, rt, *coo, prepared, k, RELEVANT, weights,
                                                               q_cuts=q_cuts, u_cuts=u_cuts, users=users, device=dev)

                        def calls():
                            res = []
                            for qc in q_cuts:
                                for uc in u_cuts:
                                    for qw, uw, dm in weights.tolist():
                                        res.append(qrlsh.evaluate_ranking(
                                            train, rt, *q_lists[qc], u_lists[uc], k, RELEVANT, users=users,
                                            candidates="heldout", query_weight=qw, user_weight=uw, default_mean=dm,
                                            device=dev))
                            return res

                        g, each = grid(), calls()
                        flat = g.totals.reshape(-1, 16)
                        for s, ev in enumerate(each):
                            if flat[s].tolist() != ev.totals.tolist():
                                raise SystemExit("fraction %g, m=%d, k=%d, %s, S=%d: setting %d gives %s, its "
                                                 "qrlsh.evaluate_ranking call %s" % (fraction, m, k, form, S, s,
                                                                                     flat[s].tolist(), ev.totals.tolist()))
                        del each
                        reps = a.reps if S < 128 else max(2, a.reps // 2)
                        gk, ck = kernels(grid, a.reps), kernels(calls, reps)
                        grid_ms, calls_ms = timed(grid, a.reps), timed(calls, reps)
                        q, u, w, index = g.best()
                        rec = {"shape": shape, "what": "ranking grid", "fraction": fraction, "requests": m, "k": k,
                               "test_cells": int(flat[0, 6]), "form": form, "settings": S, "q_cuts": q_cuts,
                               "u_cuts": u_cuts, "weight_triples": nw, "checked_setting_for_setting": True,
                               "best": {"index": index, "q_cut": q, "u_cut": u, "weights": list(w),
                                        "ndcg": num(float(g.ndcg.reshape(-1)[index])),
                                        "precision": num(float(g.precision.reshape(-1)[index])),
                                        "recall": num(float(g.recall.reshape(-1)[index]))},
                               "default_ndcg": num(float(g.ndcg[-1, -1, 0])),
                               "grid_kernels_ms": gk, "grid_kernels_total_ms": round(sum(gk.values()), 4),
                               "grid_call_ms": round(grid_ms, 4),
                               "calls_kernels_ms": ck, "calls_kernels_total_ms": round(sum(ck.values()), 4),
                               "calls_ms": round(calls_ms, 4),
                               "calls_over_grid": round(calls_ms / grid_ms, 2),
                               "calls_kernels_over_grid_kernels": round(sum(ck.values()) / sum(gk.values()), 2),
                               "grid_rank_us_per_setting": round(1e3 * gk.get("rank_grid_rank", 0.0) / S, 2)}
                        out.append(rec)
                        print(json.dumps(rec), flush=True)
        del train
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "rank_grid_probe%s.json" % ("_quick" if a.quick else "")), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
