"""Timing probe of the ranking evaluation on one GPU (qrlsh.evaluate_ranking; qrlsh_evaluate_ranking).

Shape: the N1 shape of bench.py (2000 users x 100 000 queries, 25 % rated, its ratings and list recipes, K = 28 query /
19 user neighbours), as tools/evaluate_probe.py uses it.  Cases: hold-outs of 10 % and 1 %, k = 10 and 100, both
candidate sets, all users and m = 16 requested users.  Every case is first checked, word for word, against the route it
replaces in the same process:

  new     qrlsh.evaluate_ranking(train, truth, lists, user lists, k, relevant, users, candidates): the sweep, the
          selection and the score on the device, 16 integers back;
  before  predict.fill_predictions over the whole train matrix, recommend.top_k over it (for "heldout": over a copy
          with every cell but the test cells zeroed), then torch gathers of truth at the listed columns and reductions.
          That route materialises the (nu, nq) prediction matrix whatever m is.

Then both are timed: the call times, the library's kernels of either route (HIP-event profiler), and the sweep's bytes
(the train row once per slice and request, truth once, the compact rows written once, per predicted cell one rating per
neighbour on either side plus its list entries) against a device-to-device copy of the matrix.

    python tools/rank_eval_probe.py [--quick] [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/rank_eval_probe[_quick].json.
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

from evaluate_probe import inputs, timed, kernels, num  # noqa: E402

SEED = 20
RELEVANT = 60


def before_route(train, truth, coo, usims, users, k, candidates, gain, prefix, dev):
    """-> (per_user int64 [m][8], totals int64 [12]) on the device, by fill_predictions + top_k + torch"""
    from qrlsh import predict, recommend
    pred = predict.fill_predictions(train, *coo, usims, device=dev)
    test = (train == 0) & (truth != 0)
    if candidates == "heldout":
        pred = torch.where(test, pred, torch.zeros_like(pred))
    idx, val, avail = recommend.top_k(train, pred, k, users=users, device=dev)
    rows = torch.arange(train.shape[0], device=dev) if users is None else users.to(torch.int64)
    listed = avail.to(torch.int64).clamp(max=k)
    shown = torch.arange(k, device=dev)[None, :] < listed[:, None]
    tv = truth[rows[:, None], idx.to(torch.int64).clamp(min=0)]
    known = ((tv != 0) & shown).sum(dim=1)
    hit = (tv >= RELEVANT) & shown
    hits = hit.sum(dim=1)
    first = torch.where(hits > 0, hit.to(torch.int64).argmax(dim=1) + 1, torch.zeros_like(hits))
    dcg = (hit.to(torch.int64) * gain[None, :]).sum(dim=1)
    tests = test[rows].sum(dim=1)
    rel = (test[rows] & (truth[rows] >= RELEVANT)).sum(dim=1)
    per = torch.stack([listed, hits, known, first, dcg, rel, tests, avail.to(torch.int64)], dim=1)
    extra = torch.stack([torch.tensor(len(rows), device=dev), (rel > 0).sum(), (hits > 0).sum(),
                         prefix[rel.clamp(max=k)].sum()])
    return per, torch.cat([per.sum(dim=0), extra])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="200 users x 20 000 queries instead of the N1 shape")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import _lib, predict, recommend
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("rank_eval_probe needs a GPU")
    dev = "cuda"
    nu, nq = (200, 20_000) if a.quick else (2000, 100_000)
    rt, coo, usims, prepared, mean_deg, Ku = inputs(nu, nq, 0, dev)
    shape = "%dx%d%s" % (nu, nq, "" if a.quick else " (N1)")
    out = []
    spare = torch.empty_like(rt)
    copy_ms = timed(lambda: spare.copy_(rt), 4 * a.reps)
    del spare
    few = torch.from_numpy(np.random.RandomState(5).choice(nu, size=16, replace=False).astype(np.int32)).to(dev)
    for fraction in (0.1, 0.01):
        train, count = qrlsh.holdout(rt, fraction, seed=SEED, device=dev)
        unrated = int((train == 0).sum().item())
        for users, m in ((None, nu), (few, 16)):
            # the serving call over the same train matrix: what the "all" sweep should sit near
            serve_ms = timed(lambda: recommend.for_users(train, *coo, prepared, users, 10, device=dev), a.reps)
            for k in (10, 100):
                gain = torch.from_numpy(qrlsh.dcg_gains(k)).to(dev)
                prefix = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), gain.cumsum(0)])
                for candidates in ("all", "heldout"):
                    def new():
                        return qrlsh.evaluate_ranking(train, rt, *coo, prepared, k, RELEVANT, users=users,
                                                      candidates=candidates, device=dev)

                    def before():
                        return before_route(train, rt, coo, usims, users, k, candidates, gain, prefix, dev)

                    ev, (per, totals) = new(), before()
                    if not torch.equal(ev.per_user, per) or ev.totals[:12].tolist() != totals.cpu().tolist():
                        raise SystemExit("fraction %g m=%d k=%d %s: evaluate_ranking gives %s, the old route %s"
                                         % (fraction, m, k, candidates, ev.totals[:12].tolist(), totals.cpu().tolist()))
                    kern = kernels(new, a.reps)
                    new_ms = timed(new, a.reps)
                    old_kern = kernels(before, max(2, a.reps // 2))
                    before_ms = timed(before, max(2, a.reps // 2))
                    sweep_label = "rank_sweep_heldout" if candidates == "heldout" else "rank_sweep"
                    sweep = kern.get(sweep_label, 0.0)
                    slices = max(1, min(-(-4096 // m), -(-nq // 1024)))          # rk_sweep_slices of csrc/rankeval.hip
                    share = m / nu
                    predicted = (count if candidates == "heldout" else unrated) * share
                    by = m * nq * 4 * (slices + 2) + predicted * ((mean_deg + Ku) * 4 + mean_deg * 8 + 16)
                    rec = {"shape": shape, "what": "ranking evaluation", "fraction": fraction, "m": m, "k": k,
                           "candidates": candidates, "relevant": RELEVANT, "test_cells": int(ev.totals[6]),
                           "precision": num(ev.precision), "recall": num(ev.recall), "ndcg": num(ev.ndcg),
                           "hit_rate": num(ev.hit_rate), "known_share": num(ev.known_share),
                           "checked_against_before_route": True, "sweep_slices": slices,
                           "cells_predicted": int(predicted), "cells_predicted_before": unrated,
                           "new_kernels_ms": kern, "new_kernels_total_ms": round(sum(kern.values()), 4),
                           "new_call_ms": round(new_ms, 4), "before_call_ms": round(before_ms, 4),
                           "before_library_kernels_ms": old_kern,
                           "before_library_kernels_total_ms": round(sum(old_kern.values()), 4),
                           "before_call_over_new_call": round(before_ms / new_ms, 2),
                           "for_users_k10_call_ms": round(serve_ms, 4),
                           "sweep_algorithmic_bytes": int(by), "device_copy_ms": round(copy_ms, 4),
                           "device_copy_bytes": 2 * nu * nq * 4,
                           "sweep_GBps": round(by / (sweep * 1e-3) / 1e9, 1) if sweep else None,
                           "copy_GBps": round(2 * nu * nq * 4 / (copy_ms * 1e-3) / 1e9, 1)}
                    out.append(rec)
                    print(json.dumps(rec), flush=True)
        del train
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "rank_eval_probe%s.json" % ("_quick" if a.quick else "")), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
