"""Timing probe of the live user lists (qrlsh.UserLists.rate, csrc/userlists.hip) on one GPU.

Shape: bench.py's N4 matrix, 2000 users x 100 000 queries (ratings 1 .. 100, 75 % unrated), K = 19, under two
labellings: bench.py's 40 random clusters (50 users each) and 333 random clusters (6 users each, the size the
reference's clustering gives at 2000 users).  Batches of edits that touch 1, 16 and 256 distinct users (3 cells each).
Every batch is first checked in this process: after rate() the lists, the matrix and the row statistics equal a fresh
UserLists.build over the edited matrix (users.user_similarities: the full recompute).  Then, in the same process,
  * the call time of rate() and its per-kernel times (the library's HIP-event profiler); a timed call alternates
    between the batch and the batch that restores the old values, so every call changes the matrix;
  * the call time of users.user_similarities over the same matrix (what stood in for it);
  * the new pair kernel against center_rows + row_norms + score_pairs over the pairs of the batch's changed rows;
  * the pair kernel's algorithmic bytes (every pair streams its second row once; the first row is read once per tile
    of 8 pairs) against the 8 TB/s HBM peak.

    python tools/user_lists_probe.py [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/user_lists_probe.json.
"""
import argparse
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

from query_index_probe import HBM_PEAK, timed  # noqa: E402

UPDATE = ("ratings_set", "user_rows_stats", "idmap_mark", "idmap_popc", "idmap_pack", "idmap_list", "scan_blocks",
          "user_lists_mark", "user_cluster_pairs_count", "user_cluster_pairs_fill", "user_pairs_score",
          "user_pairs_finish", "user_lists_apply")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nu", type=int, default=2000)
    ap.add_argument("--nq", type=int, default=100_000)
    ap.add_argument("--touched", default="1,16,256")
    a = ap.parse_args()
    from qrlsh import ops, users, userlists
    from qrlsh.userlists import UserLists
    if not torch.cuda.is_available():
        raise SystemExit("user_lists_probe needs a GPU")
    t0 = time.time()
    reps = a.reps + a.reps % 2
    nu, nq = a.nu, a.nq
    rng = np.random.RandomState(4)
    ratings = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    ratings[rng.rand(nu, nq) < 0.75] = 0
    K = users.max_candidates(nu)
    out = []
    for nc in (40, max(1, nu // 6)):
        labels = rng.randint(0, nc, size=nu).astype(np.int64)
        base = torch.from_numpy(ratings).cuda()
        ul = UserLists.build(base, labels, K=K, device="cuda")
        full_ms, full_kern = timed(lambda: users.user_similarities(ul.ratings, labels, K, "cuda"), a.reps)
        for t in (int(x) for x in a.touched.split(",")):
            er = np.random.default_rng(1000 * nc + t)
            who = np.repeat(er.choice(nu, size=t, replace=False), 3)
            cols = np.concatenate([er.choice(nq, size=3, replace=False) for _ in range(t)])
            vals = er.integers(0, 101, size=who.size)
            old = ul.ratings[torch.from_numpy(who).cuda(), torch.from_numpy(cols).cuda()].cpu().numpy()
            rows = ul.rate(who, cols, vals)
            picked = ul.last_picked
            fresh = UserLists.build(ul.ratings.clone(), labels, K=K, device="cuda")
            for name in ("idx", "milli", "len", "mean", "norm2", "ratings"):
                if not torch.equal(getattr(ul, name), getattr(fresh, name)):
                    raise SystemExit("clusters=%d touched=%d: %s differs from the full recompute" % (nc, t, name))
            del fresh
            turn = [0]

            def rate():
                turn[0] ^= 1
                ul.rate(who, cols, old if turn[0] else vals)
            call_ms, kern = timed(rate, reps)       # 2 * reps + 1 calls: the matrix ends with its old values again
            # the pairs of the changed rows, scored by both routes
            R = np.unique(who)
            pairs = np.array([(int(r) << 32) | int(v) for r in R for v in np.flatnonzero(labels == labels[r]) if v != r],
                             dtype=np.int64)
            pd = torch.from_numpy(pairs).cuda()
            new_ms, new_kern = timed(lambda: userlists.pairs_score(ul.ratings, ul.mean, ul.norm2, pd), a.reps)

            def old_route():
                c = users.center_rows(ul.ratings)
                return ops.score_pairs(c, ops.row_norms(c), pd)[0]
            old_ms, old_kern = timed(old_route, a.reps)
            if not torch.equal(old_route(), userlists.pairs_score(ul.ratings, ul.mean, ul.norm2, pd)):
                raise SystemExit("clusters=%d touched=%d: the pair kernel differs from the old route" % (nc, t))
            tiles = (pairs.size + 7) // 8
            by = (pairs.size + tiles) * nq * 4
            score_ms = new_kern.get("user_pairs_score", 0.0)
            rec = {"shape": "%d users x %d queries, %d clusters, K=%d, %d users touched" % (nu, nq, nc, K, t),
                   "date": datetime.date.today().isoformat(), "nu": nu, "nq": nq, "clusters": nc, "K": K, "touched_users": t,
                   "cells": int(who.size), "rows_rewritten": int(rows), "picked_rows": int(picked),
                   "checked_against_full_recompute_same_process": True,
                   "rate": {"call_ms": round(call_ms, 4), "kernels_ms": {k: v for k, v in kern.items() if k in UPDATE},
                            "kernels_total_ms": round(sum(v for k, v in kern.items() if k in UPDATE), 4)},
                   "full_user_similarities": {"call_ms": round(full_ms, 4), "kernels_total_ms": round(sum(full_kern.values()), 4)},
                   "full_over_rate_call": round(full_ms / call_ms, 2),
                   "pairs_of_changed_rows": int(pairs.size),
                   "pair_kernel": {"call_ms": round(new_ms, 4), "kernels_ms": new_kern, "algorithmic_bytes": int(by),
                                   "algorithmic_GBps": round(by / (score_ms * 1e-3) / 1e9, 1) if score_ms else None,
                                   "hbm_peak_fraction": round(by / HBM_PEAK / (score_ms * 1e-3), 3) if score_ms else None},
                   "center_rows_row_norms_score_pairs": {"call_ms": round(old_ms, 4), "kernels_ms": old_kern},
                   "old_route_over_pair_kernel_call": round(old_ms / new_ms, 2),
                   "score_pairs_alone_over_pair_kernel": round(old_kern.get("score_pairs", 0.0) / (score_ms + new_kern.get(
                       "user_pairs_finish", 0.0)), 2) if score_ms else None}
            out.append(rec)
            print(json.dumps(rec), flush=True)
        del ul, base
        torch.cuda.empty_cache()
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "user_lists_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
