"""Timing probe of the live user lists' row operations (qrlsh.UserLists.add_users / remove_users / nearest,
csrc/userrows.hip) on one GPU.

Shape: bench.py's N4 matrix, 2000 users x 100 000 queries (ratings 1 .. 100, 75 % unrated), K = 19, under two
labellings: 333 random clusters (6 users each) and bench.py's 40 (50 users each).  Batches of 1, 16 and 256 users:
appended with labels given (those of random existing users), appended with labels=None (the assignment by the nearest
existing user), and removed.  A new user is an existing one's row with a fifth of its ratings dropped, so that the
assignment finds somebody.  Every batch is first checked in this process: lists, matrix, row statistics and labels
against a fresh UserLists.build over the new matrix.  Then, in the same process,
  (a) the call time of the operation (a shallow copy of the state per call: a row operation binds new tensors and
      leaves the old ones) and its per-kernel times (the library's HIP-event profiler), against the rebuild it replaces:
      the upload of the new host matrix plus UserLists.build with the same labels;
  (b) for the appends, qrlsh_user_rows_nearest against qrlsh_user_pairs_score over the same m x nu pairs (equal scores
      checked first);
  (c) the move kernel against a device-to-device copy_ of the same matrix -- the byte floor;
  and for the removals what the pairs of the removed rows cost, which the update scores for nothing.

    python tools/user_rows_probe.py [--reps N] [--out DIR] [--budget SECONDS]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/user_rows_probe.json (rewritten after
every result).  --budget: no new batch is started once that many seconds have passed.
"""
import argparse
import copy
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

from user_columns_probe import event_ms  # noqa: E402

CHECKED = ("idx", "milli", "len", "mean", "norm2", "ratings")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nu", type=int, default=2000)
    ap.add_argument("--nq", type=int, default=100_000)
    ap.add_argument("--counts", default="1,16,256")
    ap.add_argument("--budget", type=float, default=1e9)
    a = ap.parse_args()
    from qrlsh import _lib, users, userlists
    from qrlsh.userlists import UserLists
    if not torch.cuda.is_available():
        raise SystemExit("user_rows_probe needs a GPU")
    t0 = time.time()
    nu, nq = a.nu, a.nq
    rng = np.random.RandomState(4)
    ratings = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    ratings[rng.rand(nu, nq) < 0.75] = 0
    K = users.max_candidates(nu)
    out = []

    def save():
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "user_rows_probe.json"), "w") as fh:
                json.dump(out, fh, indent=1)

    base = torch.from_numpy(ratings).cuda()
    for nc in (max(1, nu // 6), 40):
        labels = rng.randint(0, nc, size=nu).astype(np.int64)
        ul = UserLists.build(base, labels, K=K, device="cuda")
        for kind in ("add with labels", "add, labels=None", "remove"):
            for m in (int(x) for x in a.counts.split(",")):
                if time.time() - t0 > a.budget:
                    continue
                er = np.random.default_rng(100 * nc + m + len(kind))
                who = np.sort(er.choice(nu, size=m, replace=False))
                extra = {}
                if kind == "remove":
                    keep = np.ones(nu, dtype=bool)
                    keep[who] = False
                    host = ratings[keep]
                    op = lambda w: w.remove_users(who)
                else:
                    rows = ratings[who] * (er.random((m, nq)) < 0.8)
                    rd = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
                    host = np.vstack((ratings, rows)).astype(np.int32)
                    given = labels[who] if kind == "add with labels" else None
                    op = lambda w: w.add_users(rd, labels=given)
                w = copy.copy(ul)
                op(w)
                picked = w.last_picked
                fresh = UserLists.build(host, w.user_labels(), K=K, device="cuda")
                for name in CHECKED:
                    if not torch.equal(getattr(w, name), getattr(fresh, name)):
                        raise SystemExit("clusters=%d %s %d: %s differs from the fresh build" % (nc, kind, m, name))
                if not torch.equal(base, torch.from_numpy(ratings).cuda()):
                    raise SystemExit("the matrix given to build was changed")
                all_labels = w.user_labels()
                if kind == "add with labels" and not np.array_equal(all_labels[nu:], given):
                    raise SystemExit("the labels given were not kept")
                if kind == "add, labels=None":
                    extra["joined_an_existing_cluster"] = int(np.isin(all_labels[nu:], labels).sum())
                del fresh
                call_ms = event_ms(op, a.reps, before=lambda: copy.copy(ul))
                _lib.prof_enable(True)
                for _ in range(a.reps):
                    op(copy.copy(ul))
                torch.cuda.synchronize()
                kern = {lab: round(ms / a.reps, 4) for lab, (cnt, ms) in sorted(_lib.prof_report().items())}
                _lib.prof_enable(False)
                rebuild_ms = event_ms(lambda: UserLists.build(host, all_labels, K=K, device="cuda"), max(1, a.reps - 1))
                dst = torch.empty_like(w.ratings)
                dst.copy_(w.ratings)
                copy_ms = event_ms(lambda: dst.copy_(w.ratings), 2 * a.reps)
                by = 2 * w.ratings.numel() * 4
                move_ms = kern.get("ratings_rows_move", 0.0)
                if kind == "remove":
                    # the pairs (removed row, every other member of its cluster): scored by the update, all 0
                    pr = np.concatenate([(int(g) << 32) | np.flatnonzero((labels == labels[g]) & (np.arange(nu) != g))
                                         for g in who] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
                    extra["wasted_pairs"] = int(pr.size)
                    if pr.size:
                        pd = torch.from_numpy(pr).cuda()
                        extra["wasted_pairs_score_ms"] = round(event_ms(
                            lambda: userlists.pairs_score(ul.ratings, ul.mean, ul.norm2, pd), a.reps), 4)
                else:
                    # (b) the m x nu scores: the new kernel against the pair kernel over the stacked matrix
                    got = ul._nearest(rd, m, want_all=True)[2]
                    pr = ((nu + np.arange(m, dtype=np.int64))[:, None] << 32 | np.arange(nu, dtype=np.int64)[None, :]).reshape(-1)
                    pd = torch.from_numpy(pr).cuda()
                    ref = userlists.pairs_score(w.ratings, w.mean, w.norm2, pd).reshape(m, nu)
                    if not torch.equal(got, ref):
                        raise SystemExit("clusters=%d %s %d: rows_nearest and pairs_score differ" % (nc, kind, m))
                    _lib.prof_enable(True)
                    for _ in range(a.reps):
                        ul._nearest(rd, m)
                    torch.cuda.synchronize()
                    nk = _lib.prof_report()
                    _lib.prof_enable(False)
                    near_ms = sum(nk[k][1] for k in ("user_rows_nearest", "user_rows_nearest_finish")) / a.reps
                    pair_ms = event_ms(lambda: userlists.pairs_score(w.ratings, w.mean, w.norm2, pd), a.reps)
                    extra.update({"nearest_pairs": int(pr.size), "rows_nearest_kernels_ms": round(near_ms, 4),
                                  "pairs_score_same_pairs_ms": round(pair_ms, 4),
                                  "pairs_score_over_rows_nearest": round(pair_ms / near_ms, 2)})
                    del got, ref, pd
                rec = {"shape": "%d users x %d queries, %d clusters, K=%d, %s, %d users" % (nu, nq, nc, K, kind, m),
                       "date": datetime.date.today().isoformat(), "nu": nu, "nq": nq, "clusters": nc, "K": K,
                       "operation": kind, "users": m, "picked_rows": int(picked),
                       "checked_against_fresh_build_same_process": True,
                       "call_ms": round(call_ms, 3), "kernels_ms": kern, "kernels_total_ms": round(sum(kern.values()), 3),
                       "upload_plus_build_ms": round(rebuild_ms, 2), "rebuild_over_call": round(rebuild_ms / call_ms, 2),
                       "move_kernel_ms": move_ms, "copy_ms": round(copy_ms, 4), "matrix_bytes_read_plus_written": by,
                       "move_GBps": round(by / (move_ms * 1e-3) / 1e9, 1) if move_ms else None,
                       "copy_GBps": round(by / (copy_ms * 1e-3) / 1e9, 1),
                       "move_rate_over_copy_rate": round(copy_ms / move_ms, 3) if move_ms else None}
                rec.update(extra)
                out.append(rec)
                print(json.dumps(rec), flush=True)
                save()
                del w, dst, host
                torch.cuda.empty_cache()
        del ul
    print("total %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
