"""Timing probe of the live user lists' column operations (qrlsh.UserLists.add_columns / remove_columns / set_columns,
csrc/usercolumns.hip) on one GPU.

Shape: bench.py's N4 matrix, 2000 users x 100 000 queries (ratings 1 .. 100, 75 % unrated), K = 19, under two
labellings: 333 random clusters (6 users each) and bench.py's 40 (50 users each).  Batches of 1, 16 and 256 columns:
appended with 1 % and with 25 % of the users rating each; removed (existing columns: 25 % rated); overwritten with the
old column in which 1 % / 25 % of the users get another value.  Every batch is first checked in this process: the
matrix against torch indexing on the device, then lists, matrix and row statistics against a fresh UserLists.build
over it.  Then, in the same process,
  * the call time of the operation (a fresh shallow state per call: the operation is out of place, so the old matrix
    is shared) and its per-kernel times (the library's HIP-event profiler);
  * the rebuild it replaces: the upload of the new host matrix plus UserLists.build with the same labels;
  * for the move kernel alone, a device-to-device copy_ of the same matrix -- the byte floor.

    python tools/user_columns_probe.py [--reps N] [--out DIR] [--budget SECONDS]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/user_columns_probe.json (rewritten after
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

SMALL = ("idx", "milli", "len", "mean", "norm2")


def fork(ul):
    """a state the operation may change: the small tensors cloned, the matrix shared (column operations leave it)"""
    w = copy.copy(ul)
    for k in SMALL:
        setattr(w, k, getattr(ul, k).clone())
    return w


def event_ms(fn, reps, before=None):
    tot = 0.0
    for _ in range(reps):
        arg = before() if before else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(arg) if before else fn()
        e1.record()
        torch.cuda.synchronize()
        tot += e0.elapsed_time(e1)
    return tot / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nu", type=int, default=2000)
    ap.add_argument("--nq", type=int, default=100_000)
    ap.add_argument("--counts", default="1,16,256")
    ap.add_argument("--budget", type=float, default=1e9)
    a = ap.parse_args()
    from qrlsh import _lib, users
    from qrlsh.userlists import UserLists
    if not torch.cuda.is_available():
        raise SystemExit("user_columns_probe needs a GPU")
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
            with open(os.path.join(a.out, "user_columns_probe.json"), "w") as fh:
                json.dump(out, fh, indent=1)

    base = torch.from_numpy(ratings).cuda()
    for nc in (max(1, nu // 6), 40):
        labels = rng.randint(0, nc, size=nu).astype(np.int64)
        ul = UserLists.build(base, labels, K=K, device="cuda")
        for kind, fill in (("append", 0.01), ("remove", None), ("overwrite", 0.01), ("append", 0.25), ("overwrite", 0.25)):
            for m in (int(x) for x in a.counts.split(",")):
                if time.time() - t0 > a.budget:
                    continue
                er = np.random.default_rng(100 * nc + m + (7 if fill == 0.25 else 0))
                cols = np.sort(er.choice(nq, size=m, replace=False))
                cd = torch.from_numpy(cols).cuda()
                if kind == "append":
                    block = (er.integers(1, 101, size=(nu, m)) * (er.random((nu, m)) < fill)).astype(np.int32)
                    bd = torch.from_numpy(block).cuda()
                    want = torch.cat((base, bd), dim=1)
                    op = lambda w: w.add_columns(bd)
                elif kind == "remove":
                    keep = torch.ones(nq, dtype=torch.bool, device="cuda")
                    keep[cd] = False
                    want = base[:, keep].contiguous()
                    op = lambda w: w.remove_columns(cols)
                else:
                    block = ratings[:, cols].copy()
                    hit = er.random((nu, m)) < fill
                    block[hit] = er.integers(0, 101, size=int(hit.sum()))
                    bd = torch.from_numpy(block).cuda()
                    want = base.clone()
                    want[:, cd] = bd
                    op = lambda w: w.set_columns(cols, bd)
                w = fork(ul)
                rows = op(w)
                picked = w.last_picked
                if not torch.equal(w.ratings, want):
                    raise SystemExit("clusters=%d %s %d: the matrix differs from torch indexing" % (nc, kind, m))
                fresh = UserLists.build(want, labels, K=K, device="cuda")
                for name in SMALL + ("ratings",):
                    if not torch.equal(getattr(w, name), getattr(fresh, name)):
                        raise SystemExit("clusters=%d %s %d: %s differs from the fresh build" % (nc, kind, m, name))
                if not torch.equal(base, torch.from_numpy(ratings).cuda()):
                    raise SystemExit("the matrix given to build was changed")
                del fresh, w
                call_ms = event_ms(op, a.reps, before=lambda: fork(ul))
                _lib.prof_enable(True)
                for _ in range(a.reps):
                    op(fork(ul))
                torch.cuda.synchronize()
                kern = {lab: round(ms / a.reps, 4) for lab, (cnt, ms) in sorted(_lib.prof_report().items())}
                _lib.prof_enable(False)
                host = want.cpu().numpy()
                rebuild_ms = event_ms(lambda: UserLists.build(host, labels, K=K, device="cuda"), max(1, a.reps - 1))
                dst = torch.empty_like(want)
                dst.copy_(want)
                copy_ms = event_ms(lambda: dst.copy_(want), 2 * a.reps)
                by = 2 * want.numel() * 4
                move_ms = kern.get("ratings_columns_move", 0.0)
                rec = {"shape": "%d users x %d queries, %d clusters, K=%d, %s %d columns%s" % (
                           nu, nq, nc, K, kind, m, "" if fill is None else " (%g %% of users each)" % (100 * fill)),
                       "date": datetime.date.today().isoformat(), "nu": nu, "nq": nq, "clusters": nc, "K": K,
                       "operation": kind, "columns": m, "fill": fill, "rows_rewritten": int(rows), "picked_rows": int(picked),
                       "changed_rows": int(rows) - int(picked), "checked_against_fresh_build_same_process": True,
                       "call_ms": round(call_ms, 3), "kernels_ms": kern, "kernels_total_ms": round(sum(kern.values()), 3),
                       "upload_plus_build_ms": round(rebuild_ms, 2), "rebuild_over_call": round(rebuild_ms / call_ms, 1),
                       "move_kernel_ms": move_ms, "copy_ms": round(copy_ms, 4), "matrix_bytes_read_plus_written": by,
                       "move_GBps": round(by / (move_ms * 1e-3) / 1e9, 1) if move_ms else None,
                       "copy_GBps": round(by / (copy_ms * 1e-3) / 1e9, 1),
                       "move_rate_over_copy_rate": round(copy_ms / move_ms, 3) if move_ms else None}
                out.append(rec)
                print(json.dumps(rec), flush=True)
                save()
                del want, dst, host
                torch.cuda.empty_cache()
        full_ms = event_ms(lambda: users.user_similarities(ul.ratings, labels, K, "cuda"), a.reps)
        rec = {"shape": "%d users x %d queries, %d clusters, K=%d, users.user_similarities on the device matrix" % (nu, nq, nc, K),
               "clusters": nc, "full_user_similarities_call_ms": round(full_ms, 3)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        save()
        del ul
    print("total %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
