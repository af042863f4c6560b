"""Timing probe of changing the list length of the live lists in place (QueryIndex.set_list_length: qrlsh_lists_cut_*,
qrlsh_lists_regrow_mark, qrlsh_index_pick_keys, csrc/listcut.hip; UserLists.set_list_length) on one GPU.

Shapes: index and lists of configs[2] (10 M queries x 128 / 32 bands, D = 32768, bench.py's synthetic recipe, the run's
K = 40) from the hot path itself; cuts 40 -> 28 / 20 / 10 / 1, regrows 28 -> 40 and 10 -> 40 (from the runs at 28 and
10); the user side at bench.py's N4 matrix (2000 users x 100 000 queries, 40 clusters, K = 19): a cut 19 -> 10 and the
regrow 10 -> 19.  Every shape is first checked in this process, element for element, against a full run (a full
UserLists.build) at the new length.  Then each is timed
  * against the route it replaces, in the same process: the hot-path step at K2 plus QueryIndex.from_result (the user
    side: UserLists.build at K2);
  * against the same cut written as a torch mask (keep = i < K2 or src[i - K2] != src[i]; three masked selects);
  * against a device-to-device copy that moves the cut's byte floor -- 8 B per stored entry read (src, by count and
    fill) plus 8 B read and 12 B written per surviving entry.
Per-kernel times come from the library's HIP-event profiler (mean of --reps after a warm-up).

    python tools/list_length_probe.py [--reps N] [--out DIR] [--nq N] [--nu N] [--unq N]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/list_length_probe.json.
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

from query_index_probe import timed  # noqa: E402

CUT = ("lists_cut_count", "lists_cut_fill", "lists_cut_total", "scan_blocks")
REGROW = ("lists_regrow_mark", "idmap_popc", "idmap_pack", "idmap_list", "index_pick_keys", "lists_remove_count",
          "lists_remove_fill", "lists_fill_probed", "lists_remove_total", "scan_blocks")
REPROBE = ("index_probe_count", "index_probe_fill", "index_score", "index_select", "index_compact")


def same(got, want, what):
    for name, g, w in zip(("src", "dst", "val"), got, want):
        if g.shape != w.shape or not torch.equal(g, w):
            raise SystemExit("%s: %s differs from the full run" % (what, name))


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_cut(src, dst, val, K2):
    keep = torch.ones_like(src, dtype=torch.bool)
    keep[K2:] = src[K2:] != src[:-K2]
    return src[keep], dst[keep], val[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nq", type=int, default=10_000_000)
    ap.add_argument("--nu", type=int, default=2000)
    ap.add_argument("--unq", type=int, default=100_000)
    a = ap.parse_args()
    from qrlsh import ops, pipeline, synth, users
    from qrlsh.index import QueryIndex
    from qrlsh.userlists import UserLists
    if not torch.cuda.is_available():
        raise SystemExit("list_length_probe needs a GPU")
    t0 = time.time()
    nq, D, P, b = a.nq, 32768, 128, 32
    K = pipeline.max_candidates(nq)
    offsets, rows = synth.synth_csr(nq, D, seed=0)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42))
    today = datetime.date.today().isoformat()
    out = []

    def run(K2):
        return pipeline.query_similarities(offsets, rows, table, b, K2)

    def lists_of(res):
        return res.src, res.dst, res.val

    res = run(K)
    base = QueryIndex.from_result(res, table, lists=True)
    E = res.src.numel()
    scale = lambda k: max(1, round(k * K / 40))      # noqa: E731  (the targets of configs[2], scaled with a smaller --nq)
    for K2 in sorted({scale(k) for k in (28, 20, 10, 1)}, reverse=True):
        if K2 >= K:
            continue
        full = lists_of(run(K2))
        qi = copy.copy(base)
        qi.set_list_length(K2)
        same(qi.lists, full, "cut %d -> %d" % (K, K2))
        same(torch_cut(*base.lists, K2), full, "torch mask %d -> %d" % (K, K2))
        S = full[0].numel()
        del qi, full
        call_ms, kern = timed(lambda: copy.copy(base).set_list_length(K2), a.reps)
        route_ms = event_ms(lambda: QueryIndex.from_result(run(K2), table, lists=True), a.reps)
        mask_ms = event_ms(lambda: torch_cut(*base.lists, K2), a.reps)
        floor = 8 * E + 20 * S
        buf = torch.empty((floor // 2,), dtype=torch.uint8, device="cuda")
        buf2 = torch.empty_like(buf)
        copy_ms = event_ms(lambda: buf2.copy_(buf), max(a.reps, 10))
        del buf, buf2
        kms = sum(kern.get(k, 0.0) for k in ("lists_cut_count", "lists_cut_fill"))
        rec = {"shape": "cut %d -> %d, lists of %d x %d/%d" % (K, K2, nq, P, b), "date": today, "n": nq, "K_old": K,
               "K_new": K2, "stored_entries": E, "surviving_entries": S, "picked_rows": 0,
               "checked_against_full_run_same_process": True,
               "set_list_length": {"call_ms": round(call_ms, 4), "kernels_ms": {k: v for k, v in kern.items() if k in CUT}},
               "count_plus_fill_ms": round(kms, 4), "floor_bytes": floor,
               "d2d_copy_of_floor_bytes_ms": round(copy_ms, 4),
               "share_of_copy_rate": round(copy_ms / kms, 3) if kms else None,
               "floor_GBps": round(floor / (kms * 1e-3) / 1e9, 1) if kms else None,
               "torch_mask_call_ms": round(mask_ms, 4), "torch_mask_over_call": round(mask_ms / call_ms, 2),
               "hot_path_step_plus_from_result_ms": round(route_ms, 4), "route_over_call": round(route_ms / call_ms, 2)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    want = lists_of(res)
    for K1 in sorted({scale(28), scale(10)}, reverse=True):
        if K1 >= K:
            continue
        small = QueryIndex.from_result(run(K1), table, lists=True)
        E1 = small.lists[0].numel()
        qi = copy.copy(small)
        picked = qi.set_list_length(K)
        same(qi.lists, want, "regrow %d -> %d" % (K1, K))
        del qi
        call_ms, kern = timed(lambda: copy.copy(small).set_list_length(K), a.reps)
        route_ms = event_ms(lambda: QueryIndex.from_result(run(K), table, lists=True), a.reps)
        own = round(sum(v for k, v in kern.items() if k in REGROW), 4)
        probe = round(sum(v for k, v in kern.items() if k in REPROBE), 4)
        rec = {"shape": "regrow %d -> %d, lists of %d x %d/%d" % (K1, K, nq, P, b), "date": today, "n": nq, "K_old": K1,
               "K_new": K, "stored_entries": E1, "output_entries": E, "picked_rows": picked,
               "picked_share_of_rows": round(picked / nq, 4), "checked_against_full_run_same_process": True,
               "set_list_length": {"call_ms": round(call_ms, 4), "kernels_ms": kern,
                                   "kernels_total_ms": round(sum(kern.values()), 4)},
               "mark_keys_substitute_ms": own, "reprobe_ms": probe,
               "hot_path_step_plus_from_result_ms": round(route_ms, 4), "route_over_call": round(route_ms / call_ms, 2)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del small
        torch.cuda.empty_cache()
    del base, res, want, offsets, rows
    torch.cuda.empty_cache()

    # ---- the user side
    nu, unq = a.nu, a.unq
    rng = np.random.RandomState(4)
    ratings = rng.randint(1, 101, size=(nu, unq)).astype(np.int32)
    ratings[rng.rand(nu, unq) < 0.75] = 0
    labels = rng.randint(0, 40, size=nu).astype(np.int64)
    KU = users.max_candidates(nu)
    KC = max(1, round(KU * 10 / 19))
    dev = torch.from_numpy(ratings).cuda()
    built = {k: UserLists.build(dev, labels, K=k, device="cuda") for k in (KU, KC)}
    for K1, K2 in ((KU, KC), (KC, KU)):
        if K1 == K2:
            continue
        ul = copy.copy(built[K1])
        n = ul.set_list_length(K2)
        for name in ("idx", "milli", "len"):
            if not torch.equal(getattr(ul, name), getattr(built[K2], name)):
                raise SystemExit("users %d -> %d: %s differs from a full build" % (K1, K2, name))
        call_ms, kern = timed(lambda: copy.copy(built[K1]).set_list_length(K2), a.reps)
        build_ms = event_ms(lambda: UserLists.build(dev, labels, K=K2, device="cuda"), a.reps)
        rec = {"shape": "users %d -> %d, %d users x %d queries, 40 clusters" % (K1, K2, nu, unq), "date": today, "nu": nu,
               "nq": unq, "K_old": K1, "K_new": K2, "rows_rescored": n, "checked_against_full_build_same_process": True,
               "set_list_length": {"call_ms": round(call_ms, 4), "kernels_ms": kern},
               "full_build_call_ms": round(build_ms, 4), "build_over_call": round(build_ms / call_ms, 2)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "list_length_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
