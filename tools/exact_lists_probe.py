"""Probe of the exact neighbour lists (qrlsh.exact_neighbours, csrc/exactlists.hip) on one GPU: what producing the truth
costs beside measuring against it, and what the served model does with it.

(a) list_fidelity_probe's shape -- table_rows_probe's synthetic table (D = 32768 rows x 16 features of 4 values each) and
    --nq queries (default configs[2]'s 10 M), 128 permutations / 32 bands, the run's K -- at m = 16 / 1024 / 16384 sampled
    requests and K = 10 and the run's K: call and per-kernel times of exact_neighbours BESIDE list_fidelity at the same m
    in the same process (the fidelity sweep is the yardstick, not a gate: the ratio is reported whichever way it falls),
    and the sweep's rate against its byte floor, the CSR once per group of requests.
(b) all exact lists at --nq2 queries (default 100 000, the prediction shape's query count) over the same table, K = the
    run's (28): the time to build them.
(c) on that shape -- 2000 users x 100 000 queries, 25 % rated, user lists of 19 -- over the LSH lists and over the exact
    lists: evaluate(hold-out), evaluate_ranking(k = 10, candidates = "heldout"), and the recall of the LSH lists from
    list_fidelity and, independently, from the exact lists themselves.  THE RATINGS ARE RANDOM: no list can predict
    them, so (c)'s quality figures say what the calls cost and that they run, not which lists serve better.
Every shape is first checked on 16 requests against a numpy route over host copies, in the same process.

    python tools/exact_lists_probe.py [--nq N] [--nq2 N] [--reps N] [--out DIR] [--requests 16,1024,16384]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/exact_lists_probe.json.
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

from evaluate_probe import num  # noqa: E402
from list_fidelity_probe import NFEAT, NVALS, D, P, BANDS  # noqa: E402
from list_length_probe import event_ms  # noqa: E402
from query_index_probe import timed  # noqa: E402

SEED = 20
RELEVANT = 60


def build(nq, K):
    """list_fidelity_probe's table and queries -> (offsets, rows, (src, dst, val) of the LSH run at K)"""
    from qrlsh import ops, pipeline
    from qrlsh.table import LiveTable
    rng = np.random.default_rng(1)
    base_id = 1 + np.arange(NFEAT) * NVALS
    lt = LiveTable(NFEAT, D, "cuda")
    for f in range(NFEAT):
        lt.dictionary.maps[f] = {str(v): int(base_id[f] + v) for v in range(NVALS)}
    lt.dictionary.nrows = 1 + NFEAT * NVALS
    lt._place((rng.integers(0, NVALS, size=(D, NFEAT)) + base_id).astype(np.int32), np.arange(D, dtype=np.int64))
    g = torch.Generator(device="cuda").manual_seed(2)
    rank = torch.rand((nq, NFEAT), generator=g, device="cuda").argsort(dim=1).argsort(dim=1)
    k = 5 + torch.randint(0, 2, (nq, 1), generator=g, device="cuda")
    vals = torch.randint(0, NVALS, (nq, NFEAT), generator=g, device="cuda") + torch.from_numpy(base_id).cuda()
    lt.qrows = torch.where(rank < k, vals, torch.full_like(vals, -1)).to(torch.int32).contiguous()
    del rank, vals, k
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42))
    off, rows = lt.answer_sets()
    res = pipeline.query_similarities(off, rows, table, BANDS, K)
    lists = (res.src, res.dst, res.val)
    del res
    torch.cuda.empty_cache()
    return off, rows, lists


def numpy_route(off, rows, nq, K, queries):
    """exact_neighbours' (dst, inter, union [m, K], counts [m, 2]) from host arrays: one membership gather over the whole
    CSR per request, then a sort by the one-word key (inter << 43) // union (injective for unions <= 2^21) and the id"""
    sizes = np.diff(off)
    nonempty = np.nonzero(sizes > 0)[0]
    ids = np.arange(nq)
    m = len(queries)
    dst = np.full((m, K), -1, dtype=np.int32)
    inter_o, union_o = np.zeros((m, K), dtype=np.int32), np.zeros((m, K), dtype=np.int32)
    counts = np.zeros((m, 2), dtype=np.int32)
    for x, s in enumerate(int(q) for q in queries):
        member = np.zeros(D, dtype=np.int64)
        member[rows[off[s]:off[s + 1]]] = 1
        inter = np.zeros(nq, dtype=np.int64)
        inter[nonempty] = np.add.reduceat(member[rows], off[:-1][nonempty])
        union = sizes[s] + sizes - inter
        pos = np.nonzero((inter > 0) & (ids != s))[0]
        key = (inter[pos] << 43) // union[pos]
        best = pos[np.lexsort((pos, -key))[:K]]
        L = len(best)
        dst[x, :L], inter_o[x, :L], union_o[x, :L] = best, inter[best], union[best]
        counts[x] = (L, len(pos))
    return dst, inter_o, union_o, counts


def check_against_numpy(off, rows, nq, K, queries, what):
    from qrlsh import exactlists, ops
    t1 = time.time()
    want = numpy_route(ops.to_host(off), ops.to_host(rows), nq, K, queries)
    numpy_s = (time.time() - t1) / max(len(queries), 1)
    got = exactlists.exact_neighbours(off, rows, D, K, queries=queries)
    have = (got.dst, got.inter, got.union, torch.stack([got.listed, got.positives], dim=1))
    for name, g, w in zip(("dst", "inter", "union", "counts"), have, want):
        if not np.array_equal(g.cpu().numpy(), w):
            raise SystemExit("%s, K = %d: exact_neighbours' %s differs from the numpy route" % (what, K, name))
    return numpy_s


def recall_from_exact(off, rows, lsh, exact, K):
    """hits / reachable of the LSH lists' first K entries, from the exact lists alone: an entry is a hit when the row is
    not full (fewer than K queries share a row at all) or its J is not below that of the exact K-th entry"""
    from qrlsh import fidelity
    src, dst, _ = lsh
    s64 = src.to(torch.int64)
    start = torch.zeros(int(exact.listed.numel()) + 1, dtype=torch.int64, device=src.device)
    start[1:] = torch.bincount(s64, minlength=int(exact.listed.numel())).cumsum(0)
    place = torch.arange(int(src.numel()), device=src.device) - start[s64]
    inter = fidelity.edge_overlaps(off, rows, src, dst).to(torch.int64)
    sizes = off[1:] - off[:-1]
    union = sizes[s64] + sizes[dst.to(torch.int64)] - inter
    full = (exact.listed == K)[s64]
    ki, ku = exact.inter[:, K - 1].to(torch.int64)[s64], exact.union[:, K - 1].to(torch.int64)[s64]
    hit = (place < K) & (~full | (inter * ku >= ki * union))
    return int(hit.sum().item()), int(exact.listed.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nq", type=int, default=10_000_000)
    ap.add_argument("--nq2", type=int, default=100_000)
    ap.add_argument("--nu", type=int, default=2000)
    ap.add_argument("--requests", default="16,1024,16384")
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import exactlists, fidelity, pipeline, predict
    if not torch.cuda.is_available():
        raise SystemExit("exact_lists_probe needs a GPU")
    t0 = time.time()
    today = datetime.date.today().isoformat()
    G = fidelity.group_size(D)
    out = []

    def emit(rec):
        rec = dict({"date": today, "D": D, "group": G}, **rec)
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "exact_lists_probe.json"), "w") as fh:
                json.dump(out, fh, indent=1)

    # ---- (a) chosen requests beside list_fidelity
    if "a" in a.parts:
        nq = a.nq
        K = min(pipeline.max_candidates(nq), fidelity.MAX_K)
        off, rows, (src, dst, val) = build(nq, K)
        nnz = int(rows.numel())
        shape = "%d queries x %d/%d, K = %d, table %d x %d" % (nq, P, BANDS, K, D, NFEAT)
        sample = fidelity.sample_positions(nq, max(int(x) for x in a.requests.split(",")), seed=0)
        Ks = sorted({min(10, K), K})
        numpy_s = {K2: check_against_numpy(off, rows, nq, K2, sample[:16], "(a)") for K2 in Ks}
        buf = torch.empty_like(rows)
        copy_ms = event_ms(lambda: buf.copy_(rows), max(a.reps, 10))
        del buf
        for m in (int(x) for x in a.requests.split(",")):
            chosen = torch.from_numpy(sample[:m]).cuda()
            for K2 in Ks:
                exact = lambda: exactlists.exact_neighbours(off, rows, D, K2, queries=chosen)          # noqa: E731
                judge = lambda: fidelity.list_fidelity(off, rows, D, src, dst, val, nq, K2, queries=chosen)   # noqa: E731
                call_ms, kern = timed(exact, a.reps)
                fd_ms, fd_kern = timed(judge, a.reps)
                res = exact()
                groups = -(-len(chosen) // G)
                S = exactlists.slice_count(nq, len(chosen), D)
                floor = groups * (4 * nnz + 8 * (nq + 1))
                sweep, fd_sweep = kern.get("exact_sweep", 0.0), fd_kern.get("fidelity_sweep", 0.0)
                emit({"what": "exact_neighbours beside list_fidelity", "shape": shape, "nq": nq, "m": len(chosen), "K": K2,
                      "call_ms": round(call_ms, 3), "kernels_ms": kern, "groups": groups, "slices": S,
                      "scratch_bytes": len(chosen) * S * K2 * 3 * 4,
                      "list_fidelity_call_ms": round(fd_ms, 3), "list_fidelity_kernels_ms": fd_kern,
                      "exact_sweep_over_fidelity_sweep": round(sweep / fd_sweep, 3) if fd_sweep else None,
                      "exact_call_over_fidelity_call": round(call_ms / fd_ms, 3),
                      "sweep_floor_bytes": floor,
                      "sweep_floor_GBps": round(floor / (sweep * 1e-3) / 1e9, 1) if sweep else None,
                      "d2d_copy_of_rows_ms": round(copy_ms, 4),
                      "d2d_copy_GBps": round(2 * 4 * nnz / (copy_ms * 1e-3) / 1e9, 1),
                      "numpy_route_s_per_request": round(numpy_s[K2], 3), "checked_requests": 16,
                      "mean_positives": round(float(res.positives.double().mean().item()), 1),
                      "mean_listed": round(float(res.listed.double().mean().item()), 2)})
        del off, rows, src, dst, val
        torch.cuda.empty_cache()

    # ---- (b) all queries of the prediction shape, (c) the served model over the LSH lists and over the exact ones
    if "b" in a.parts or "c" in a.parts:
        nq, nu = a.nq2, a.nu
        K, Ku = min(pipeline.max_candidates(nq), fidelity.MAX_K), pipeline.max_candidates(nu)
        off, rows, lsh = build(nq, K)
        shape = "%d x %d, 25 %% rated, K = %d / %d, table %d x %d" % (nu, nq, K, Ku, D, NFEAT)
        pick = fidelity.sample_positions(nq, 16, seed=0)
        numpy_s = check_against_numpy(off, rows, nq, K, pick, "(b)")
        build_all = lambda: exactlists.exact_neighbours(off, rows, D, K)                                # noqa: E731
        call_ms, kern = timed(build_all, a.reps)
        exact = build_all()
        coo_ms = event_ms(lambda: exact.coo(), a.reps)
        x = exact.coo()
        emit({"what": "all exact lists", "shape": shape, "nq": nq, "m": nq, "K": K, "call_ms": round(call_ms, 3),
              "kernels_ms": kern, "groups": -(-nq // G), "slices": exactlists.slice_count(nq, nq, D),
              "coo_ms": round(coo_ms, 3), "entries": int(x[0].numel()), "lsh_entries": int(lsh[0].numel()),
              "cut_as_milli_0": int(exact.listed.sum().item()) - int(x[0].numel()),
              "numpy_route_s_per_request": round(numpy_s, 3), "checked_requests": 16,
              "mean_positives": round(float(exact.positives.double().mean().item()), 1)})
        if "c" in a.parts:
            rng = np.random.RandomState(0)
            ratings = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
            for r0 in range(0, nu, 250):
                ratings[r0:r0 + 250][rng.rand(min(250, nu - r0), nq) < 0.75] = 0
            usims = {u: {"indexes": rng.randint(0, nu, size=Ku), "values": np.round(rng.rand(Ku), 3)} for u in range(nu)}
            rt = torch.from_numpy(ratings).cuda()
            prepared = predict.user_lists(usims, nu, "cuda")
            train, count = qrlsh.holdout(rt, 0.1, seed=SEED)
            lf = fidelity.list_fidelity(off, rows, D, *lsh, nq, K)
            lf_ms, _ = timed(lambda: fidelity.list_fidelity(off, rows, D, *lsh, nq, K), 1)
            hits, reachable = recall_from_exact(off, rows, lsh, exact, K)
            if (hits, reachable) != (int(lf.totals[3]), int(lf.totals[5])):
                raise SystemExit("(c): the recall from the exact lists (%d / %d) differs from list_fidelity's (%d / %d)"
                                 % (hits, reachable, lf.totals[3], lf.totals[5]))
            own = fidelity.list_fidelity(off, rows, D, *x, nq, K)
            emit({"what": "recall of the LSH lists, from both calls", "shape": shape, "K": K, "hits": hits,
                  "reachable": reachable, "recall_list_fidelity": num(lf.recall, 6),
                  "recall_from_exact_lists": num(hits / reachable if reachable else float("nan"), 6),
                  "list_fidelity_all_queries_call_ms": round(lf_ms, 3), "inversion_share": num(lf.inversion_share, 6),
                  "exact_lists_judged_by_list_fidelity": {"hits": int(own.totals[3]), "listed": int(own.totals[0]),
                                                          "inversions": int(own.totals[7])}})
            for name, lists in (("LSH", lsh), ("exact", x)):
                run_ev = lambda: qrlsh.evaluate(train, *lists, prepared, truth=rt, fraction=0.1, seed=SEED)   # noqa: E731
                run_rk = lambda: qrlsh.evaluate_ranking(train, rt, *lists, prepared, 10, RELEVANT,           # noqa: E731
                                                        candidates="heldout")
                ev, rk = run_ev(), run_rk()
                ev_ms, _ = timed(run_ev, a.reps)
                rk_ms, _ = timed(run_rk, a.reps)
                emit({"what": "served model over the lists", "lists": name, "shape": shape, "held_out_cells": int(count),
                      "ratings": "uniform random: the figures are about cost, no list can predict them",
                      "list_entries": int(lists[0].numel()), "mean_milli": round(float(lists[2].double().mean().item()), 1),
                      "evaluate_holdout_call_ms": round(ev_ms, 3), "n": int(ev.n), "covered": int(ev.covered),
                      "rmse": num(ev.rmse), "mae": num(ev.mae), "coverage": num(ev.coverage),
                      "evaluate_ranking_k10_heldout_call_ms": round(rk_ms, 3), "precision": num(rk.precision),
                      "recall": num(rk.recall), "ndcg": num(rk.ndcg), "hit_rate": num(rk.hit_rate)})
    print("total %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
