"""Timing probe of the diversified lists (qrlsh.diversify, qrlsh.for_users_diverse, qrlsh.list_redundancy) on one GPU.

Shape: the N1 shape of the serving probes (2000 users x 100 000 queries, 25 % rated, K = 28 query / 19 user
neighbours).  The ratings and user lists follow bench.py's N1 recipe; the query lists take each query's neighbours out
of its id window (+-64) with a fifth of the values at 1000, so that neighbours predict alike and pools hold stored
neighbours -- with uniformly random lists a pool of 1024 out of 100 000 columns has next to no internal edge.
Configurations: pools of 64, 256 and 1024; k = 10 and 28; 16 and 2000 requests; penalty 0, a moderate penalty
(20 rating points per unit of similarity) and max_sim = 1.

Every configuration is checked first: the device result against the host route below on every request, and the host
route against the plain restatement of the tests (tests/diversify_cases.greedy_ref) on the first 16 requests.  Then,
per configuration: the call time of qrlsh.diversify over device pools; the per-kernel times of its two phases from the
library's HIP-event profiler; for_users(k = pool) alone (what the rerank adds to); the route a caller has today (pools
and lists copied to the host, the pool's dense similarity built with numpy, the greedy selection there -- and the time
of greedy_ref itself on 16 requests); the half-edge bytes phase A writes; the redundancy of the plain and of the
reranked lists.

    python tools/diversify_probe.py [--quick] [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/diversify_probe[_quick].json.
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

MODERATE = 20000
SETTINGS = (("plain", 0, 1001), ("moderate", MODERATE, 1001), ("exclude", 0, 1))


def inputs(nu, nq, seed, dev, window=64):
    from qrlsh import pipeline, predict
    rng = np.random.RandomState(seed)
    Kq, Ku = pipeline.max_candidates(nq), pipeline.max_candidates(nu)
    ratings = rng.randint(1, 101, size=(nu, nq)).astype(np.int32)
    for r0 in range(0, nu, 250):
        ratings[r0:r0 + 250][rng.rand(min(250, nu - r0), nq) < 0.75] = 0
    # Kq distinct window offsets per query, the first deg of them kept; rows value descending, id ascending
    deg = rng.randint(0, Kq + 1, size=nq)
    offs = np.argsort(rng.rand(nq, 2 * window), axis=1)[:, :Kq]
    offs = np.where(offs < window, offs - window, offs - window + 1)            # -window .. -1, 1 .. window
    dst = np.arange(nq)[:, None] + offs
    keep = (np.arange(Kq)[None, :] < deg[:, None]) & (dst >= 0) & (dst < nq)
    mil = np.where(rng.rand(nq, Kq) < 0.2, 1000, rng.randint(1, 1001, size=(nq, Kq)))
    src = np.broadcast_to(np.arange(nq)[:, None], dst.shape)[keep]
    dst, mil = dst[keep], mil[keep]
    o = np.lexsort((dst, -mil, src))
    coo_host = tuple(x[o].astype(np.int32) for x in (src, dst, mil))
    usims = {u: {"indexes": rng.randint(0, nu, size=Ku), "values": np.round(rng.rand(Ku), 3)} for u in range(nu)}
    rt = torch.from_numpy(ratings).to(dev)
    coo = tuple(torch.from_numpy(x).to(dev) for x in coo_host)
    return rt, coo, coo_host, predict.user_lists(usims, nu, dev), (Kq, Ku)


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


class HostRoute:
    """what a caller can do today with the pools and the lists on the host: per request the dense similarity of the pool
    from the CSR rows (numpy), then the greedy selection over it"""

    def __init__(self, coo_host, nq):
        src, self.dst, self.mil = coo_host
        self.off = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=nq)))).astype(np.int64)
        self.pos = np.full(nq, -1, dtype=np.int64)

    def dense(self, cols):
        n = len(cols)
        if n == 0:
            return np.zeros((0, 0), dtype=np.int64), 0
        self.pos[cols] = np.arange(n)
        lens = self.off[cols + 1] - self.off[cols]
        ent = np.repeat(self.off[cols] - np.concatenate(([0], np.cumsum(lens)[:-1])), lens) + np.arange(lens.sum())
        a, b, v = np.repeat(np.arange(n), lens), self.pos[self.dst[ent]], self.mil[ent].astype(np.int64)
        self.pos[cols] = -1
        ok = (b >= 0) & (b != a)
        s = np.zeros((n, n), dtype=np.int64)
        np.maximum.at(s, (a[ok], b[ok]), v[ok])
        return np.maximum(s, s.T), 2 * int(ok.sum())

    @staticmethod
    def greedy(s, vals, k, penalty, max_sim):
        n = len(vals)
        r, free = np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
        base, picks, red = 1000 * vals.astype(np.int64), [], []
        for _ in range(min(k, n)):
            elig = free & (r < max_sim)
            if not elig.any():
                break
            c = int(np.argmax(np.where(elig, base - penalty * r, np.iinfo(np.int64).min)))   # first of the largest
            picks.append(c)
            red.append(int(r[c]))
            free[c] = False
            r = np.maximum(r, s[c])
        return picks, red


def redundancy_of(cols_picked, s, where):
    """[entries, pairs, sim sum, largest] of one list given as columns; s is dense over pool positions"""
    p = np.array([where[int(c)] for c in cols_picked], dtype=np.int64)
    sub = np.triu(s[np.ix_(p, p)], 1)
    return [len(p), int((sub > 0).sum()), int(sub.sum()), int(sub.max()) if sub.size else 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="pools of 64 and 256, 16 and 200 requests")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import _lib
    import diversify_cases as DC
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("diversify_probe needs a GPU")
    dev = "cuda"
    nu, nq = 2000, 100_000
    rt, coo, coo_host, prepared, (Kq, Ku) = inputs(nu, nq, 0, dev)
    route = HostRoute(coo_host, nq)
    lists = {}
    for q in range(nq):
        lo, hi = route.off[q], route.off[q + 1]
        if hi > lo:
            lists[q] = (route.dst[lo:hi].astype(np.int64), route.mil[lo:hi].astype(np.int64))
    out = []
    for m in ((16, 200) if a.quick else (16, 2000)):
        users = torch.from_numpy(np.random.RandomState(m).choice(nu, size=m, replace=False).astype(np.int32)).to(dev)
        for pool in ((64, 256) if a.quick else (64, 256, 1024)):
            def serve():
                return qrlsh.for_users(rt, *coo, prepared, users, pool, device=dev)
            ci, cv, av = serve()
            serve_ms = timed(serve, a.reps)
            # the host route: the copies, then per request the dense similarity and the greedy selection of every
            # variant (the dense matrices are not kept: 8 MB each at a pool of 1024)
            t0 = time.perf_counter()
            hi_, hv, ha = (t.cpu().numpy() for t in (ci, cv, av))
            _ = tuple(t.cpu().numpy() for t in coo)
            copy_s = time.perf_counter() - t0
            variants = [(k, name, penalty, max_sim) for k in (10, 28) for name, penalty, max_sim in SETTINGS]
            want = {v: (np.full((m, v[0]), -1, dtype=np.int32), np.zeros((m, v[0]), dtype=np.int32)) for v in variants}
            host_red = {v: [0, 0, 0, 0] for v in variants}
            greedy_s = {v: 0.0 for v in variants}
            dense_s, half_edges = 0.0, 0
            for x in range(m):
                t0 = time.perf_counter()
                cols = hi_[x, :max(0, min(pool, ha[x]))].astype(np.int64)
                s, he = route.dense(cols)
                dense_s += time.perf_counter() - t0
                half_edges += he
                where = {int(c): p for p, c in enumerate(cols)}
                for v in variants:
                    t0 = time.perf_counter()
                    picks, red = route.greedy(s, hv[x, :len(cols)], v[0], v[2], v[3])
                    greedy_s[v] += time.perf_counter() - t0
                    want[v][0][x, :len(picks)], want[v][1][x, :len(picks)] = cols[picks], red
                    words = redundancy_of(cols[picks], s, where)
                    host_red[v] = [host_red[v][0] + words[0], host_red[v][1] + words[1], host_red[v][2] + words[2],
                                   max(host_red[v][3], words[3])]
            for v in variants:
                k, name, penalty, max_sim = v

                def rerank():
                    return qrlsh.diversify(ci, cv, av, *coo, nq, k, penalty=penalty, max_sim=max_sim, device=dev)
                got = tuple(t.cpu().numpy() for t in rerank())
                if not (np.array_equal(got[0], want[v][0]) and np.array_equal(got[2], want[v][1])):
                    raise SystemExit("m=%d pool=%d k=%d %s: the device differs from the host route" % (m, pool, k, name))
                t0 = time.perf_counter()
                ref = DC.greedy_ref(hi_[:16], hv[:16], ha[:16], lists, k, penalty, max_sim)
                ref_s = time.perf_counter() - t0
                for g, w in zip(got, ref):
                    if not np.array_equal(g[:16], w):
                        raise SystemExit("m=%d pool=%d k=%d %s: differs from greedy_ref" % (m, pool, k, name))
                kern = kernels(rerank, a.reps)
                dev_idx = torch.from_numpy(got[0]).to(dev)
                dev_red = qrlsh.list_redundancy(dev_idx, *coo, nq, device=dev)
                if [int(t) for t in dev_red.totals] != host_red[v]:
                    raise SystemExit("m=%d pool=%d k=%d %s: list_redundancy differs from the host" % (m, pool, k, name))
                plain = np.where(np.arange(k)[None, :] < np.minimum(ha, k)[:, None], hi_[:, :k], -1)
                rec = {"m": m, "pool": pool, "k": k, "setting": name, "penalty": penalty, "max_sim": max_sim,
                       "diversify_call_ms": round(timed(rerank, a.reps), 4),
                       "list_redundancy_call_ms": round(timed(lambda: qrlsh.list_redundancy(
                           dev_idx, *coo, nq, device=dev), a.reps), 4),
                       "kernels_ms": {lab: ms for lab, ms in kern.items() if lab.startswith("diversify")},
                       "for_users_at_pool_call_ms": round(serve_ms, 4),
                       "host_route_ms": {"copy_pools_and_lists": round(copy_s * 1e3, 2),
                                         "dense_similarity": round(dense_s * 1e3, 2),
                                         "greedy": round(greedy_s[v] * 1e3, 2),
                                         "total": round((copy_s + dense_s + greedy_s[v]) * 1e3, 2)},
                       "greedy_ref_16_requests_ms": round(ref_s * 1e3, 2),
                       "half_edges": half_edges, "half_edge_bytes_written": 4 * half_edges,
                       "redundancy_plain": host_red[(k, "plain", 0, 1001)], "redundancy_reranked": host_red[v],
                       "lists_changed": int((got[0] != plain).any(axis=1).sum()),
                       "checked": "device == host route on every request; == greedy_ref on the first 16"}
                out.append(rec)
                print(json.dumps(rec), flush=True)
            if a.out:   # after every (m, pool): what has run is kept
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "diversify_probe%s.json" % ("_quick" if a.quick else "")), "w") as fh:
                    json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
