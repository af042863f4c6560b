"""Probe of the exact neighbour lists served from postings (qrlsh.answer_postings, exact_neighbours(postings=...),
csrc/postings.hip) on one GPU, beside the sweep route (postings=None) on the same box in the same process.

(a) exact_lists_probe's shape -- the synthetic table (D = 32768 rows x 16 features) and --nq queries (default configs[2]'s
    10 M) -- at m = 16 / 1024 / 16384 sampled requests and K = 10 and the run's K: call and per-kernel times of both
    routes and their ratio; the postings build alone, in ms and bytes against a device-to-device copy of the same bytes;
    the bytes of posting lists a request reads; and, on the 16 requests checked on the host, the share of candidates whose
    bound inter / |A(s)| is below the final K-th entry (what the bound can drop at most).
(b) all requests at --nq2 queries (default 100 000), both routes.
(c) all requests over a --nq3 prefix of the queries (default 1 M; 0 = skip), the postings route alone (the sweep on a
    sample): the basis of an estimate for all 10 M.
Every shape is checked for equality first: against exact_lists_probe's numpy route on 16 requests and against the sweep
route on every request timed, in the same process.

    python tools/exact_postings_probe.py [--nq N] [--nq2 N] [--nq3 N] [--reps N] [--out DIR] [--requests 16,1024,16384]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/exact_postings_probe.json.
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

from exact_lists_probe import build, numpy_route  # noqa: E402
from list_fidelity_probe import D  # noqa: E402
from list_length_probe import event_ms  # noqa: E402
from query_index_probe import timed  # noqa: E402

FIELDS = ("dst", "inter", "union", "listed", "positives")


def same(a, b, what):
    for k in FIELDS:
        if not torch.equal(getattr(a, k), getattr(b, k)):
            raise SystemExit("%s: the postings route's %s differs from the sweep route's" % (what, k))


def check_against_numpy(off, rows, nq, K, queries, postings, what):
    """-> the share of the 16 requests' candidates whose bound inter / a is below the final K-th J"""
    from qrlsh import exactlists, ops
    ho, hr = ops.to_host(off), ops.to_host(rows)
    want = numpy_route(ho, hr, nq, K, queries)
    got = exactlists.exact_neighbours(off, rows, D, K, queries=queries, postings=postings)
    have = (got.dst, got.inter, got.union, torch.stack([got.listed, got.positives], dim=1))
    for name, g, w in zip(("dst", "inter", "union", "counts"), have, want):
        if not np.array_equal(g.cpu().numpy(), w):
            raise SystemExit("%s, K = %d: the postings route's %s differs from the numpy route" % (what, K, name))
    sizes = np.diff(ho)
    below = total = 0
    for x, s in enumerate(int(q) for q in queries):
        member = np.zeros(D, dtype=np.int64)
        member[hr[ho[s]:ho[s + 1]]] = 1
        inter = np.bincount(np.repeat(np.arange(nq), sizes)[member[hr] > 0], minlength=nq)
        inter[s] = 0
        cand = inter[inter > 0]
        total += len(cand)
        if want[3][x, 0] == K:                       # a full list: its K-th entry is a threshold
            ki, ku = int(want[1][x, K - 1]), int(want[2][x, K - 1])
            below += int((cand * ku < ki * int(sizes[s])).sum())
    return below / total if total else 0.0


def list_bytes(off, rows, postings, queries):
    """mean bytes of posting lists (4 per entry) the requests read"""
    lens = (postings.p_off[1:] - postings.p_off[:-1])
    tot = 0
    for s in queries.tolist():
        tot += int(lens[rows[int(off[s].item()):int(off[s + 1].item())].to(torch.int64)].sum().item())
    return 4.0 * tot / max(len(queries), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    ap.add_argument("--nq", type=int, default=10_000_000)
    ap.add_argument("--nq2", type=int, default=100_000)
    ap.add_argument("--nq3", type=int, default=1_000_000)
    ap.add_argument("--requests", default="16,1024,16384")
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    import qrlsh
    from qrlsh import exactlists, fidelity, pipeline
    if not torch.cuda.is_available():
        raise SystemExit("exact_postings_probe needs a GPU")
    t0 = time.time()
    today = datetime.date.today().isoformat()
    out = []

    def emit(rec):
        rec = dict({"date": today, "D": D}, **rec)
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "exact_postings_probe.json"), "w") as fh:
                json.dump(out, fh, indent=1)

    def build_record(off, rows, nq, shape):
        nnz = int(rows.numel())
        make = lambda: qrlsh.answer_postings(off, rows, D)                                              # noqa: E731
        call_ms, kern = timed(make, a.reps)
        postings = make()
        nbytes = 8 * (D + 1) + 4 * nnz
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        copy_ms = event_ms(lambda: dst.copy_(src), max(a.reps, 10))
        del src, dst
        emit({"what": "postings build", "shape": shape, "nq": nq, "nnz": nnz, "call_ms": round(call_ms, 3),
              "kernels_ms": kern, "postings_bytes": nbytes, "csr_bytes": 8 * (nq + 1) + 4 * nnz,
              "scratch_bytes": int(qrlsh._lib.load().qrlsh_answer_postings_scratch_bytes(nnz, D)),
              "d2d_copy_of_the_same_bytes_ms": round(copy_ms, 4), "build_over_copy": round(call_ms / copy_ms, 1)})
        return postings

    def both(off, rows, nq, K, chosen, postings, shape, what, sweep_too=True):
        m = nq if chosen is None else len(chosen)
        via = lambda: exactlists.exact_neighbours(off, rows, D, K, queries=chosen, postings=postings)   # noqa: E731
        old = lambda: exactlists.exact_neighbours(off, rows, D, K, queries=chosen)                      # noqa: E731
        got = via()
        rec = {"what": what, "shape": shape, "nq": nq, "m": m, "K": K}
        if sweep_too:
            same(got, old(), "%s m=%d K=%d" % (what, m, K))
            sw_ms, sw_kern = timed(old, a.reps)
            rec.update({"sweep_call_ms": round(sw_ms, 3), "sweep_kernels_ms": sw_kern})
        po_ms, po_kern = timed(via, a.reps)
        rec.update({"postings_call_ms": round(po_ms, 3), "postings_kernels_ms": po_kern,
                    "postings_us_per_request": round(1e3 * po_ms / max(m, 1), 3),
                    "mean_positives": round(float(got.positives.double().mean().item()), 1),
                    "mean_listed": round(float(got.listed.double().mean().item()), 2)})
        if sweep_too:
            rec["sweep_over_postings"] = round(sw_ms / po_ms, 2)
        emit(rec)

    if "a" in a.parts:
        nq = a.nq
        K = min(pipeline.max_candidates(nq), fidelity.MAX_K)
        off, rows, lists = build(nq, K)
        del lists
        torch.cuda.empty_cache()
        shape = "%d queries, K = %d, table %d x 16" % (nq, K, D)
        postings = build_record(off, rows, nq, shape)
        sample = fidelity.sample_positions(nq, max(int(x) for x in a.requests.split(",")), seed=0)
        Ks = sorted({min(10, K), K})
        share = {K2: check_against_numpy(off, rows, nq, K2, sample[:16], postings, "(a)") for K2 in Ks}
        per_request = list_bytes(off, rows, postings, torch.from_numpy(sample[:256]))
        emit({"what": "what a request reads", "shape": shape, "nq": nq, "requests": 256,
              "posting_list_bytes_per_request": round(per_request), "sweep_share_bytes_per_request":
              round((4 * int(rows.numel()) + 8 * (nq + 1)) / fidelity.group_size(D)),
              "candidates_below_the_final_bound_share": {str(k): round(v, 4) for k, v in share.items()},
              "checked_requests": 16})
        for m in (int(x) for x in a.requests.split(",")):
            chosen = torch.from_numpy(sample[:m]).cuda()
            for K2 in Ks:
                both(off, rows, nq, K2, chosen, postings, shape, "chosen requests, both routes")
        if "c" in a.parts and 0 < a.nq3 < nq:
            n3 = a.nq3
            off3 = off[:n3 + 1].clone()
            rows3 = rows[:int(off3[-1].item())].clone()
            shape3 = "the first %d of those queries" % n3
            del off, rows, postings
            torch.cuda.empty_cache()
            p3 = build_record(off3, rows3, n3, shape3)
            pick = torch.from_numpy(fidelity.sample_positions(n3, 1024, seed=1)).cuda()
            same(exactlists.exact_neighbours(off3, rows3, D, K, queries=pick, postings=p3),
                 exactlists.exact_neighbours(off3, rows3, D, K, queries=pick), "(c) sample")
            both(off3, rows3, n3, K, None, p3, shape3, "all requests of a prefix, postings route", sweep_too=False)
            del off3, rows3, p3
        torch.cuda.empty_cache()

    if "b" in a.parts:
        nq = a.nq2
        K = min(pipeline.max_candidates(nq), fidelity.MAX_K)
        off, rows, lists = build(nq, K)
        del lists
        shape = "%d queries, K = %d, table %d x 16" % (nq, K, D)
        postings = build_record(off, rows, nq, shape)
        pick = fidelity.sample_positions(nq, 16, seed=0)
        check_against_numpy(off, rows, nq, K, pick, postings, "(b)")
        both(off, rows, nq, K, None, postings, shape, "all requests, both routes")
    print("total %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
