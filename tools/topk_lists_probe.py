#!/usr/bin/env python3
"""The select form's lists on the step's real pairs, and the fill call alone (development tool):
    python tools/topk_lists_probe.py [nq = 10000000] [reps = 20]
One step of the standard workload, then
  * the population of the three select kernels: how many lists topk_len_kernel puts on the medium and the long list
    (nlists[0], nlists[1], read back from the workspace and recomputed from the pairs), the long lists' lengths
    (min / median / p99 / max) and the share of the directed edges they hold;
  * qrlsh_topk_select_fill `reps` times on those lists with the auxiliary stream on and off (qrlsh_set_overlap),
    alternating; min / median / max ms per call (events round the call), the three kernels' own times (the library's
    profiler), and a check sum of the rows written.
The library is the tree's, or the one QRLSH_LIB names (to compare builds of csrc/topk.hip)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd")):
    sys.path.insert(0, p)
import torch
import qrlsh
from qrlsh import ops, pipeline, _lib
nq = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
lib = _lib.load()
off, rows = qrlsh.synth_csr(nq, 32768, seed=0, device="cuda")
table = ops.perm_table(ops.legacy_permutations(128, 32768, seed=42), "cuda")
K = pipeline.max_candidates(nq)
res = pipeline.query_similarities(off, rows, table, 32, K, validate=False)
pairs, ib = res.pairs, ops.id_bits_for(nq)
milli, rev = ops.score_pairs_rev(res.sig, res.norm2, pairs, ib)
n = pairs.numel()
# the lists, from the pairs: a query's list = its forward run (i = q) + its reverse run (j = q)
deg = torch.bincount(pairs >> 32, minlength=nq) + torch.bincount(pairs & 0xFFFFFFFF, minlength=nq)
lng = deg[deg > 64].sort().values
out = {"nq": nq, "K": K, "unique_pairs": n, "directed_edges": 2 * n, "medium_lists": int(((deg > 16) & (deg <= 64)).sum()),
       "long_lists": int(lng.numel()), "edges_in_medium_lists": int(deg[(deg > 16) & (deg <= 64)].sum()),
       "edges_in_long_lists": int(lng.sum())}
if lng.numel():
    out["long_len"] = {"min": int(lng[0]), "median": int(lng[lng.numel() // 2]), "p99": int(lng[int(lng.numel() * 0.99)]),
                       "max": int(lng[-1])}
    out["long_share_of_directed_edges"] = round(out["edges_in_long_lists"] / (2.0 * n), 4)
# the same calls ops.topk_select makes, with the workspace kept
P, st = ops._ptr, ops._stream()
if isinstance(rev, tuple):
    rs, rd = ops.sort_u64(rev[0], rev[1], 11, 11 + ib)
else:
    rs, rd = ops.sort_u64(rev, None, ib + 11, ib + 11 + ib)
ws = torch.empty((lib.qrlsh_topk_select_workspace_bytes(nq),), dtype=torch.uint8, device="cuda")
total = torch.zeros(1, dtype=torch.int64, device="cuda")
_lib.check(lib.qrlsh_topk_select_count(P(pairs), n, P(rs), P(rd), nq, K, ib, P(ws), ws.numel(), P(total), st))
m = int(total.item())
a16 = ((nq + 1) * 4 + 15) & ~15                      # csrc/topk.hip sel_ws: 4 u32 arrays, off u64[nq + 2], nlists u64[2]
o = 4 * a16 + (nq + 2) * 8
nl = ws[o:o + 16].view(torch.int64).tolist()
out["nlists_workspace"] = nl
assert nl == [out["medium_lists"], out["long_lists"]], (nl, out)
src, dst, val = (torch.empty((m,), dtype=torch.int32, device="cuda") for _ in range(3))
def fill():
    _lib.check(lib.qrlsh_topk_select_fill(P(pairs), P(milli), n, P(rs), P(rd), nq, K, ib, P(ws), P(src), P(dst), P(val), st))
ts = {1: [], 0: []}
for ov in (1, 0):
    lib.qrlsh_set_overlap(ov); fill(); fill()
torch.cuda.synchronize()
for _ in range(reps):
    for ov in (1, 0):
        lib.qrlsh_set_overlap(ov)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fill(); b.record(); torch.cuda.synchronize(); ts[ov].append(a.elapsed_time(b))
lib.qrlsh_set_overlap(1)
for ov in (1, 0):
    t = sorted(ts[ov])
    out["fill_ms_overlap_%d" % ov] = {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4), "max": round(t[-1], 4)}
# the three kernels one by one (events round every launch: with the profiler on they follow each other on one stream)
_lib.prof_enable(True)
for _ in range(reps):
    fill()
torch.cuda.synchronize()
rep = _lib.prof_report()
_lib.prof_enable(False)
out["kernel_ms"] = {lab: round(ms / reps, 4) for lab, (cnt, ms) in sorted(rep.items())}
out["kept_edges"] = m
out["checksum"] = int((src.to(torch.int64) * 3 + dst.to(torch.int64) * 5 + val.to(torch.int64) * 7).sum().item())
out["equal_to_step"] = bool(torch.equal(src, res.src) and torch.equal(dst, res.dst) and torch.equal(val, res.val))
out["lib"] = os.environ.get("QRLSH_LIB", "tree")
print(json.dumps(out))
