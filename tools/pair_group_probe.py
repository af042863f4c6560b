#!/usr/bin/env python3
"""The pair grouping alone on the step's real emitted words (development tool):
    python tools/pair_group_probe.py [nq = 10000000] [reps = 10]
MinHash + bucket emit of the standard workload once, then qrlsh_pair_regions_scatter32 `reps` times on those words with
the step's own group bits and capacities; prints min / median / max ms per call (events round the call).  The library
is the tree's, or the one QRLSH_LIB names: build dedup.hip with -DQR_PG_IPT_N1=.. -DQR_PG_IPT_N2=.. into another
libqrlsh.so to compare tile sizes.  Per-level times: run it under `rocprofv3 --kernel-trace --stats` (two launches of
pair_group_scatter_kernel per call, 2 warm-up calls + reps)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd")):
    sys.path.insert(0, p)
import torch
import qrlsh
from qrlsh import ops, _lib
nq = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
lib = _lib.load()
off, rows = qrlsh.synth_csr(nq, 32768, seed=0, device="cuda")
table = ops.perm_table(ops.legacy_permutations(128, 32768, seed=42), "cuda")
_, _, keys = ops.minhash(off, rows, table, b=32)
em = ops.emit_pairs_any(keys, 4)
del keys, off, rows
n = em.numel(); ib = ops.id_bits_for(nq); wpq = n / nq
g = ops.region_group_bits(ib, nq, wpq)
words = lib.qrlsh_pair_regions_words(n, nq, g, wpq); tw = lib.qrlsh_pair_regions_tmp_words(n, nq, g, wpq)
nreg = lib.qrlsh_pair_regions_count(n, nq, g, wpq)
regions = torch.empty((words,), dtype=torch.int32, device="cuda")
tmp = torch.empty((max(tw, 1),), dtype=torch.int64, device="cuda")
counts = torch.empty((nreg + 256,), dtype=torch.int32, device="cuda"); ovf = torch.empty((1,), dtype=torch.int32, device="cuda")
P, st = ops._ptr, ops._stream()
def run():
    _lib.check(lib.qrlsh_pair_regions_scatter32(P(em), n, g, ib, nq, wpq, P(tmp), P(regions), P(counts), P(ovf), st))
run(); run(); torch.cuda.synchronize()
ts = []
for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); run(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
ts.sort()
print("lib", os.environ.get("QRLSH_LIB", "tree"), "n", n, "g", g, "ovf", int(ovf.item()), "sum", int(counts[:nreg].to(torch.int64).sum().item()),
      "pair_group ms min %.4f med %.4f max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1]))
