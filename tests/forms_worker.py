"""Worker for the forms of the bucket path that the library picks once, when it loads (QRLSH_FIN_PACKED=0: the
separate-counter small-part finish at T >= 12; QRLSH_EMIT_GROUPS=n: the number of band groups): started as a child
process by tests/test_gpu_buckets.py with the variable set, so the test process's own library keeps its defaults.
Runs the T = 12 exact-fill cases and the two-group case of tests/bucket_cases.py through ops.emit_pairs_any and writes
each case's emitted words, sorted, to <out_dir>/<n>.u64, with <out_dir>/cases.json naming them (the parent checks them
against the oracle).  usage: python forms_worker.py <out_dir>"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "query-recommendation-system_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bucket_cases as B  # noqa: E402
from qrlsh import ops  # noqa: E402


def main():
    out = sys.argv[1]
    torch.cuda.set_device(0)
    done = []
    cases = [B.fill_case(12, N) for N in B.FILLS[12]] + [B.two_group_case()]
    for n, c in enumerate(cases):
        stats = {}
        emitted = ops.emit_pairs_any(torch.from_numpy(c.keys).cuda(), 4, stats)
        words, _ = torch.sort(emitted)          # (signed order: the words are below 2^63, so the same as unsigned)
        del emitted
        name = "%d.u64" % n
        words.cpu().numpy().tofile(os.path.join(out, name))
        done.append({"name": c.name, "file": name, "path": stats["bucket_path"], "words": int(words.numel())})
        print("%s: %d words, %s" % (c.name, words.numel(), stats["bucket_path"]), flush=True)
        del words
        torch.cuda.empty_cache()
    with open(os.path.join(out, "cases.json"), "w") as f:
        json.dump(done, f)
    print("FORMS_WORKER_OK", os.environ.get("QRLSH_FIN_PACKED"), os.environ.get("QRLSH_EMIT_GROUPS"))


if __name__ == "__main__":
    main()
