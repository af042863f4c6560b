"""Timing probe of appending queries to a built index (qrlsh_index_append, csrc/index.hip) on one GPU.

Shapes: the index at configs[2] (10 M queries x 128 / 32 bands, D = 32768, bench.py's synthetic recipe, the hot path's
own MinHash band keys), then batches of m = 1, 1024, 16 384 and 1 M further queries of the same recipe appended to it.
Every shape is first checked: the appended arrays equal a fresh qrlsh_index_build of the same n + m keys byte for
byte, and two sampled bands equal the numpy restatement (tests/index_append_cases.restate_layout).  Then, in the
same process, per-kernel times from the library's HIP-event profiler and the call time of
  * the append (the batch's keys are restored by a copy of [b][m] words before every call), and
  * the rebuild the append replaces: qrlsh_index_build over the same n + m keys,
with the algorithmic bytes of the append (12 B read + 12 B written per record of b x (n + m), plus the directory and the
batch's sort), the fraction of the 8 TB/s HBM peak, the ratio to the rebuild and the distance from the byte floor at
the 6.29 TB/s streaming-copy rate DESIGN section 4 records.

    python tools/query_index_append_probe.py [--reps N] [--out DIR]

Each result is printed as one JSON line; --out DIR also writes them all to DIR/query_index_append_probe.json.
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

from query_index_probe import HBM_PEAK, timed  # noqa: E402

COPY_RATE = 6.29e12      # streaming copy, DESIGN section 4


def check(ops, base, new, fresh, n, m, bands):
    """the appended arrays against the fresh build (all bands, on the device) and the restatement (sampled bands)"""
    import index_append_cases as AC
    got = ops.index_append(*base[:3], new.clone())
    for name, a, f in zip(("keys", "ids", "dir"), got, fresh):
        if a.shape != f.shape or not torch.equal(a, f):
            raise SystemExit("append m=%d: %s differ from the fresh build" % (m, name))
    dw = got[2].numel() // got[0].shape[0]
    for t in bands:
        raw = torch.cat((base[3][t], new[t])).cpu().numpy()[None]
        sk, ids, dirw = AC.restate_layout(raw)
        if not (np.array_equal(got[0][t].cpu().numpy().view(np.uint64), sk[0]) and
                np.array_equal(got[1][t].cpu().numpy().view(np.uint32), ids[0]) and
                np.array_equal(got[2][t * dw:(t + 1) * dw].cpu().numpy().view(np.uint32), dirw)):
            raise SystemExit("append m=%d: band %d differs from the restatement" % (m, t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for a JSON file of all results (default: print only)")
    a = ap.parse_args()
    from qrlsh import _lib, ops, synth
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("query_index_append_probe needs a GPU")
    t0 = time.time()
    nq, extra, D, P, b = 10_000_000, 1 << 20, 32768, 128, 32
    offsets, rows = synth.synth_csr(nq + extra, D, seed=0)
    table = ops.perm_table(ops.legacy_permutations(P, D, seed=42))
    _, _, allkeys = ops.minhash(offsets, rows, table, b=b, want_norm=True, compact=True, validate=False)
    del offsets, rows
    raw = allkeys[:, :nq].contiguous()                     # the indexed queries' keys, unsorted (for the restatement)
    keys, ids, dirw = ops.index_build(raw.clone())
    base = (keys, ids, dirw, raw)
    out = []
    for m in (1, 1024, 16384, extra):
        n = nq + m
        new = allkeys[:, nq:n].contiguous()
        full = allkeys[:, :n].contiguous()
        fresh = ops.index_build(full.clone())
        check(ops, base, new, fresh, nq, m, (0, 17))
        del fresh
        work = new.clone()

        def append():
            work.copy_(new)
            ops.index_append(keys, ids, dirw, work)
        call_ms, kern = timed(append, a.reps)
        fwork = full.clone()

        def rebuild():
            fwork.copy_(full)
            ops.index_build(fwork)
        rcall_ms, rkern = timed(rebuild, a.reps)
        del fwork
        torch.cuda.empty_cache()
        rec_n = b * n
        dir_bytes = int(lib.qrlsh_index_dir_words(n, b)) * 4
        # merge: key + id of every record read and written, the directory written; the batch: four sort passes over
        # (key, id) and a histogram read each, the rank's key read and position written, the positions read by the merge
        by = rec_n * 24 + dir_bytes + b * m * (4 * (2 * 12 + 8) + 8 + 4 + 4)
        kms, rms = sum(kern.values()), sum(rkern.values())
        floor_ms = (rec_n * 24 + dir_bytes) / COPY_RATE * 1e3
        rec = {"shape": "append m=%d to 10M x 128/32" % m, "n": nq, "m": m, "checked_against_fresh_build": True,
               "checked_against_restatement_bands": [0, 17],
               "call_ms_incl_batch_key_copy": round(call_ms, 4), "kernels_ms": kern, "kernels_total_ms": round(kms, 4),
               "algorithmic_bytes": int(by), "GBps": round(by / (kms * 1e-3) / 1e9, 1),
               "hbm_peak_fraction": round(by / HBM_PEAK / (kms * 1e-3), 3),
               "rebuild_same_keys": {"call_ms_incl_key_restore_copy": round(rcall_ms, 4), "kernels_ms": rkern,
                                     "kernels_total_ms": round(rms, 4)},
               "append_over_rebuild": round(kms / rms, 3), "rebuild_over_append": round(rms / kms, 2),
               "byte_floor_ms_at_6.29TBps": round(floor_ms, 4), "append_over_byte_floor": round(kms / floor_ms, 2)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    print("total %.1f s" % (time.time() - t0), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "query_index_append_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
