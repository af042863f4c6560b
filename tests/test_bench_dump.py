"""CPU tests: bench.py --dump-outputs.  The sample depends on the shape alone, every written array holds the
caller's values for the sampled queries, and the parts of N ranks merge into exactly what one GPU's result gives.
A HotPathResult built from the oracle's whole-path output stands in for the device's."""
import os

import numpy as np
import pytest
import torch

import bench
from oracle import oracle as O
from qrlsh import pipeline
from qrlsh.dist import shard_range

NQ, D, P, B = 20000, 32768, 128, 32


@pytest.fixture(scope="module")
def ref():
    off, rows = O.synth_csr(NQ, D, seed=0)
    return O.query_similarities(off, rows, D, P, B, pipeline.max_candidates(NQ), 42)


def _result(ref, q0=0, n=NQ, pair_mask=None):
    """the HotPathResult a rank owning queries [q0, q0 + n) and the candidate pairs under pair_mask returns"""
    sig = ref["sig"][q0:q0 + n]
    pairs = ref["pairs"] if pair_mask is None else ref["pairs"][pair_mask]
    milli = ref["milli"] if pair_mask is None else ref["milli"][pair_mask]
    own = (ref["src"] >= q0) & (ref["src"] < q0 + n)
    t = torch.from_numpy
    return pipeline.HotPathResult(t(sig.copy()), t((sig.astype(np.int64) ** 2).sum(1)), t(pairs.view(np.int64).copy()),
                                  t(milli.copy()), t(ref["src"][own].copy()), t(ref["dst"][own].copy()),
                                  t(ref["val"][own].copy()))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_sample_is_fixed_sorted_and_bounded():
    a, b = bench.dump_query_ids(10_000_000, 128), bench.dump_query_ids(10_000_000, 128)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_QUERIES
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10_000_000
    assert np.array_equal(bench.dump_query_ids(1000, 128), np.arange(1000))      # small shapes: every query
    big = bench.dump_query_ids(10_000_000, 8192)                                  # wide rows: fewer of them
    assert len(big) * (4 * 8192 + 16) <= bench.DUMP_SIG_BYTES


def test_dump_holds_the_results_values_for_the_sampled_queries(ref, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_QUERIES", 3000)
    qids = bench.dump_query_ids(NQ, P)
    nbytes = bench.write_dump(str(tmp_path), [bench.dump_part(_result(ref), qids, NQ, 0, NQ)])
    d = _load(tmp_path)
    assert set(d) == {"queries", "sig", "norm2", "pairs", "milli", "src", "dst", "val"}
    assert nbytes == sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20
    for k, v in d.items():
        assert v.dtype in (np.float32, np.float64), k
    assert np.array_equal(d["queries"], qids)
    assert np.array_equal(d["sig"], ref["sig"][qids])
    assert np.array_equal(d["norm2"], (ref["sig"][qids].astype(np.int64) ** 2).sum(1))
    ij = O.u64_to_pairs(ref["pairs"])
    on = np.isin(ij[:, 0], qids) | np.isin(ij[:, 1], qids)
    assert on.sum() > len(qids)                                     # the sample has real candidate lists
    assert np.array_equal(d["pairs"], ij[on]) and np.array_equal(d["milli"], ref["milli"][on])
    kept = np.isin(ref["src"], qids)
    for k in ("src", "dst", "val"):
        assert np.array_equal(d[k], ref[k][kept]), k


def test_dump_of_sharded_ranks_equals_the_one_gpu_dump(ref, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_QUERIES", 3000)
    qids = bench.dump_query_ids(NQ, P)
    bench.write_dump(str(tmp_path / "one"), [bench.dump_part(_result(ref), qids, NQ, 0, NQ)])
    world, parts = 3, []
    host = ref["pairs"] % np.uint64(world)                          # every pair scored by exactly one rank
    for rank in range(world):
        q0, n, _ = shard_range(NQ, world, rank)
        parts.append(bench.dump_part(_result(ref, q0, n, host == rank), qids, NQ, q0, n))
    bench.write_dump(str(tmp_path / "three"), parts)
    one, three = _load(tmp_path / "one"), _load(tmp_path / "three")
    assert one.keys() == three.keys()
    for k in one:
        assert np.array_equal(one[k], three[k]), k


def test_dump_thins_long_lists_by_a_fixed_sample(ref, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_QUERIES", 3000)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 500)
    qids = bench.dump_query_ids(NQ, P)
    for sub in ("a", "b"):
        bench.write_dump(str(tmp_path / sub), [bench.dump_part(_result(ref), qids, NQ, 0, NQ)])
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert len(a["pairs"]) == len(a["milli"]) == 500 and len(a["src"]) == len(a["val"]) == 500
    w = a["pairs"][:, 0] * 2.0 ** 32 + a["pairs"][:, 1]
    assert np.all(np.diff(w) > 0)                                   # a sorted subset of the sorted list
    ij = O.u64_to_pairs(ref["pairs"])
    pos = np.searchsorted(ij[:, 0] * 2.0 ** 32 + ij[:, 1], w)
    assert np.array_equal(ij[pos], a["pairs"]) and np.array_equal(ref["milli"][pos], a["milli"])


@pytest.mark.gpu
def test_bench_dump_outputs_of_the_device_path(tmp_path):
    """the real command on a small workload, on one GPU and as two gloo ranks sharing it: one JSON line naming the
    requested timed steps, and the same arrays from both, equal to the oracle's values for the sampled queries"""
    import json
    import subprocess
    import sys
    nq = 200_000
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    common = ["--steps", "3", "--warmup", "1", "--nq-total", str(nq), "--no-secondary", "--cpu-sample", "0"]
    runs = {"one": ["--gpus", "1"], "two": ["--gpus", "2", "--dist-backend", "gloo", "--share-gpu"]}
    for name, extra in runs.items():
        p = subprocess.run([sys.executable, bench.__file__] + extra + common + ["--dump-outputs", str(tmp_path / name)],
                           env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        assert json.loads(lines[0])["steps"] == 3
    one, two = _load(tmp_path / "one"), _load(tmp_path / "two")
    assert one.keys() == two.keys()
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    off, rows = O.synth_csr(nq, D, seed=0)
    r = O.query_similarities(off, rows, D, P, B, pipeline.max_candidates(nq), 42)
    qids = bench.dump_query_ids(nq, P)
    assert np.array_equal(one["queries"], qids) and len(qids) < nq
    assert np.array_equal(one["sig"], r["sig"][qids])
    assert np.array_equal(one["norm2"], (r["sig"][qids].astype(np.int64) ** 2).sum(1))
    ij = O.u64_to_pairs(r["pairs"])
    on = np.isin(ij[:, 0], qids) | np.isin(ij[:, 1], qids)
    assert np.array_equal(one["pairs"], ij[on]) and np.array_equal(one["milli"], r["milli"][on])
    kept = np.isin(r["src"], qids)
    for k in ("src", "dst", "val"):
        assert np.array_equal(one[k], r[k][kept]), k


@pytest.mark.parametrize("steps", ["0", "-1"])
def test_bench_refuses_a_run_without_timed_steps(steps, monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", steps])
    with pytest.raises(SystemExit):
        bench.parse()
