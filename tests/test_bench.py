"""bench.py's command line and outputs: a plain run times the headline only (the other legs need --full), and
--dump-outputs writes what the last timed step returned, so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_dtypes_and_cap(tmp_path, monkeypatch):
    import bench
    idx = np.array([[9, 3, 10_000_001]], dtype=np.int64)
    sc = np.array([[0.5, 0.25, -1.0]], dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "a"), idx, sc)
    gi, gs = np.load(tmp_path / "a" / "indices.npy"), np.load(tmp_path / "a" / "scores.npy")
    assert gi.dtype == np.float64 and gs.dtype == np.float32
    assert np.array_equal(gi.astype(np.int64), idx) and np.array_equal(gs, sc)
    # above the cap: a fixed, seeded sample of the same columns of both arrays, identical from call to call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 12 * 40)
    idx = np.arange(1000, dtype=np.int64)[None, :]
    sc = -np.arange(1000, dtype=np.float32)[None, :]
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), idx, sc)
    gi, gs = np.load(tmp_path / "b" / "indices.npy"), np.load(tmp_path / "b" / "scores.npy")
    assert gi.shape == gs.shape == (1, 40) and np.array_equal(gs, -gi.astype(np.float32))
    assert np.array_equal(gi, np.load(tmp_path / "c" / "indices.npy"))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """A small plain run in a fresh process: the result line holds the contract fields and no --full leg, and the dumped
    arrays are the answer of the same path to the last timed query, computed here again."""
    import torch
    import bench
    from hyperdb._native import GpuIndex, METRIC_IDS
    from hyperdb.sharded import ShardedIndex
    from oracle import ranking_oracle as orc
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    n, d, k, steps, warmup = 300_000, 384, 100, 4, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--rows", str(n), "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dtype"] == "f16"
    assert line["batched"] is None and line["api"] is None and line["cpu_baseline"] is None and "extra" not in line
    gi, gs = np.load(out / "indices.npy"), np.load(out / "scores.npy")
    assert gi.dtype == np.float64 and gs.dtype == np.float32 and gi.shape == gs.shape == (1, k)

    dev = torch.device("cuda", 0)
    V, _, _ = bench.make_shard(n, d, torch.float16, 0, 1, dev)
    q = bench.make_queries(steps + warmup, d, torch.float16, dev).to(torch.float32)[warmup + steps - 1:warmup + steps]
    ix = GpuIndex(V, device=dev)
    sh = ShardedIndex(ix, n_total=n)
    try:
        ei, es = sh.query(q, k, METRIC_IDS["cosine_similarity"])
    finally:
        sh.close()
        ix.close()
    assert np.array_equal(gi.astype(np.int64), ei) and np.array_equal(gs, es)
    orc.check_topk(ei[0], es[0], V.cpu().numpy(), q[0].cpu().numpy().astype(np.float16), "cosine_similarity", k, tol=1e-3)
