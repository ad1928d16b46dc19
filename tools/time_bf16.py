"""bfloat16 storage: call latency of cosine top-100 on (a) a bf16 index, (b) the same tensor widened to float64 -- what the engine
did with a torch.bfloat16 matrix before it stored the dtype -- and (c) an fp16 index of the same values.

p50 over --calls synchronous calls per index and query count (hyperDB_ranking_algorithm_sort for one query, rank_batch for more:
host queries in, host results out), after --warmup calls of the same shape; the three indices take turns call by call, so drift
of the clock or of the machine hits all of them alike.  Claims checked: (a) at least 2x faster than (b) at every query count;
(a) against (c) is recorded only (three bf16 MFMAs per k-step against one fp16 MFMA).

    python tools/time_bf16.py [--rows 2000000 [10000000 ...]] [--d 384] [--calls 60] [--warmup 5] [--out profiles/bf16_time.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import hyperdb.ranking_algorithm as ranking


def one_call(h, Q):
    t0 = time.perf_counter()
    if Q.shape[0] == 1:
        ranking.hyperDB_ranking_algorithm_sort(h, Q[0], top_k=100, metric="cosine_similarity")
    else:
        ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2_000_000])
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 4, 16, 64, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_bf16.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_bf16.py: cosine top-100, d = {a.d}, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the three indices alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a) bf16 index   (b) the same tensor widened to float64   (c) fp16 index of the same values",
             f"# {'rows':>10} {'queries':>7} {'(a) bf16':>10} {'(b) f64':>10} {'(c) fp16':>10} {'(b)/(a)':>8} {'(a)/(c)':>8}  mfma(a)  2x claim"]
    misses = []
    for n in a.rows:
        g = torch.Generator(device=dev); g.manual_seed(n)
        Vb = torch.randn((n, a.d), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
        hs = [ranking.register_vectors(Vb), ranking.register_vectors(Vb.to(torch.float64)), ranking.register_vectors(Vb.to(torch.float16))]
        rng = np.random.default_rng(7)
        for nq in a.queries:
            Q = rng.standard_normal((nq, a.d)).astype(np.float32)
            for _ in range(a.warmup):
                for h in hs:
                    one_call(h, Q)
            t = [[], [], []]
            for _ in range(a.calls):
                for i, h in enumerate(hs):
                    t[i].append(one_call(h, Q))
            p = [float(np.median(x)) for x in t]
            ok = p[1] / p[0] >= 2.0
            if not ok:
                misses.append((n, nq, p[1] / p[0]))
            lines.append(f"  {n:>10} {nq:>7} {p[0]:>10.1f} {p[1]:>10.1f} {p[2]:>10.1f} {p[1] / p[0]:>8.2f} {p[0] / p[2]:>8.2f}  {hs[0].index.stat('mfma'):>7}  "
                         f"{'holds' if ok else 'MISSED'}")
            print(lines[-1], flush=True)
        for h in hs:
            h.close()
        del Vb, hs
        torch.cuda.empty_cache()
    if misses:
        lines.append("# verdict: the 2x claim against the float64 widening is MISSED at " +
                     ", ".join(f"{n} rows x {q} queries ({r:.2f}x)" for n, q, r in misses))
    else:
        lines.append("# verdict: the bf16 index is at least 2x faster than the float64 widening in every row of the table")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
