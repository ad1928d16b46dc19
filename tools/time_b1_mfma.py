"""Packed-bit batches on the bf16 matrix cores (set_option("b1_mfma_min_q", n), csrc/hdb_mfma_b1.h): call latency of cosine and
euclidean top-100 through rank_batch on
  (m)  a bits index with the option on (b1_mfma_min_q = 5),
  (s)  the SAME handle with the option off: the bit scan, four queries per pass,
  (i)  a storage="int8" index over the same 0/1 values,
  (f)  a bfloat16 index over the same 0/1 values.

The protocol of tools/time_b1.py: p50 over --calls synchronous calls per contender, metric and query count (host queries in, host
results out), after --warmup calls of the same shape; the contenders take turns call by call, so drift of the clock or of the machine
hits all of them alike; (m) takes two turns per round ((m) and (m')) and the difference of their two medians is the run-to-run spread
the other columns are read against.  A contender that does not fit the device's free memory beside the others is dropped and its
columns read "-".  The rule hdb_mfma_b1_min_q (csrc/hdb_caps.h) is derived from the (s)/(m) column: the smallest measured batch
size from which (m) beats (s) by more than the spread at every larger measured size.

    python tools/time_b1_mfma.py [--shapes 10000000x384 ...] [--queries 5 8 16 64 128] [--calls 60] --out profiles/b1_mfma_time.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from time_b1 import one_call, packed_rows, shape, widened

METRICS = ("cosine_similarity", "euclidean_metric")
SHAPES = [(10_000_000, 384), (2_000_000, 384), (2_000_000, 128), (2_000_000, 256), (2_000_000, 512), (10_000_000, 1024),
          (2_000_000, 768), (2_000_000, 1024), (375_000, 4096)]


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_b1_mfma.py: top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (m), (m') bits index with b1_mfma_min_q = 5, two turns per round (spread = |m - m'| / m)   (s) the same handle with the option off (bit scan)   "
             "(i) storage=\"int8\" index   (f) bfloat16 index; the same 0/1 values in all",
             f"# {'rows':>10} {'bits':>5} {'metric':>18} {'queries':>7} {'(m) mfma':>9} {'(m) again':>9} {'spread':>7} {'(s) scan':>9} {'(i) i8':>9} {'(f) bf16':>9} {'(s)/(m)':>8} {'(i)/(m)':>8} {'(f)/(m)':>8}"]
    print("\n".join(lines), flush=True)
    for n, d in a.shapes:
        packed = packed_rows(n, d, dev)
        hb = ranking.register_vectors(packed, storage="bits", bitorder="little")
        assert hb.index.dtype == 10 and hb.index.V.numel() == n * d // 8
        i8 = widened(packed, d, torch.int8)
        hi = ranking.register_vectors(i8, storage="int8") if i8 is not None else None
        bf = widened(packed, d, torch.bfloat16)
        hf = ranking.register_vectors(bf) if bf is not None else None
        # contender -> (handle, value of b1_mfma_min_q for the turn or None)
        turns = [("m", hb, 5), ("s", hb, 0), ("i", hi, None), ("f", hf, None), ("m2", hb, 5)]
        turns = [t for t in turns if t[1] is not None]
        rng = np.random.default_rng(7)

        def turn(h, opt, Q, metric):
            if opt is not None:
                h.index.set_option("b1_mfma_min_q", opt)         # (outside the timed call)
            us = one_call(ranking, h, Q, metric)
            if opt is not None:
                assert h.index.stat("mfma") == (1 if opt else 0)
            return us

        for metric in METRICS:
            for nq in a.queries:
                Q = rng.standard_normal((nq, d)).astype(np.float32)
                Q /= np.linalg.norm(Q, axis=1, keepdims=True)
                for _ in range(a.warmup):
                    for _, h, opt in turns[:-1]:
                        turn(h, opt, Q, metric)
                t = {name: [] for name, _, _ in turns}
                for _ in range(a.calls):
                    for name, h, opt in turns:
                        t[name].append(turn(h, opt, Q, metric))
                p = {name: float(np.median(x)) for name, x in t.items()}
                col = lambda c: f"{p[c]:>9.1f}" if c in p else f"{'-':>9}"
                rat = lambda c: f"{p[c] / p['m']:>8.2f}" if c in p else f"{'-':>8}"
                lines.append(f"  {n:>10} {d:>5} {metric:>18} {nq:>7} {p['m']:>9.1f} {p['m2']:>9.1f} {abs(p['m'] - p['m2']) / p['m']:>7.3f} "
                             f"{col('s')} {col('i')} {col('f')} {rat('s')} {rat('i')} {rat('f')}")
                print(lines[-1], flush=True)
                if a.out:                                        # (kept current: a run that is cut short leaves what it measured)
                    with open(a.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
        for h in (hb, hi, hf):
            if h is not None:
                h.close()
        del packed, i8, bf, hb, hi, hf, turns
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=shape, nargs="*", default=SHAPES)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[5, 8, 16, 64, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_b1_mfma.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
