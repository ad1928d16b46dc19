"""int8 storage (storage="int8"): call latency of cosine top-100 through rank_batch on (a) an int8 index, (b) a float8 e4m3 index and
(c) a bfloat16 index over the SAME values -- integers of at most four significant bits in [-120, 120], which all three formats
hold exactly.  The float8 index is the yardstick: same bytes, same kernels, another conversion (8 instructions per 16-byte load
on the VALU scan and 8 per 8-byte fragment on the matrix cores, where int8 pays 16 and 12).

p50 over --calls synchronous calls per index and query count (host queries in, host results out), after --warmup calls of the same
shape.  The contenders take turns call by call, so drift of the clock or of the machine hits all of them alike; the int8 index
takes two turns per round ((a) and (a')) and the difference of their two medians is the run-to-run spread the other columns are
read against.  Shapes: --rows (default 10M) at d = 384 and --side-rows (default 2M) at d = 128 / 256 / 384 / 512.

    python tools/time_i8.py [--rows 10000000] [--side-rows 2000000] [--calls 60] [--warmup 5] --out profiles/i8_time.txt
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

F8 = torch.float8_e4m3fn
CHUNK = 1_000_000


def shared_values():
    """The integers that are int8, float8 e4m3 and bfloat16 numbers at once: |x| <= 127 with at most four significant bits."""
    mags = [m for m in range(0, 128) if m == 0 or (m >> max(m.bit_length() - 4, 0)) << max(m.bit_length() - 4, 0) == m]
    vals = sorted(set(mags) | {-m for m in mags})
    return torch.tensor(vals, dtype=torch.int8)


def make_matrices(n, d, dev):
    """Random draws from shared_values() on the device as int8, and the same values as float8 and bfloat16 through three tables
    converted on the host (each value is exact in each format), a million rows at a time."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    vals = shared_values()
    as8 = vals.float().to(F8)
    assert torch.equal(as8.float(), vals.float()) and torch.equal(vals.to(torch.bfloat16).float(), vals.float()), "a shared value is not exact"
    t_i8, t_f8, t_bf = vals.to(dev), as8.view(torch.uint8).to(dev), vals.to(torch.bfloat16).to(dev)
    i8 = torch.empty((n, d), dtype=torch.int8, device=dev)
    f8 = torch.empty((n, d), dtype=torch.uint8, device=dev)
    bf = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        pick = torch.randint(0, vals.numel(), (m, d), generator=g, device=dev)
        i8[r0:r0 + m] = t_i8[pick]
        f8[r0:r0 + m] = t_f8[pick]
        bf[r0:r0 + m] = t_bf[pick]
    return {"i8": i8, "f8": f8.view(F8), "bf16": bf}


def one_call(ranking, h, Q):
    t0 = time.perf_counter()
    ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")
    return (time.perf_counter() - t0) * 1e6


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_i8.py: cosine top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a), (a') int8 index, two turns per round (spread = |a - a'| / a)   (b) float8 e4m3 index   (c) bfloat16 index; the same values in all three",
             f"# {'rows':>10} {'d':>4} {'queries':>7} {'(a) i8':>9} {'(a) again':>9} {'spread':>7} {'(b) f8':>9} {'(c) bf16':>9} {'(a)/(b)':>8} {'(a)/(c)':>8}  mfma a/b/c"]
    shapes = [(n, 384) for n in a.rows] + [(n, d) for n in a.side_rows for d in (128, 256, 384, 512)]
    for n, d in shapes:
        mats = make_matrices(n, d, dev)
        hs = [ranking.register_vectors(mats["i8"], storage="int8"), ranking.register_vectors(mats["f8"]), ranking.register_vectors(mats["bf16"])]
        assert hs[0].index.dtype == 7 and hs[1].index.dtype == 5 and hs[2].index.dtype == 3
        order = [0, 1, 2, 0]                             # (a) (b) (c) (a')
        rng = np.random.default_rng(7)
        for nq in a.queries:
            Q = rng.standard_normal((nq, d)).astype(np.float32)
            for _ in range(a.warmup):
                for h in hs:
                    one_call(ranking, h, Q)
            t = [[], [], [], []]
            for _ in range(a.calls):
                for slot, i in enumerate(order):
                    t[slot].append(one_call(ranking, hs[i], Q))
            p = [float(np.median(x)) for x in t]
            st = [h.index.stat("mfma") for h in hs]
            lines.append(f"  {n:>10} {d:>4} {nq:>7} {p[0]:>9.1f} {p[3]:>9.1f} {abs(p[0] - p[3]) / p[0]:>7.3f} {p[1]:>9.1f} {p[2]:>9.1f} "
                         f"{p[0] / p[1]:>8.2f} {p[0] / p[2]:>8.2f}  {st[0]}/{st[1]}/{st[2]}")
            print(lines[-1], flush=True)
        for h in hs:
            h.close()
        del mats, hs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[10_000_000])
    ap.add_argument("--side-rows", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 4, 5, 16, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_i8.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
