"""MXFP4 storage (storage="mxfp4"): call latency of cosine top-100 through rank_batch on (a) an MXFP4 index, (b) an int8 index over
the SAME values and (c) a packed-bit index over their signs (x > 0) -- random e2m1 codes under scale byte 128, i.e. the integers
{0, +-1, +-2, +-3, +-4, +-6, +-8, +-12}, which int8 holds exactly.  The int8 index is the yardstick for the arithmetic (twice the
bytes per element, the same 32 VALU instructions per 16-byte load), the bits index for the bytes (an eighth of int8's).

p50 over --calls synchronous calls per index and query count (host queries in, host results out), after --warmup calls of the same
shape.  The contenders take turns call by call, so drift of the clock or of the machine hits all of them alike; the MXFP4 index
takes two turns per round ((a) and (a')) and the difference of their two medians is the run-to-run spread the other columns are
read against.  Shapes: --rows (default 10M) at d = 384 and --side-rows (default 2M) at d = 128 / 512 / 1024 / 2048.

    python tools/time_f4.py [--rows 10000000] [--side-rows 2000000] [--calls 60] [--warmup 5] --out profiles/f4_time.txt
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

CHUNK = 1_000_000


def make_matrices(n, d, dev):
    """Random code bytes on the device -> (codes, scales) for the MXFP4 index, the same values as int8, their signs as packed bits
    in the little order, a million rows at a time."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    mags = torch.tensor([0, 1, 2, 3, 4, 6, 8, 12], dtype=torch.int8)
    table = torch.cat([mags, -mags]).to(dev)                        # the value of code c under scale byte 128
    codes = torch.empty((n, d // 2), dtype=torch.uint8, device=dev)
    i8 = torch.empty((n, d), dtype=torch.int8, device=dev)
    bits = torch.empty((n, d // 8), dtype=torch.uint8, device=dev)
    weights = (1 << torch.arange(8, device=dev)).to(torch.int32)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        c = torch.randint(0, 256, (m, d // 2), generator=g, device=dev, dtype=torch.int32)
        codes[r0:r0 + m] = c.to(torch.uint8)
        v = table[torch.stack([c & 15, c >> 4], dim=-1).reshape(m, d)]
        i8[r0:r0 + m] = v
        bits[r0:r0 + m] = ((v > 0).reshape(m, d // 8, 8).to(torch.int32) * weights).sum(dim=-1).to(torch.uint8)
    return codes, torch.full((n, d // 32), 128, dtype=torch.uint8, device=dev), i8, bits


def one_call(ranking, h, Q):
    t0 = time.perf_counter()
    ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")
    return (time.perf_counter() - t0) * 1e6


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_f4.py: cosine top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a), (a') MXFP4 index, two turns per round (spread = |a - a'| / a)   (b) int8 index, the same values   (c) bits index, their signs",
             f"# {'rows':>10} {'d':>5} {'queries':>7} {'(a) mxfp4':>9} {'(a) again':>9} {'spread':>7} {'(b) i8':>9} {'(c) bits':>9} {'(a)/(b)':>8} {'(a)/(c)':>8}  mfma a/b/c"]
    shapes = [(n, 384) for n in a.rows] + [(n, d) for n in a.side_rows for d in (128, 512, 1024, 2048)]
    for n, d in shapes:
        codes, scales, i8, bits = make_matrices(n, d, dev)
        hs = [ranking.register_vectors((codes, scales), storage="mxfp4"), ranking.register_vectors(i8, storage="int8"),
              ranking.register_vectors(bits, storage="bits", bitorder="little")]
        assert hs[0].index.dtype == 13 and hs[1].index.dtype == 7 and hs[2].index.dtype == 10
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
            lines.append(f"  {n:>10} {d:>5} {nq:>7} {p[0]:>9.1f} {p[3]:>9.1f} {abs(p[0] - p[3]) / p[0]:>7.3f} {p[1]:>9.1f} {p[2]:>9.1f} "
                         f"{p[0] / p[1]:>8.2f} {p[0] / p[2]:>8.2f}  {st[0]}/{st[1]}/{st[2]}")
            print(lines[-1], flush=True)
        for h in hs:
            h.close()
        del codes, scales, i8, bits, hs
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
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 2, 4, 5, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_f4.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
