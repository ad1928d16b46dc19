"""Packed-bit storage (storage="bits"): call latency of cosine / euclidean top-100 and hamming top-100 through rank_batch on (a) a
bits index, (b) a storage="int8" index over the same 0/1 values -- the best the library offered this data before -- and, for
hamming, (c) a float16 index over the same values at its defaults (the bit metrics read the sign cache either way).

p50 over --calls synchronous calls per index, metric and query count (host queries in, host results out), after --warmup calls of
the same shape.  The contenders take turns call by call, so drift of the clock or of the machine hits all of them alike; the bits
index takes two turns per round ((a) and (a')) and the difference of their two medians is the run-to-run spread the other columns
are read against.  Shapes: --shapes rows x bits pairs (default 10M x 384, 2M x 384, 10M x 1024, 2M x 1024); a contender that does
not fit the device's free memory beside the others is dropped and its columns read "-".

    python tools/time_b1.py [--shapes 10000000x384 2000000x384 ...] [--calls 60] [--warmup 5] --out profiles/b1_time.txt

--trace ROWSxBITS: no table; 30 one-query cosine top-100 calls on a bits index of that shape, for a kernel-trace run of its own
(the filter pass is the hdb_bscan_kernel launch over all rows: rows x (d/8 + 4) bytes / its time).
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
METRICS = ("cosine_similarity", "euclidean_metric", "hamming_distance")


def packed_rows(n, d, dev):
    """Random packed rows (little bit order), uint8 [n, d/8] on the device."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    out = torch.empty((n, d // 8), dtype=torch.uint8, device=dev)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        out[r0:r0 + m] = torch.randint(0, 256, (m, d // 8), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
    return out


def widened(packed, d, dtype):
    """The 0/1 values of the packed rows as `dtype` [n, d] on the device, or None when the device has no room for them."""
    n = packed.shape[0]
    free_b, _ = torch.cuda.mem_get_info(packed.device)
    if n * d * torch.empty((), dtype=dtype).element_size() + (4 << 30) > free_b:
        return None
    out = torch.empty((n, d), dtype=dtype, device=packed.device)
    sh = torch.arange(8, device=packed.device, dtype=torch.int32)
    for r0 in range(0, n, CHUNK):
        p = packed[r0:r0 + CHUNK].to(torch.int32)
        out[r0:r0 + CHUNK] = ((p.unsqueeze(-1) >> sh) & 1).reshape(p.shape[0], d).to(dtype)
    return out


def one_call(ranking, h, Q, metric):
    t0 = time.perf_counter()
    ranking.rank_batch(h, Q, top_k=100, metric=metric)
    return (time.perf_counter() - t0) * 1e6


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_b1.py: top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a), (a') bits index, two turns per round (spread = |a - a'| / a)   (b) storage=\"int8\" index   (c) float16 index (hamming only); the same 0/1 values in all three",
             f"# {'rows':>10} {'bits':>5} {'metric':>18} {'queries':>7} {'(a) bits':>9} {'(a) again':>9} {'spread':>7} {'(b) i8':>9} {'(c) f16':>9} {'(b)/(a)':>8} {'(c)/(a)':>8}"]
    for n, d in a.shapes:
        packed = packed_rows(n, d, dev)
        hs = [ranking.register_vectors(packed, storage="bits", bitorder="little")]
        assert hs[0].index.dtype == 10 and hs[0].index.V.numel() == n * d // 8
        i8 = widened(packed, d, torch.int8)
        hs.append(ranking.register_vectors(i8, storage="int8") if i8 is not None else None)
        f16 = widened(packed, d, torch.float16)
        hs.append(ranking.register_vectors(f16) if f16 is not None else None)
        rng = np.random.default_rng(7)
        for metric in METRICS:
            order = [0, 1, 2, 0] if metric == "hamming_distance" else [0, 1, 0]
            order = [i for i in order if hs[i] is not None]
            for nq in a.queries:
                Q = rng.standard_normal((nq, d)).astype(np.float32)
                Q /= np.linalg.norm(Q, axis=1, keepdims=True)
                for _ in range(a.warmup):
                    for i in set(order):
                        one_call(ranking, hs[i], Q, metric)
                t = {slot: [] for slot in range(len(order))}
                for _ in range(a.calls):
                    for slot, i in enumerate(order):
                        t[slot].append(one_call(ranking, hs[i], Q, metric))
                p = {slot: float(np.median(x)) for slot, x in t.items()}
                pa, pa2 = p[0], p[len(order) - 1]
                by = {i: p[slot] for slot, i in enumerate(order) if i != 0}
                col = lambda i: f"{by[i]:>9.1f}" if i in by else f"{'-':>9}"
                rat = lambda i: f"{by[i] / pa:>8.2f}" if i in by else f"{'-':>8}"
                lines.append(f"  {n:>10} {d:>5} {metric:>18} {nq:>7} {pa:>9.1f} {pa2:>9.1f} {abs(pa - pa2) / pa:>7.3f} {col(1)} {col(2)} {rat(1)} {rat(2)}")
                print(lines[-1], flush=True)
        for h in hs:
            if h is not None:
                h.close()
        del packed, i8, f16, hs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def trace_calls(n, d):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    h = ranking.register_vectors(packed_rows(n, d, dev), storage="bits", bitorder="little")
    q = np.random.default_rng(7).standard_normal((1, d)).astype(np.float32)
    for _ in range(30):
        ranking.rank_batch(h, q, top_k=100, metric="cosine_similarity")
    print(f"traced 30 one-query cosine top-100 calls on {n} x {d} bits: the filter pass reads {n * (d // 8 + 4)} bytes")
    h.close()


def shape(text):
    n, d = text.lower().split("x")
    return int(n), int(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=shape, nargs="*", default=[(10_000_000, 384), (2_000_000, 384), (10_000_000, 1024), (2_000_000, 1024)])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--trace", type=shape, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_b1.py measures on the GPU"
    if a.trace:
        trace_calls(*a.trace)
        return
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
