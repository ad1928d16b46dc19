"""MXFP4 rows wider than 512 elements on the bf16 matrix cores (set_option("b1_mfma_min_q", 5) with set_option("f8_ks_min_q", 5) on a
storage="mxfp4" index, csrc/hdb_mfma_f4_wide.h): call latency of top-100 through rank_batch on
  (a)  the MXFP4 index with both options on: the waves of a workgroup split K, one launch,
  (v)  the SAME handle with both options at 0: the VALU scan's passes (two queries per pass up to d = 1024, one beyond) -- the
       behaviour without the options, so the yardstick,
  (f)  a bfloat16 index over the same values (random e2m1 codes under scale byte 128: the integers {0, +-1 .. +-12}) through its K
       slices,
  (s)  a storage="bits" index over the signs of those values with b1_mfma_min_q = 5 (its K slices).

The protocol of tools/time_f4_mfma.py: p50 over --calls synchronous calls per contender and query count (host queries in, host
results out), after --warmup calls of the same shape; the contenders take turns call by call, so drift of the clock or of the machine
hits all of them alike; (a) takes two turns per round ((a) and (a')) and the difference of their two medians is the run-to-run
spread the other columns are read against.  A contender that does not fit the device's free memory is dropped: "-".  Cosine at
every shape, euclidean at the first.  The rule hdb_mfma_f4_wide_min_q (csrc/hdb_caps.h) is derived from the (v)/(a) column.

    python tools/time_f4_wide.py [--shapes 2000000x768 ...] [--queries 5 8 16 64 128] [--calls 60] --out profiles/f4_wide_time.txt
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

CHUNK = 500_000
SHAPES = [(2_000_000, 768), (2_000_000, 1024), (1_000_000, 1536), (2_000_000, 2048), (375_000, 4096), (10_000_000, 1024)]


def make_matrices(n, d, dev):
    """Random code bytes -> (codes, scales) of the MXFP4 index, the same values as bfloat16 (or None: no room) and their signs
    packed little bit first, CHUNK rows at a time."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    mags = torch.tensor([0, 1, 2, 3, 4, 6, 8, 12], dtype=torch.float32)
    table = torch.cat([mags, -mags]).to(dev)                            # the value of code c under scale byte 128
    pow2 = (2 ** torch.arange(8, device=dev)).to(torch.int32)
    free_b, _ = torch.cuda.mem_get_info(dev)
    codes = torch.empty((n, d // 2), dtype=torch.uint8, device=dev)
    bits = torch.empty((n, d // 8), dtype=torch.uint8, device=dev)
    bf = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if n * d * 2 + (8 << 30) < free_b else None
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        c = torch.randint(0, 256, (m, d // 2), generator=g, device=dev, dtype=torch.int32)
        codes[r0:r0 + m] = c.to(torch.uint8)
        v = table[torch.stack([c & 15, c >> 4], dim=-1).reshape(m, d)]
        if bf is not None:
            bf[r0:r0 + m] = v.to(torch.bfloat16)
        bits[r0:r0 + m] = ((v > 0).to(torch.int32).reshape(m, d // 8, 8) * pow2).sum(-1).to(torch.uint8)
    return codes, torch.full((n, d // 32), 128, dtype=torch.uint8, device=dev), bf, bits


def turn(ranking, h, opts, Q, metric, mfma):
    for name, value in opts:                                            # (outside the timed call)
        h.index.set_option(name, value)
    t0 = time.perf_counter()
    ranking.rank_batch(h, Q, top_k=100, metric=metric)
    us = (time.perf_counter() - t0) * 1e6
    assert mfma is None or h.index.stat("mfma") == mfma, (opts, h.index.stat("mfma"))
    return us


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_f4_wide.py: top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a), (a') MXFP4 index, b1_mfma_min_q = 5 and f8_ks_min_q = 5, two turns per round (spread = |a - a'| / a)   (v) the same handle, both options 0 (VALU passes)   "
             "(f) bfloat16 index, the same values (K slices)   (s) bits index over the signs, b1_mfma_min_q = 5 (K slices)",
             f"# {'rows':>10} {'d':>5} {'metric':>9} {'queries':>7} {'(a) wide':>9} {'(a) again':>9} {'spread':>7} {'(v) valu':>9} {'(f) bf16':>9} {'(s) bits':>9} {'(v)/(a)':>8} {'(f)/(a)':>8} {'(s)/(a)':>8}"]
    print("\n".join(lines), flush=True)
    on, off = (("b1_mfma_min_q", 5), ("f8_ks_min_q", 5)), (("b1_mfma_min_q", 0), ("f8_ks_min_q", 0))
    for at, (n, d) in enumerate(a.shapes):
        codes, scales, bf, bits = make_matrices(n, d, dev)
        h4 = ranking.register_vectors((codes, scales), storage="mxfp4")
        hf = ranking.register_vectors(bf) if bf is not None else None
        hs = ranking.register_vectors(bits, storage="bits", bitorder="little")
        hs.index.set_option("b1_mfma_min_q", 5)
        assert h4.index.dtype == 13 and hs.index.dtype == 10
        del codes, scales, bf, bits
        turns = [("a", h4, on, 1), ("v", h4, off, 0), ("f", hf, (), None), ("s", hs, (), None), ("a2", h4, on, 1)]
        turns = [t for t in turns if t[1] is not None]
        rng = np.random.default_rng(7)
        for metric in ("cosine_similarity", "euclidean_metric") if at == 0 else ("cosine_similarity",):
            for nq in a.queries:
                Q = rng.standard_normal((nq, d)).astype(np.float32)
                for _ in range(a.warmup):
                    for _, h, opts, mfma in turns[:-1]:
                        turn(ranking, h, opts, Q, metric, mfma)
                t = {name: [] for name, _, _, _ in turns}
                for _ in range(a.calls):
                    for name, h, opts, mfma in turns:
                        t[name].append(turn(ranking, h, opts, Q, metric, mfma))
                p = {name: float(np.median(x)) for name, x in t.items()}
                col = lambda c: f"{p[c]:>9.1f}" if c in p else f"{'-':>9}"
                rat = lambda c: f"{p[c] / p['a']:>8.2f}" if c in p else f"{'-':>8}"
                lines.append(f"  {n:>10} {d:>5} {metric.split('_')[0]:>9} {nq:>7} {p['a']:>9.1f} {p['a2']:>9.1f} {abs(p['a'] - p['a2']) / p['a']:>7.3f} "
                             f"{col('v')} {col('f')} {col('s')} {rat('v')} {rat('f')} {rat('s')}")
                print(lines[-1], flush=True)
                if a.out:                                        # (kept current line by line: a run cut short leaves what it measured)
                    with open(a.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
        for h in (h4, hf, hs):
            if h is not None:
                h.close()
        del h4, hf, hs, turns
        torch.cuda.empty_cache()


def shape(text):
    n, d = text.lower().split("x")
    return int(n), int(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=shape, nargs="*", default=SHAPES)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[5, 8, 16, 64, 128])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_f4_wide.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
