"""Large MXFP4 batches on the bf16 matrix cores with the query parts in LDS (set_option("f8_lds_min_q", 5) beside
set_option("b1_mfma_min_q", 5) on a storage="mxfp4" index, csrc/hdb_mfma_f4_lds.h): call latency of cosine top-100 through rank_batch
on (a) an MXFP4 index with both options on, (r) the SAME handle with f8_lds_min_q = 0 -- the register flavour, csrc/hdb_mfma_f4.h --
and (b) a bfloat16 index over the same values (random e2m1 codes under scale byte 128: the integers {0, +-1, .. +-12}, which bf16
holds exactly).

p50 over --calls synchronous calls per contender and query count (host queries in, host results out), after --warmup calls of the
same shape.  The contenders take turns call by call, so drift of the clock or of the machine hits all of them alike; the LDS
contender takes two turns per round ((a) and (a')) and the difference of their two medians is the run-to-run spread the other columns
are read against.  Shapes: --rows (default 10M) at d = 384 and --side-rows (default 2M) at d = 128 / 256 / 384 / 512.

    python tools/time_f4_lds.py [--rows 10000000] [--side-rows 2000000] [--calls 60] [--warmup 5] --out profiles/f4_lds_time.txt
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
METRIC = "cosine_similarity"


def make_matrices(n, d, dev):
    """Random code bytes on the device -> (codes, scales) for the MXFP4 index and the same values as bfloat16, a million rows at a time."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    mags = torch.tensor([0, 1, 2, 3, 4, 6, 8, 12], dtype=torch.bfloat16)
    table = torch.cat([mags, -mags]).to(dev)                        # the value of code c under scale byte 128
    codes = torch.empty((n, d // 2), dtype=torch.uint8, device=dev)
    bf = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        c = torch.randint(0, 256, (m, d // 2), generator=g, device=dev, dtype=torch.int32)
        codes[r0:r0 + m] = c.to(torch.uint8)
        bf[r0:r0 + m] = table[torch.stack([c & 15, c >> 4], dim=-1).reshape(m, d)]
    return codes, torch.full((n, d // 32), 128, dtype=torch.uint8, device=dev), bf


def one_call(ranking, h, Q, option):
    if option is not None:
        h.index.set_option("f8_lds_min_q", option)
    t0 = time.perf_counter()
    ranking.rank_batch(h, Q, top_k=100, metric=METRIC)
    return (time.perf_counter() - t0) * 1e6, f"{h.index.stat('mfma')}{h.index.stat('f8_lds')}"


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_f4_lds.py: cosine top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a), (a') MXFP4 index, b1_mfma_min_q = f8_lds_min_q = 5, two turns per round (spread = |a - a'| / a)   (r) the same handle, f8_lds_min_q = 0   (b) bfloat16 index, the same values",
             f"# {'rows':>10} {'d':>5} {'queries':>7} {'(a) lds':>9} {'(a) again':>9} {'spread':>7} {'(r) regs':>9} {'(b) bf16':>9} {'(r)/(a)':>8} {'(b)/(a)':>8}  mfma+f8_lds a/r/b"]
    shapes = [(n, 384) for n in a.rows] + [(n, d) for n in a.side_rows for d in (128, 256, 384, 512)]
    for n, d in shapes:
        torch.cuda.empty_cache()
        codes, scales, bf = make_matrices(n, d, dev)
        f4, bfh = ranking.register_vectors((codes, scales), storage="mxfp4"), ranking.register_vectors(bf)
        del codes, scales, bf
        assert f4.index.dtype == 13 and bfh.index.dtype != 13
        f4.index.set_option("b1_mfma_min_q", 5)
        turns = [(f4, 5), (f4, 0), (bfh, None), (f4, 5)]                 # (a) (r) (b) (a')
        rng = np.random.default_rng(7)
        for nq in a.queries:
            Q = rng.standard_normal((nq, d)).astype(np.float32)
            for _ in range(a.warmup):
                for h, option in turns:
                    one_call(ranking, h, Q, option)
            t = [[], [], [], []]
            st = ["", "", "", ""]
            for _ in range(a.calls):
                for slot, (h, option) in enumerate(turns):
                    us, st[slot] = one_call(ranking, h, Q, option)
                    t[slot].append(us)
            p = [float(np.median(x)) for x in t]
            lines.append(f"  {n:>10} {d:>5} {nq:>7} {p[0]:>9.1f} {p[3]:>9.1f} {abs(p[0] - p[3]) / p[0]:>7.3f} {p[1]:>9.1f} {p[2]:>9.1f} "
                         f"{p[1] / p[0]:>8.2f} {p[2] / p[0]:>8.2f}  {st[0]}/{st[1]}/{st[2]}")
            print(lines[-1], flush=True)
            if a.out:                                    # (kept current line by line: a run cut short leaves what it measured)
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
        f4.close()
        bfh.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[10_000_000])
    ap.add_argument("--side-rows", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[16, 32, 64, 128, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_f4_lds.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
