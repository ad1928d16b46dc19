"""The opt-in int8 shadow of a bfloat16 index (option bf16_quant): call latency of cosine top-100 on ONE bfloat16 handle that holds a
shadow with its 5-bit plane, alternating call by call between
  (s)  use_quant = 1, the plane on (plane_min_n = 0: at every size),
  (s') the same again -- the difference of the two medians is the run-to-run spread the other columns are read against,
  (p)  use_quant = 1, use_plane = 0 (the int8 pass over every row),
  (v)  use_quant = 0: the VALU scan, i.e. the handle without its shadow and the library before the option,
and (c) an fp16 index at its defaults over the same values (every bfloat16 value of magnitude 2^-14 .. 65504 is an fp16 number; it
serves large matrices from its own automatic shadow) as a reference.  The contenders take turns call by call, so drift of the clock or
of the machine hits all of them alike.  p50 over --calls synchronous calls (rank_batch: host queries in, host results out) after
--warmup calls of the same shape.

Sizes: --rows at d = 384 and --side-rows at d = 128 / 256 / 512 / 768; 1 and 4 queries each.  At the largest d = 384 size the one-off
build time of the shadow (quantize("int8"), synchronised) and quant_bytes + plane_bytes are recorded.

The rule (quant_min_rows(HDB_BF16), csrc/hdb_plan.h): the smallest measured n at d = 384 from which the shadow beats (v) by at least
5 % in both of two runs, at that size and every larger one, for 1 and for 4 queries.  The shadow's column is the one the default
options take at that size: (s) for one query from HDB_PLANE_MIN_ROWS (2M) rows on, (p) otherwise.  Each run prints its own candidate;
the rule is the larger of the two.

    python tools/time_bf16_quant.py [--runs 2] [--calls 60] [--warmup 5] --out profiles/bf16_quant_time.txt
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
PLANE_MIN_ROWS = 2_000_000            # HDB_PLANE_MIN_ROWS (csrc/hdb_plan.h)


def make_matrices(n, d, dev):
    """Gaussian rows rounded to bfloat16, generated on the device a million rows at a time, and the same values as fp16."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    vb = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    vh = torch.empty((n, d), dtype=torch.float16, device=dev)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        x = torch.randn((m, d), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
        vb[r0:r0 + m] = x
        vh[r0:r0 + m] = x.to(torch.float16)
    return vb, vh


def one_call(ranking, h, Q):
    t0 = time.perf_counter()
    ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")
    return (time.perf_counter() - t0) * 1e6


# (name, use_quant, use_plane) of the bfloat16 handle's turns
TURNS = (("s", 1, 1), ("s'", 1, 1), ("p", 1, 0), ("v", 0, 1))


def run_table(a, run, lines):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines.append(f"# run {run}")
    lines.append(f"# {'rows':>10} {'d':>4} {'queries':>7} {'(s) plane':>9} {'(s) again':>9} {'spread':>7} {'(p) int8':>9} {'(v) valu':>9} {'(c) fp16':>9} "
                 f"{'(v)/(s)':>8} {'(v)/(p)':>8} {'(c)/(s)':>8}  quant s/p/v  plane s/p  cands  quant(c)")
    shapes = [(n, 384) for n in a.rows] + [(n, d) for n in a.side_rows for d in (128, 256, 512, 768)]
    wins = {}                                           # rows at d = 384 -> the shadow beats (v) by 5 % at 1 and at 4 queries
    for n, d in shapes:
        vb, vh = make_matrices(n, d, dev)
        hb = ranking.register_vectors(vb)
        hb.index.set_option("bf16_quant", 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hb.index.quantize("int8")
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        hb.index.set_option("quant_min_n", 0)
        hb.index.set_option("plane_min_n", 0)
        hc = ranking.register_vectors(vh)
        if d == 384 and n == max(a.rows):
            qb, pb = hb.index.stat("quant_bytes"), hb.index.stat("plane_bytes")
            lines.append(f"# {n} x {d}: shadow built in {build_ms:.1f} ms, quant_bytes {qb / 1e9:.2f} GB + plane_bytes {pb / 1e9:.2f} GB beside "
                         f"the {n * d * 2 / 1e9:.2f} GB matrix")
            print(lines[-1], flush=True)
        rng = np.random.default_rng(7)
        ok = True
        for nq in (1, 4):
            Q = rng.standard_normal((nq, d)).astype(np.float32)

            def turn(i):
                _, uq, up = TURNS[i]
                hb.index.set_option("use_quant", uq)
                hb.index.set_option("use_plane", up)
                return one_call(ranking, hb, Q)

            for _ in range(a.warmup):
                for i in range(len(TURNS)):
                    turn(i)
                one_call(ranking, hc, Q)
            t = [[] for _ in range(len(TURNS) + 1)]
            st = {}
            for _ in range(a.calls):
                for i in range(len(TURNS)):
                    t[i].append(turn(i))
                    st[TURNS[i][0]] = (hb.index.stat("quant"), hb.index.stat("plane"), hb.index.stat("quant_cands") if TURNS[i][1] else 0)
                t[-1].append(one_call(ranking, hc, Q))
            p = [float(np.median(x)) for x in t]
            lines.append(f"  {n:>10} {d:>4} {nq:>7} {p[0]:>9.1f} {p[1]:>9.1f} {abs(p[0] - p[1]) / p[0]:>7.3f} {p[2]:>9.1f} {p[3]:>9.1f} {p[4]:>9.1f} "
                         f"{p[3] / p[0]:>8.2f} {p[3] / p[2]:>8.2f} {p[4] / p[0]:>8.2f}  {st['s'][0]}/{st['p'][0]}/{st['v'][0]}        "
                         f"{st['s'][1]}/{st['p'][1]}      {st['s'][2]:>5}  {hc.index.stat('quant')}")
            print(lines[-1], flush=True)
            shadow = p[0] if (nq == 1 and n >= PLANE_MIN_ROWS) else p[2]          # the column the default options take at this size
            ok = ok and p[3] >= 1.05 * shadow
        if d == 384:
            wins[n] = ok
        hb.close()
        hc.close()
        del vb, vh, hb, hc
        torch.cuda.empty_cache()
    cand = None
    for n in sorted(wins, reverse=True):
        if not wins[n]:
            break
        cand = n
    lines.append(f"# run {run}: the shadow beats (v) by at least 5 % at 1 and at 4 queries, at that size and every larger one, from "
                 f"{cand if cand is not None else 'no measured size'} rows on (d = 384)")
    print(lines[-1], flush=True)
    return cand


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[250_000, 500_000, 1_000_000, 1_250_000, 2_000_000, 5_000_000, 10_000_000])
    ap.add_argument("--side-rows", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_bf16_quant.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    lines = [f"# tools/time_bf16_quant.py: cosine top-100 through rank_batch, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# ONE bfloat16 handle with bf16_quant = 1, quantize(\"int8\"), quant_min_n = 0, plane_min_n = 0:",
             "# (s), (s') use_quant = 1, plane on, two turns per round (spread = |s - s'| / s)   (p) use_quant = 1, use_plane = 0"
             "   (v) use_quant = 0 (the VALU scan: the parent's path)   (c) an fp16 index at its defaults over the same values"]
    cands = []
    for run in range(1, a.runs + 1):
        cands.append(run_table(a, run, lines))
        if a.out:                                       # (kept after every run: a later run that is cut short loses nothing)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    rule = None if any(c is None for c in cands) else max(cands)
    lines.append(f"# rule (both runs): quant_min_rows(HDB_BF16) = {rule if rule is not None else 'never under -1 (no size satisfies the criterion)'}")
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
