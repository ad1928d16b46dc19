"""float8 e4m3 storage: call latency of cosine top-100 on (a) a float8 index, (b) a bfloat16 index and (c) an fp16 index at its
defaults (so a large fp16 index serves its calls from its int8 shadow and 5-bit plane) over the SAME values -- every float8 code
widens exactly to both wider formats -- and (v) a second float8 index over the same tensor with use_mfma = 0, which keeps every
batch on the VALU scan: the (v) / (a) column at 5 and 8 queries is what the planner's first matrix-core batch size is read from.

Latency table (the default mode).  p50 over --calls synchronous calls per index and query count (hyperDB_ranking_algorithm_sort for
one query, rank_batch for more: host queries in, host results out), after --warmup calls of the same shape.  The contenders take
turns call by call, so drift of the clock or of the machine hits all of them alike; the float8 index takes two turns per round
((a) and (a')) and the difference of their two medians is the run-to-run spread the other columns are read against.  Sizes:
--rows (default 2M and 10M) at d = 384 and --side-rows at d = 128 / 256 / 512.

    python tools/time_f8.py [--rows 2000000 10000000] [--side-rows 2000000] [--calls 60] [--warmup 5] --out profiles/f8_time.txt

Kernel trace of the one-query passes (a second, separate run: tracing slows the host side of a call).  --trace-run is the workload:
one-query cosine top-100 calls on the float8 index and on an fp16 index with use_mfma = 0 and use_quant = 0 (its VALU pass);
--trace-report reads the kernel statistics of that run and appends the achieved TB/s of the two filter passes -- (row bytes + 4 bytes
of 1/||v||) x rows over the kernel's mean time -- to the table file.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/time_f8.py --trace-run --rows 10000000
    python tools/time_f8.py --trace-report DIR --rows 10000000 --out profiles/f8_time.txt
"""
import argparse
import csv
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

F8 = torch.float8_e4m3fn
CHUNK = 1_000_000


def make_matrices(n, d, dev, want=("f8", "bf16", "f16")):
    """Random float8 codes with the exponent's top bit clear (finite, magnitudes below 2) generated on the device as bytes, and the
    same values in the wider formats through a 256-entry table (each code widens exactly), a million rows at a time."""
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    codes = torch.randint(0, 256, (n, d), generator=g, device=dev, dtype=torch.uint8) & 0xBF
    lut = torch.arange(256, dtype=torch.uint8).view(F8).float()
    out = {"f8": codes.view(F8)}
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        if name not in want:
            continue
        table = lut.to(dt).to(dev)
        wide = torch.empty((n, d), dtype=dt, device=dev)
        for r0 in range(0, n, CHUNK):
            wide[r0:r0 + CHUNK] = table[codes[r0:r0 + CHUNK].long()]
        out[name] = wide
    return out


def one_call(ranking, h, Q):
    t0 = time.perf_counter()
    if Q.shape[0] == 1:
        ranking.hyperDB_ranking_algorithm_sort(h, Q[0], top_k=100, metric="cosine_similarity")
    else:
        ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")
    return (time.perf_counter() - t0) * 1e6


def latency_table(a):
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_f8.py: cosine top-100, p50 of {a.calls} calls in us (host queries in, host results out), {a.warmup} warm-up calls "
             "per shape, the contenders alternate call by call",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a), (a') float8 index, two turns per round (spread = |a - a'| / a)   (b) bfloat16 index   (c) fp16 index at its defaults"
             "   (v) float8 index, use_mfma = 0",
             f"# {'rows':>10} {'d':>4} {'queries':>7} {'(a) f8':>9} {'(a) again':>9} {'spread':>7} {'(b) bf16':>9} {'(c) fp16':>9} {'(v) valu':>9} {'(b)/(a)':>8} {'(c)/(a)':>8} {'(v)/(a)':>8}"
             "  mfma a/b/c/v  quant(c)"]
    shapes = [(n, 384) for n in a.rows] + [(n, d) for n in a.side_rows for d in (128, 256, 512)]
    for n, d in shapes:
        mats = make_matrices(n, d, dev)
        hs = [ranking.register_vectors(mats["f8"]), ranking.register_vectors(mats["bf16"]), ranking.register_vectors(mats["f16"]),
              ranking.register_vectors(mats["f8"])]
        hs[3].index.set_option("use_mfma", 0)
        order = [0, 1, 2, 0, 3]                          # (a) (b) (c) (a') (v)
        rng = np.random.default_rng(7)
        for nq in a.queries:
            Q = rng.standard_normal((nq, d)).astype(np.float32)
            for _ in range(a.warmup):
                for h in hs:
                    one_call(ranking, h, Q)
            t = [[], [], [], [], []]
            for _ in range(a.calls):
                for slot, i in enumerate(order):
                    t[slot].append(one_call(ranking, hs[i], Q))
            p = [float(np.median(x)) for x in t]
            st = [h.index.stat("mfma") for h in hs]
            lines.append(f"  {n:>10} {d:>4} {nq:>7} {p[0]:>9.1f} {p[3]:>9.1f} {abs(p[0] - p[3]) / p[0]:>7.3f} {p[1]:>9.1f} {p[2]:>9.1f} {p[4]:>9.1f} "
                         f"{p[1] / p[0]:>8.2f} {p[2] / p[0]:>8.2f} {p[4] / p[0]:>8.2f}  {st[0]}/{st[1]}/{st[2]}/{st[3]}       {hs[2].index.stat('quant')}")
            print(lines[-1], flush=True)
        for h in hs:
            h.close()
        del mats, hs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def trace_run(a):
    from hyperdb._native import GpuIndex, METRIC_IDS
    dev = torch.device("cuda", 0)
    n, d = a.rows[0], 384
    mats = make_matrices(n, d, dev, want=("f8", "f16"))
    f8, f16 = GpuIndex(mats["f8"]), GpuIndex(mats["f16"])
    for name in ("use_mfma", "use_quant", "use_fused"):
        f16.set_option(name, 0)
    Q = np.random.default_rng(7).standard_normal((1, d)).astype(np.float32)
    for _ in range(a.calls):
        f8.topk_views(Q, 100, METRIC_IDS["cosine_similarity"])
        f16.topk_views(Q, 100, METRIC_IDS["cosine_similarity"])
    torch.cuda.synchronize()
    print("float8: path", f8.stat("path"), "mfma", f8.stat("mfma"), " fp16: path", f16.stat("path"), "mfma", f16.stat("mfma"), "quant", f16.stat("quant"))


# the one-query filter pass (QT = 1, MODE = 1, dot accumulation) of an element type, in the mangled and the demangled spelling
_PASS = {"float8": (r"hdb_scan_kernelI6hdb_f8Li1ELi1ELi0E", r"hdb_scan_kernel<hdb_f8, 1, 1, 0,"),
         "fp16": (r"hdb_scan_kernelI6__halfLi1ELi1ELi0E", r"hdb_scan_kernel<__half, 1, 1, 0,")}


def trace_report(a):
    files = glob.glob(os.path.join(a.trace_report, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no *kernel_stats.csv under {a.trace_report}"
    rows = list(csv.DictReader(open(files[0], newline="")))
    n, d = a.rows[0], 384
    lines = [f"# kernel trace (rocprofv3 --kernel-trace --stats, a separate run): one cosine query, {n} rows x {d}, the filter pass over all rows;",
             "# achieved TB/s = rows x (row bytes + 4 bytes of 1/||v||) / mean kernel time",
             f"# {'pass':>8} {'calls':>6} {'mean us':>9} {'min us':>9} {'row bytes':>9} {'TB/s':>7}"]
    got = {}
    for name, (mangled, plain) in _PASS.items():
        hit = [r for r in rows if re.search(mangled, r["Name"]) or plain in r["Name"]]
        if not hit:
            lines.append(f"  {name:>8}  (no such kernel in the trace)")
            continue
        r = max(hit, key=lambda x: float(x["TotalDurationNs"]))
        rb = d * (1 if name == "float8" else 2)
        mean = float(r["AverageNs"])
        got[name] = n * (rb + 4) / mean / 1e3
        lines.append(f"  {name:>8} {int(r['Calls']):>6} {mean / 1e3:>9.1f} {float(r['MinNs']) / 1e3:>9.1f} {rb:>9} {got[name]:>7.2f}")
    if len(got) == 2:
        lines.append(f"# the float8 pass reaches {got['float8'] / got['fp16']:.2f} of the fp16 VALU pass's bytes per second")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2_000_000, 10_000_000])
    ap.add_argument("--side-rows", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 4, 5, 8, 16, 64, 128])
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-report", default=None)
    a = ap.parse_args()
    if a.trace_report:
        return trace_report(a)
    assert torch.cuda.is_available(), "time_f8.py measures on the GPU"
    if a.trace_run:
        return trace_run(a)
    assert a.calls >= 50, "p50 over at least 50 calls"
    latency_table(a)


if __name__ == "__main__":
    main()
