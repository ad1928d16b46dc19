"""Record which path hdb_topk takes: one call per row on ONE GPU, one JSON line per row -> tests/golden/dispatch_table.jsonl.

usage: python tools/dispatch_table.py OUT.jsonl [--max-n N] [--all-stats]        (HYPERDB_HIP_LIB selects the library)

A line holds the call -- "call": "dtype d n nq k metric" -- and, where they are not zero, exact requested, mask / bias present, a
matrix with a NaN row (nonfinite), what the index held before the call (pre_shadow, pre_auto, pre_plane) and the options set
("opt.<name>"); then "stats", the statistics in the order the header line names, where the header also holds the CU count.  A
statistic the path of the call leaves untouched is "-": the full sort (k > 2048) writes no fused / local / sample_rows /
sample_m, a call on an empty matrix writes quant and plane only.
One process; one matrix per (dtype, d), sliced to the row counts of its rows, reused over all their calls.
tests/test_topk_plan.py replays the table through plan_topk on the host; a GPU test replays its short rows on the live library."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

HEADER = ("dispatch of hdb_topk, one call per line; a stat the path does not write is -.  The widest default rule "
          "(d = 512 batches through the shadow from 10M rows) is reached through quant_batch_min_n on a 2M-row matrix, not through a "
          "10M-row one")
DTYPES = {"f16": 0, "f32": 1, "f64": 2, "bf16": 3}
METRICS = {"dot": 0, "cosine": 1, "euclidean": 2, "hamming": 3, "manhattan": 4, "jaccard": 5, "pearson": 6}
STATS = ("path", "fused", "local", "mfma", "f32_split", "quant", "quant_auto", "plane", "chunks", "sample_rows", "sample_m")


def rows():
    """(dtype, d, n, nq, k, metric, extras) in recording order; extras: exact, mask, bias, shadow ("explicit"), finite, opts."""
    out = []

    def add(dtype, d, n, nq, k, metric, **kw):
        out.append((dtype, d, n, nq, k, metric, kw))

    # ---- fp16 d = 384: the flagship shape ----
    for nq, k in ((1, 10), (5, 100), (300, 3000)):
        add("f16", 384, 0, nq, k, "cosine")
    for nq in (1, 2, 3, 4, 5, 16, 17, 24, 25, 128, 129, 256, 257):
        add("f16", 384, 70001, nq, 100, "cosine")
    for n in (8192, 8193):
        for nq in (1, 5, 257):
            add("f16", 384, n, nq, 100, "cosine")
    for n in (8193, 70001):
        for k in (1, 128, 129, 2048, 2049):
            add("f16", 384, n, 1, k, "dot")
    for k in (1, 128, 129, 2048, 2049):
        add("f16", 384, 70001, 8, k, "euclidean")
    for n in (8192, 70001):
        for metric in METRICS:
            for nq in (1, 5):
                add("f16", 384, n, nq, 100, metric)
    add("f16", 384, 70001, 4, 100, "hamming")
    for n in (65535, 65536):                           # 32 k > n at k = 2048
        for nq in (1, 8):
            add("f16", 384, n, nq, 2048, "dot")
            add("f16", 384, n, nq, 2048, "hamming")
    for n in (8223, 8224):                             # ... and at k = 257
        add("f16", 384, n, 1, 257, "cosine")
    for metric in ("cosine", "hamming"):
        for nq in (1, 5):
            add("f16", 384, 70001, nq, 100, metric, exact=True)
            add("f16", 384, 70001, nq, 100, metric, mask=True)
            add("f16", 384, 70001, nq, 100, metric, bias=True)
            add("f16", 384, 70001, nq, 100, metric, opts={"force_exact": 1})
    for opts in ({"use_fused": 0}, {"use_local": 0}, {"use_mfma": 0}, {"use_batch1": 0}, {"local_max_q": 4}, {"max_blocks": 64},
                 {"fused_max_q": 4}, {"mfma_min_q": 3}, {"bits_fused": 0}, {"bits_local": 0}, {"bits_max_q": 8}, {"sample_target": 1000},
                 {"exact_bytes": 1 << 20}):
        for metric, nq in (("cosine", 1), ("cosine", 8), ("hamming", 1)):
            add("f16", 384, 70001, nq, 100, metric, opts=opts)
    for nq in (1, 3):
        add("f16", 384, 8192, nq, 100, "cosine", opts={"local_small": 1})
        add("f16", 384, 70001, nq, 100, "manhattan", opts={"use_l1_tile": 0})
    # hamming: bits_fused = 3 keeps one-query calls on 1M+ rows with the six launches
    for n in (999999, 1000000):
        for nq in (1, 2, 5):
            add("f16", 384, n, nq, 100, "hamming", opts={"bits_fused": 3})
            add("f16", 384, n, nq, 100, "jaccard")
    # the explicit shadow: fp16 from 1.25M rows
    for n in (1249999, 1250000):
        for nq, k, metric in ((1, 100, "cosine"), (4, 128, "dot"), (2, 100, "euclidean"), (5, 100, "cosine"), (1, 129, "cosine"), (1, 100, "manhattan")):
            add("f16", 384, n, nq, k, metric, shadow="explicit")
    add("f16", 384, 70001, 1, 100, "cosine", shadow="explicit")
    add("f16", 384, 70001, 1, 100, "cosine", shadow="explicit", opts={"quant_min_n": 0})
    add("f16", 384, 70001, 1, 100, "cosine", shadow="explicit", opts={"quant_min_n": 0, "use_quant": 0})
    add("f16", 384, 70001, 1, 100, "cosine", shadow="explicit", opts={"quant_min_n": 0, "quant_max_k": 64})
    add("f16", 384, 70001, 1, 100, "cosine", shadow="explicit", opts={"quant_min_n": 0}, exact=True)
    # fused_max_q: three queries join the one-wave single launch from 1.5M rows
    for n in (1499999, 1500000):
        for nq in (1, 3, 4):
            add("f16", 384, n, nq, 100, "cosine")
    # the automatic shadow and its plane from 2M rows; batches from 3M (5-16 queries) / 5M (17-24 queries)
    for n, nqs in ((1999999, (1, 4, 5)), (2000000, (1, 4, 5)), (2999999, (4, 5, 16, 17)), (3000000, (4, 5, 16, 17)),
                   (4999999, (16, 17, 24, 25)), (5000000, (16, 17, 24, 25))):
        for nq in nqs:
            add("f16", 384, n, nq, 100, "cosine")
    add("f16", 384, 2000000, 1, 129, "dot")
    for opts in ({"auto_quant": 0}, {"use_quant": 0}, {"use_plane": 0}, {"plane_min_n": 4000000}, {"quant_batch_kernel": 0}, {"mfma_variant": 32},
                 {"max_blocks": 64}, {"quant_batch_min_n": 0}, {"quant_min_n": 2500000}):
        for nq in (1, 8):
            add("f16", 384, 3000000, nq, 100, "cosine", opts=opts)
    for opts in ({"quant_min_n": 0}, {"quant_min_n": 0, "plane_min_n": 0}, {"quant_batch_min_n": 0}):
        for nq in (1, 8, 300):
            add("f16", 384, 70001, nq, 100, "dot", opts=opts)
    # ---- other fp16 widths ----
    for d in (40, 128, 256, 512, 640, 768, 896, 1024, 2048):
        for nq in (1, 2, 5, 129, 257):
            add("f16", d, 20000, nq, 100, "cosine")
        add("f16", d, 20000, 1, 100, "euclidean")
        add("f16", d, 70001, 1, 100, "cosine")
    for n in (4000000, 4000001):                       # fp16 d = 1024: the single launch up to 4M rows
        for nq in (1, 2):
            add("f16", 1024, n, nq, 100, "cosine")
    for n in (1999999, 2000000):                       # d = 512: one to four queries from 2M rows, batches by the 10M rule
        for nq in (1, 5, 17):
            add("f16", 512, n, nq, 100, "dot")
            add("f16", 512, n, nq, 100, "dot", opts={"quant_batch_min_n": 2000000})
    # ---- float32 ----
    for nq in (1, 2, 3, 4, 5, 8, 9, 16, 64, 65, 128, 129, 256, 257):
        add("f32", 384, 70001, nq, 100, "cosine")
    for nq in (1, 5):
        add("f32", 384, 8192, nq, 100, "cosine")
    for metric in METRICS:
        add("f32", 384, 70001, 2, 100, metric)
    add("f32", 384, 70001, 16, 100, "cosine", opts={"f32_split": 0})
    add("f32", 384, 70001, 4, 100, "cosine", opts={"f32_min_q": 2})
    add("f32", 384, 70001, 4, 100, "cosine", opts={"f32_split_min_q": 4, "f32_min_q": 2})
    add("f32", 384, 70001, 16, 2049, "cosine")
    for n in (299999, 300000):                         # three or four queries take the batched single launch from 300k rows
        for nq in (2, 3):
            add("f32", 384, n, nq, 100, "dot")
    for n in (499999, 500000):                         # the explicit shadow: float32 from 500k rows
        for nq in (1, 5):
            add("f32", 384, n, nq, 100, "cosine", shadow="explicit")
    for n in (1499999, 1500000):                       # float32 d = 512: the single launch from 1.5M rows
        for nq in (1, 2):
            add("f32", 512, n, nq, 100, "cosine")
    for d in (40, 512, 1024):
        for nq in (1, 5, 64, 65):
            add("f32", d, 20000, nq, 100, "cosine")
    add("f32", 384, 20000, 16, 100, "cosine", finite=False)
    add("f32", 384, 20000, 2, 100, "cosine", finite=False)
    # float32 batches as bf16 parts: cosine / euclidean / pearson, never dot_product, never a call that asks for the exact selection
    for nq in (16, 64):
        for metric in ("dot", "euclidean", "pearson"):
            add("f32", 384, 70001, nq, 100, metric)
    add("f32", 384, 70001, 16, 100, "cosine", exact=True)
    add("f32", 384, 70001, 16, 100, "dot", exact=True)
    add("f32", 384, 70001, 16, 100, "dot", opts={"f32_split": 0})
    for d, nq in ((768, 8), (1024, 16)):
        for metric in ("dot", "cosine"):
            add("f32", d, 20000, nq, 100, metric)
    # widths that ride a wider geometry (fp16 d = 96 -> 128, float32 d = 100 -> 128, d = 300 -> 384): the matrix cores on a finite matrix only
    for dtype, d in (("f16", 96), ("f32", 100), ("f32", 300)):
        for nq in (6, 40):
            for metric in ("dot", "cosine"):
                add(dtype, d, 20000, nq, 100, metric)
                add(dtype, d, 20000, nq, 100, metric, finite=False)
    # ---- bfloat16, float64 ----
    for d in (40, 384, 512):
        for nq in (1, 5, 129):
            add("bf16", d, 20000, nq, 100, "cosine")
        add("bf16", d, 20000, 8, 100, "hamming")
    add("bf16", 384, 20000, 8, 100, "cosine", finite=False)
    add("bf16", 384, 20000, 8, 2049, "cosine")
    for metric in ("dot", "hamming", "manhattan"):
        for nq in (1, 5):
            add("f64", 384, 20000, nq, 100, metric)
    add("f64", 384, 8192, 1, 100, "dot")
    add("f64", 384, 20000, 2, 2049, "dot")
    return out


def record(max_n=None, all_stats=False):
    """Run the rows with n <= max_n on cuda:0 -> the table's lines as dicts, header first.  all_stats: also the statistics a path
    does not define (to see what a library leaves in them)."""
    import torch
    from hyperdb._native import GpuIndex

    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tdt = {"f16": torch.float16, "f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
    todo = [r for r in rows() if max_n is None or r[2] <= max_n]
    groups = {}
    for r in todo:
        groups.setdefault((r[0], r[1], r[6].get("finite", True)), []).append(r)
    lines = [{"header": HEADER, "rows": len(todo), "cus": cus, "stats": " ".join(STATS)}]
    for (dtype, d, finite), grp in groups.items():
        nmax = max(r[2] for r in grp)
        gen = torch.Generator(device=dev); gen.manual_seed(d * 7 + DTYPES[dtype])
        base = torch.empty((max(nmax, 1), d), dtype=tdt[dtype], device=dev)
        step = 1 << 20                                  # (in pieces: no float32 temporary of the whole matrix)
        for r0 in range(0, nmax, step):
            base[r0:r0 + step].copy_(torch.randn((min(step, nmax - r0), d), generator=gen, device=dev, dtype=torch.float32))
        if not finite:
            base[5, 3] = float("nan")
        grp.sort(key=lambda r: (r[2], json.dumps(r[6].get("opts", {}), sort_keys=True), r[6].get("shadow", "")))
        ix, ix_key = None, None
        for dtype, d, n, nq, k, metric, kw in grp:
            opts = kw.get("opts", {})
            key = (n, json.dumps(opts, sort_keys=True), kw.get("shadow", ""))
            if key != ix_key:
                if ix is not None:
                    ix.close()
                ix = GpuIndex(base[:n], device=dev)
                for name, value in opts.items():
                    ix.set_option(name, value)
                if kw.get("shadow") == "explicit":
                    ix.quantize("int8")
                ix_key = key
            ix.set_row_mask((torch.arange(n, device=dev) % 3 != 0).to(torch.uint8) if kw.get("mask") else None)
            ix.set_bias(torch.full((n,), 0.5, device=dev) if kw.get("bias") else None)
            row = {"call": f"{dtype} {d} {n} {nq} {k} {metric}"}
            flags = {"exact": int(bool(kw.get("exact"))), "mask": int(bool(kw.get("mask"))), "bias": int(bool(kw.get("bias"))),
                     "nonfinite": int(not finite), "pre_shadow": int(ix.stat("quant_bytes") > 0), "pre_auto": ix.stat("quant_auto"),
                     "pre_plane": int(ix.stat("plane_bytes") > 0)}
            row.update({name: v for name, v in flags.items() if v})
            for name, value in sorted(opts.items()):
                row["opt." + name] = value
            Q = torch.randn((nq, d), generator=gen, device=dev, dtype=torch.float32).to(torch.float64 if dtype == "f64" else torch.float32)
            ix.topk_device(Q, k, METRICS[metric], exact=bool(kw.get("exact")))
            torch.cuda.synchronize(dev)
            defined = STATS
            if n == 0 and not all_stats:
                defined = ("quant", "plane")
            elif k > 2048 and n > 8192 and not all_stats:
                defined = tuple(s for s in STATS if s not in ("fused", "local", "sample_rows", "sample_m"))
            row["stats"] = " ".join(str(ix.stat(s)) if s in defined else "-" for s in STATS)
            lines.append(row)
        if ix is not None:
            ix.close()
        del base
        torch.cuda.empty_cache()
    return lines


def main():
    max_n = int(sys.argv[sys.argv.index("--max-n") + 1]) if "--max-n" in sys.argv else None
    lines = record(max_n, "--all-stats" in sys.argv)
    with open(sys.argv[1], "w") as fh:
        fh.write("".join(json.dumps(line) + "\n" for line in lines))
    print(f"{len(lines) - 1} rows -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
