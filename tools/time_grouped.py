"""Grouped top-k (hdb_topk_grouped_host): call latency on one MI355X, cosine top-10 and top-100, 1 and 16 queries.

Two matrices of Gaussian rows, generated on the device from a seed: --rows16 x --dim float16 and --rows32 x --dim float32.  Groups are
contiguous runs of 1, 4 and 32 rows (a document's chunks are adjacent rows).  Per cell, alternating call by call:
    (g), (g')  GpuIndex.topk_grouped at the index's defaults, two turns per round -- the difference of their medians is the spread
               every other column is read against;
    (a)        the floor: GpuIndex.topk at the same k on the same handle (what rank_batch runs).  A grouped call answered in its first
               round is that call at k' = k * group_oversample plus one collapse launch and one status read-back;
    (b)        the only way to the answer before this entry point: hdb_scores per query, torch scatter_reduce(amax) over the group
               ids and torch.topk (it returns group ids, not rows, and writes and re-reads n floats per query);
    (x)        the exact grouped pass alone (group_fast_rounds = 0), over --exact-calls calls;
    (o2), (o8) topk_grouped with group_oversample = 2 and 8, to judge the default of 4.
Beside every grouped time the statistics of the call: rounds run, rows per query of the last round, queries answered exactly.
One huge group (every row in ONE group: no fast round can succeed, the exact pass answers) is timed separately at the end.

p50 over --calls synchronous calls (device queries in, host results out) after --warmup calls.  A cell loses to (a) only when it is
behind by more than the spread; nothing here is a pass condition.

    python tools/time_grouped.py [--rows16 10000000] [--rows32 2000000] [--dim 384] [--calls 60] --out profiles/grouped_time.txt
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


def build(n, d, dtype, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    V = torch.empty((n, d), dtype=dtype, device=dev)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        V[r0:r0 + m] = torch.randn((m, d), generator=g, device=dev, dtype=torch.float32).to(dtype)
    return V


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def rounds(contenders, calls, warmup):
    """contenders: list of (callable, calls or None).  They alternate call by call; -> p50 us per contender."""
    for fn, own in contenders:
        for _ in range(warmup if own is None else 1):
            fn()
    t = [[] for _ in contenders]
    for c in range(calls):
        for i, (fn, own) in enumerate(contenders):
            if own is not None and c >= own:
                continue
            t[i].append(timed(fn)[0])
    return [float(np.median(x)) for x in t]


def cells(a, lines, ix, name, Q):
    from hyperdb._native import METRIC_IDS
    cos = METRIC_IDS["cosine_similarity"]
    n, dev = ix.n, ix.device
    for size in a.group_sizes:
        groups = (torch.arange(n, device=dev, dtype=torch.int64) // size).to(torch.int32)
        g64 = groups.to(torch.int64)
        n_groups = (n + size - 1) // size
        ix.set_groups(groups, n_groups)
        for k in a.k:
            for nq in a.queries:
                Qd = Q[:nq].contiguous()
                stats = {}

                def grouped(tag, oversample=4, fast=2):
                    def run():
                        ix.set_option("group_oversample", oversample)
                        ix.set_option("group_fast_rounds", fast)
                        out = ix.topk_grouped(Qd, k, cos)
                        stats[tag] = (ix.stat("group_rounds"), ix.stat("group_k"), ix.stat("group_exact"))
                        return out
                    return run

                def old_way():
                    out = []
                    for q in range(nq):
                        s = ix.scores(Qd[q], cos)
                        best = torch.full((n_groups,), -float("inf"), device=dev).scatter_reduce(0, g64, s, "amax", include_self=True)
                        out.append(torch.topk(best, min(k, n_groups))[1])
                    return torch.stack(out).cpu()

                cont = [(grouped("g"), None), (lambda: ix.topk(Qd, k, cos), None), (old_way, a.old_calls), (grouped("x", fast=0), a.exact_calls),
                        (grouped("o2", oversample=2), None), (grouped("o8", oversample=8), None), (grouped("g"), None)]
                pg, pa, pb, px, p2, p8, pg2 = rounds(cont, a.calls, a.warmup)
                spread = abs(pg - pg2) / pg
                verdict = "LOSS" if pg > pa * (1 + spread) else "win" if pa > pg * (1 + spread) else "tie"
                st = lambda t: "/".join(str(v) for v in stats[t])
                lines.append(f"  {name:>5} {size:>5} {k:>4} {nq:>3} {pg:>9.1f} {pg2:>9.1f} {spread:>6.3f} {st('g'):>10} {pa:>9.1f} {pg / pa:>6.2f} {verdict:>5} "
                             f"{pb:>10.1f} {pb / pg:>6.2f} {px:>10.1f} {p2:>9.1f} {st('o2'):>10} {p8:>9.1f} {st('o8'):>10}")
                print(lines[-1], flush=True)
    ix.set_option("group_oversample", 4)
    ix.set_option("group_fast_rounds", 2)


def huge(a, lines, ix, name, Q):
    from hyperdb._native import METRIC_IDS
    cos = METRIC_IDS["cosine_similarity"]
    ix.set_groups(torch.zeros(ix.n, dtype=torch.int32, device=ix.device), 1)
    for nq in a.queries:
        Qd = Q[:nq].contiguous()
        for fast in (2, 0):
            ix.set_option("group_fast_rounds", fast)
            run = lambda: ix.topk_grouped(Qd, 10, cos)
            p, = rounds([(run, a.exact_calls)], a.exact_calls, 1)
            lines.append(f"  {name:>5} one group, top-10, {nq:>3} queries, group_fast_rounds = {fast}: {p:>10.1f} us   rounds/k'/exact = "
                         f"{ix.stat('group_rounds')}/{ix.stat('group_k')}/{ix.stat('group_exact')}")
            print(lines[-1], flush=True)
    ix.set_option("group_fast_rounds", 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows16", type=int, default=10_000_000)
    ap.add_argument("--rows32", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--group-sizes", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--exact-calls", type=int, default=10, help="calls of the exact pass (x) and of the one-group case")
    ap.add_argument("--old-calls", type=int, default=10, help="calls of the scores + scatter_reduce + topk baseline (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_grouped.py measures on the GPU"
    from hyperdb._native import GpuIndex
    dev = torch.device("cuda", 0)
    d = a.dim
    Q = torch.from_numpy(np.random.default_rng(7).standard_normal((max(a.queries), d)).astype(np.float32)).to(dev)
    lines = [f"# tools/time_grouped.py: cosine, p50 of {a.calls} calls in us (device queries in, host results out), {a.warmup} warm-up calls, the contenders",
             f"# alternate call by call; Gaussian rows x {d}; groups = contiguous runs of `size` rows.  {torch.cuda.get_device_name(0)}",
             "# (g), (g') topk_grouped at the defaults, two turns (spread = |g - g'| / g); r/k'/x = fast rounds run / rows per query of the last round / queries",
             "# answered by the exact pass; (a) topk at the same k on the same handle (the floor; verdict: (g) against (a), beyond the spread);",
             f"# (b) hdb_scores per query + torch scatter_reduce(amax) + topk ({a.old_calls} calls); (x) the exact grouped pass alone, group_fast_rounds = 0 ({a.exact_calls} calls);",
             "# (o2), (o8) topk_grouped with group_oversample = 2 / 8",
             f"# {'index':>5} {'size':>5} {'k':>4} {'nq':>3} {'(g) us':>9} {'(g) again':>9} {'spread':>6} {'r/k_/x':>10} {'(a) us':>9} {'g/a':>6} {'':>5} "
             f"{'(b) us':>10} {'b/g':>6} {'(x) us':>10} {'(o2) us':>9} {'r/k_/x':>10} {'(o8) us':>9} {'r/k_/x':>10}"]
    tail = ["# one huge group (every row in one group): no fast round can find a second group, the exact pass answers"]
    for name, rows, dtype in (("fp16", a.rows16, torch.float16), ("fp32", a.rows32, torch.float32)):
        if rows <= 0:
            continue
        V = build(rows, d, dtype, dev)
        ix = GpuIndex(V)
        lines.append(f"# {name}: {rows} rows")
        cells(a, lines, ix, name, Q)
        huge(a, tail, ix, name, Q)
        ix.close()
        del V, ix
        torch.cuda.empty_cache()
    text = "\n".join(lines + tail) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
