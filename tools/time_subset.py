"""Row-list scan (hdb_index_set_row_subset): what a selective filter costs through the list against the masked call.

Every cell times the SAME handle twice -- use_subset = 0 (the masked path of every build before the list existed) and use_subset = 1
with subset_min_n = 0, subset_ratio = 1 (the list wherever a call can take it) -- cosine top-100, host queries in, host results out
(hdb_topk_host: synchronised).  The two alternate call by call after --warmup calls of each; p50 over --calls calls each, in us.
A cell whose list call cannot be taken even at ratio 1 (m * ceil(nq / 4) > n) is printed as "not eligible".  Each cell also checks
that the two answers agree modulo ties at the dtype's tolerance (oracle.same_result_modulo_ties) at the timed size.

Indexes: 10M x 384 fp16 with defaults (the automatic int8 shadow included), 2M x 384 float32, 1M x 768 bfloat16; kept shares 1/2 ..
1/1024 (m = n / share exactly) with random ascending rows; 1, 4 and 16 queries.  Ladder: 50k .. 1M rows of 384 fp16 at share 1/64, one query.

The last lines derive the two rules of hdb_plan.h from the table: subset_ratio = the smallest power of two R such that every measured
cell with m * ceil(nq / 4) * R <= n is at least 1.10x faster through the list; subset_min_n = the smallest ladder size from which the
list wins by 1.10x at that size and every larger one, never below 32 768.

    python tools/time_subset.py [--calls 200] [--warmup 10] [--out profiles/subset_time.txt]
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

from hyperdb._native import GpuIndex, METRIC_IDS
from oracle import ranking_oracle as orc

COS = METRIC_IDS["cosine_similarity"]
MARGIN = 1.10
FLOOR = 32768
_TORCH = {"fp16": torch.float16, "fp32": torch.float32, "bf16": torch.bfloat16}
_TOL = {"fp16": 1e-3, "fp32": 1e-5, "bf16": 1e-5}


def timed(ix, Q, use):
    ix.set_option("use_subset", use)
    t0 = time.perf_counter()
    out = ix.topk(Q, 100, COS)
    return (time.perf_counter() - t0) * 1e6, out


def cell(ix, dt, n, share, nq, calls, warmup, rng, dev):
    """-> (m, p50 masked, p50 list or None, the two answers agree)"""
    g = torch.Generator(device=dev); g.manual_seed(int(n // share) + nq)
    m = n // share                                                   # exactly the share: the rule's inequality is read at m itself
    rows = torch.sort(torch.randperm(n, generator=g, device=dev)[:m]).values.contiguous()
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    mask[rows] = 1
    Q = rng.standard_normal((nq, ix.d)).astype(np.float32)
    ix.set_row_subset(mask, rows)
    try:
        for _ in range(warmup):
            timed(ix, Q, 0); timed(ix, Q, 1)
        _, a = timed(ix, Q, 0)
        assert ix.stat("subset") == 0
        _, b = timed(ix, Q, 1)
        taken = ix.stat("subset") == 1
        assert taken == (m * ((nq + 3) // 4) <= n), (m, nq, n, taken)
        same = all(orc.same_result_modulo_ties(a[0][q], a[1][q], b[0][q], b[1][q], _TOL[dt]) for q in range(nq))
        if not taken:
            t0 = [timed(ix, Q, 0)[0] for _ in range(calls)]
            return m, float(np.median(t0)), None, same
        t = [[], []]
        for _ in range(calls):
            t[0].append(timed(ix, Q, 0)[0])
            t[1].append(timed(ix, Q, 1)[0])
        return m, float(np.median(t[0])), float(np.median(t[1])), same
    finally:
        ix.set_row_mask(None)


def build(dt, n, d, dev):
    g = torch.Generator(device=dev); g.manual_seed(n + d)
    V = torch.empty((n, d), dtype=_TORCH[dt], device=dev)
    step = 1_000_000
    for lo in range(0, n, step):                                   # (in pieces: no float32 copy of the whole matrix)
        hi = min(n, lo + step)
        V[lo:hi] = torch.randn((hi - lo, d), generator=g, device=dev, dtype=torch.float32).to(_TORCH[dt])
    ix = GpuIndex(V, device=dev)
    ix.set_option("subset_min_n", 0)
    ix.set_option("subset_ratio", 1)
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="row counts times this (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_subset.py measures on the GPU"
    assert a.calls >= 200, "p50 over at least 200 calls of each path"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    lines = [f"# tools/time_subset.py: cosine top-100, p50 of {a.calls} calls in us (host queries in, host results out), {a.warmup} warm-up calls "
             "of each path, masked (use_subset = 0) and list (use_subset = 1, subset_min_n = 0, subset_ratio = 1) alternate call by call on one handle",
             f"# {torch.cuda.get_device_name(0)}",
             f"# {'index':>16} {'share':>6} {'m':>9} {'queries':>7} {'masked':>9} {'list':>9} {'masked/list':>11}  m*ceil(nq/4)/n  agree"]
    cells = []            # (n, m, nq, speedup)
    bad = []
    for dt, n, d in (("fp16", 10_000_000, 384), ("fp32", 2_000_000, 384), ("bf16", 1_000_000, 768)):
        n = int(n * a.scale)
        ix = build(dt, n, d, dev)
        try:
            for share in (2, 4, 8, 16, 64, 1024):
                for nq in (1, 4, 16):
                    m, p0, p1, same = cell(ix, dt, n, share, nq, a.calls, a.warmup, rng, dev)
                    if not same:
                        bad.append((dt, n, share, nq))
                    load = m * ((nq + 3) // 4) / n
                    if p1 is None:
                        lines.append(f"  {n:>9}x{d} {dt} {'1/' + str(share):>6} {m:>9} {nq:>7} {p0:>9.1f} {'-':>9} {'not eligible':>11}  {load:>14.3f}  {same}")
                    else:
                        cells.append((n, m, nq, p0 / p1))
                        lines.append(f"  {n:>9}x{d} {dt} {'1/' + str(share):>6} {m:>9} {nq:>7} {p0:>9.1f} {p1:>9.1f} {p0 / p1:>11.2f}  {load:>14.3f}  {same}")
                    print(lines[-1], flush=True)
        finally:
            ix.close()
        del ix
        torch.cuda.empty_cache()
    lines.append("# ladder: rows x 384 fp16, share 1/64, one query")
    ladder = []
    for n in (50_000, 100_000, 250_000, 500_000, 1_000_000):
        n = max(int(n * a.scale), 20_000)
        ix = build("fp16", n, 384, dev)
        try:
            m, p0, p1, same = cell(ix, "fp16", n, 64, 1, a.calls, a.warmup, rng, dev)
        finally:
            ix.close()
        if not same:
            bad.append(("fp16 ladder", n, 64, 1))
        ladder.append((n, p0 / p1))
        lines.append(f"  {n:>9}x384 fp16 {'1/64':>6} {m:>9} {1:>7} {p0:>9.1f} {p1:>9.1f} {p0 / p1:>11.2f}  {m / n:>14.3f}  {same}")
        print(lines[-1], flush=True)
    # ---- the two rules ----
    ratio = None
    for e in range(0, 21):
        R = 1 << e
        sel = [c for c in cells if c[1] * ((c[2] + 3) // 4) * R <= c[0]]
        if all(c[3] >= MARGIN for c in sel):
            ratio = R
            lines.append(f"# subset_ratio rule: R = {R} is the smallest power of two with every measured cell m * ceil(nq / 4) * R <= n at least "
                         f"{MARGIN:.2f}x faster through the list ({len(sel)} cells, slowest {min((c[3] for c in sel), default=float('nan')):.2f}x)")
            break
    if ratio is None:
        lines.append("# subset_ratio rule: no power of two up to 2^20 admits only winning cells")
    min_n = None
    for i, (n, _) in enumerate(ladder):
        if all(s >= MARGIN for _, s in ladder[i:]):
            min_n = max(n, FLOOR)
            break
    lines.append(f"# subset_min_n rule: {min_n if min_n is not None else 'no ladder size wins by 1.10x at that size and every larger one'}"
                 f" (smallest ladder size from which the list wins by {MARGIN:.2f}x at that size and every larger one; never below {FLOOR})")
    lines.append("# answers: " + ("masked and list agree modulo ties in every cell" if not bad else f"DISAGREE at {bad}"))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
