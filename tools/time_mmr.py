"""Diverse top-k (hdb_mmr_host): call latency on one MI355X, cosine relevance and cosine pair similarity, lambda 0.5.

Gaussian rows are generated on the device from a seed.  Contenders, alternating call by call, p50 over --calls synchronous calls
(host queries in, host results out) after --warmup calls:
  (m), (m')  GpuIndex.mmr(Q, fetch_k, top_k) at the defaults, two turns per round -- the difference of their medians is the spread
             every other column is read against;
  (a)        GpuIndex.topk at fetch_k on the same handle: the floor, the call's own first half;
  (b)        the only way before: topk_device + a torch gather of the rows + a torch matmul for the Gram matrix + the Python greedy
             loop of top_k steps (--loop-calls calls).
Written down BEFORE measuring, from the kernel guide's constants (`pred` = (a) + the sum, in microseconds):
  pairs      mc^2 d / 2 fma at the float32 vector rate (157.3 TFLOPS = 78.6e12 fma/s) plus the gather of mc rows at the gather rate
             (5.5 TB/s), per query, mc = fetch_k;
  selection  top_k x (one dependent global load + two workgroup reductions): the load sits between the L2-hit (~200 cycles) and the
             HBM-miss latency (~900 cycles); taken as 550 + 2 x 100 cycles at 2.4 GHz per step.  Queries select side by side (one
             workgroup each) while they fit one chunk; chunks serialise;
  launches   three per chunk (prep, pairs, select) behind the status read-back of the first half: 4 x 5 us per chunk for the
             launches and one synchronisation.
`m/pred` says how far the call lands from it.  No time is a pass condition; a verdict counts only beyond the spread, losses are
printed as LOSS.  --trace runs the three new launches alone, a few calls of one shape, for a kernel trace taken in a run of its own.

    python tools/time_mmr.py [--calls 60] [--warmup 3] --out profiles/mmr_time.txt
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

FMA_RATE = 78.6e12
GATHER_RATE = 5.5e12
CLOCK = 2.4e9
STEP_CYCLES = 550 + 2 * 100
LAUNCH_US = 5.0
CHUNK = 1_000_000
CELLS = ((10, 40), (100, 400), (100, 2048))
BATCHES = (1, 16, 256)


def rows_on_device(n, d, dtype, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    V = torch.empty((n, d), dtype=dtype, device=dev)
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        V[r0:r0 + m] = torch.randn((m, d), generator=g, device=dev, dtype=torch.float32).to(dtype)
    return V


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


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
            t[i].append(timed(fn))
    return [float(np.median(x)) for x in t]


def predicted_us(ix, nq, k, m, chunks):
    row_bytes = ix.V.element_size() * ix.V.shape[1]
    pairs = nq * (m * m * ix.d / 2 / FMA_RATE + m * row_bytes / GATHER_RATE)
    select = chunks * k * STEP_CYCLES / CLOCK
    return (pairs + select) * 1e6 + chunks * 4 * LAUNCH_US


def before(ix, Q, m, k, cos):
    """topk_device + gather + Gram matrix + the greedy loop in torch: three launches and more per step."""
    li, ls, _ = ix.topk_device(Q, m, cos)
    out = []
    for q in range(li.shape[0]):
        X = ix.V[li[q]].to(torch.float32)
        X = X / X.norm(dim=1, keepdim=True)
        P = X @ X.T
        r = ls[q]
        pen = torch.full_like(r, -float("inf"))
        taken = torch.zeros_like(r, dtype=torch.bool)
        picks = []
        for t in range(k):
            val = r if t == 0 else 0.5 * r - 0.5 * pen
            s = torch.argmax(torch.where(taken, torch.full_like(val, -float("inf")), val))
            taken[s] = True
            pen = torch.maximum(pen, P[s])
            picks.append(s)
        out.append(li[q][torch.stack(picks)].cpu())
    return out


def cell(a, lines, ix, name, nq, k, m):
    from hyperdb._native import METRIC_IDS
    cos = METRIC_IDS["cosine_similarity"]
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((nq, ix.d)).astype(np.float32)
    call = lambda: ix.mmr(Q, m, k, cos, 0.5)
    floor = lambda: ix.topk(Q, m, cos)
    call()
    chunks = ix.stat("mmr_chunks")
    cont = [(call, None), (floor, None), (lambda: before(ix, Q, m, k, cos), a.loop_calls), (call, None)]
    pm, pa, pb, pm2 = rounds(cont, a.calls, a.warmup)
    spread = abs(pm - pm2) / pm
    mark = lambda other: "win" if other > pm * (1 + spread) else "LOSS" if pm > other * (1 + spread) else "tie"
    pred = pa + predicted_us(ix, nq, k, m, chunks)
    lines.append(f"  {name:<22} {nq:>4} {k:>5} {m:>7} {chunks:>6} {pm:>10.1f} {pm2:>10.1f} {spread:>7.3f} {pa:>10.1f} {pm / pa:>6.2f} {mark(pa):>4} "
                 f"{pm - pa:>10.1f} {pred - pa:>10.1f} {pm / pred:>7.2f} {pb:>12.1f} {pb / pm:>7.2f} {mark(pb):>4}")
    print(lines[-1], flush=True)


def trace(a):
    """The three new launches alone on one shape, for rocprofv3 --kernel-trace --stats in a run of its own."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    dev = torch.device("cuda", 0)
    cos = METRIC_IDS["cosine_similarity"]
    ix = GpuIndex(rows_on_device(a.rows, 384, torch.float16, dev))
    Q = np.random.default_rng(7).standard_normal((16, 384)).astype(np.float32)
    for k, m in CELLS:
        li, ls, _ = ix.topk_device(Q, m, cos)
        for _ in range(5):
            ix.mmr_device(li, ls, k, 0.5, cos)
    torch.cuda.synchronize()
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-calls", type=int, default=3, help="calls of the torch loop (b)")
    ap.add_argument("--big-rows", type=int, default=10_000_000)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--trace", action="store_true", help="run only the three new launches, for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_mmr.py measures on the GPU"
    if a.trace:
        return trace(a)
    assert a.calls >= 50, "p50 over at least 50 calls"
    from hyperdb._native import GpuIndex
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_mmr.py: cosine relevance, cosine pairs, lambda 0.5, p50 of {a.calls} calls in us (host queries in, host results out), {a.warmup} warm-up calls,",
             f"# the contenders alternate call by call; Gaussian rows.  {torch.cuda.get_device_name(0)}",
             "# (m), (m') GpuIndex.mmr at the defaults, two turns (spread = |m - m'| / m); chunks: the stat mmr_chunks",
             "# (a) topk at fetch_k on the same handle (the floor, the call's own first half; verdict: (m) against (a), beyond the spread)",
             f"# (b) topk_device + torch gather + torch Gram matrix + the Python greedy loop ({a.loop_calls} calls; verdict: (m) against it)",
             f"# expected m - a, written down before measuring: per query fetch_k^2 d / 2 fma at {FMA_RATE / 1e12:.1f}e12 fma/s + fetch_k rows at {GATHER_RATE / 1e12:.1f} TB/s;",
             f"#   per chunk top_k x {STEP_CYCLES} cycles at {CLOCK / 1e9:.1f} GHz (one dependent load between L2 hit and HBM miss + two workgroup reductions) + 4 x {LAUNCH_US:.0f} us",
             f"# {'index':<22} {'nq':>4} {'top_k':>5} {'fetch_k':>7} {'chunks':>6} {'(m) us':>10} {'(m) again':>10} {'spread':>7} {'(a) us':>10} {'m/a':>6} {'':>4} "
             f"{'m - a':>10} {'expected':>10} {'m/pred':>7} {'(b) us':>12} {'b/m':>7} {'':>4}"]
    for n, dtype, name in ((a.big_rows, torch.float16, "fp16"), (a.rows, torch.float32, "fp32")):
        ix = GpuIndex(rows_on_device(n, 384, dtype, dev))
        for k, m in CELLS:
            for nq in BATCHES:
                cell(a, lines, ix, f"{n} x 384 {name}", nq, k, m)
        ix.close()
        del ix
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
