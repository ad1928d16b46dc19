"""Range search (hdb_range_host + hdb_range_fetch): call latency on one MI355X, cosine.

Gaussian rows are generated on the device from a seed.  Contenders, alternating call by call, p50 over --calls synchronous calls (host
queries in, host results out) after --warmup calls:
  (r), (r')  GpuIndex.range(Q, thr) at the defaults, sorted, two turns per round -- the difference of their medians is the spread
             every other column is read against;
  (a)        topk_exact of the same queries at k = 100 on the same handle: the floor -- the same score pass, a fixed-size selection;
  (b)        the only way before: hdb_scores per query + torch.nonzero + torch.sort (--loop-calls calls).
Thresholds pass about 0, 100, 10 000 and 1 % of the rows per query (cosine of Gaussian rows is N(0, 1 / d): the normal quantile).
Written down BEFORE measuring, from the bytes at the README's 6.0 TB/s (`pred`, in microseconds):
  the matrix once per chunk of queries (the stat range_chunks);
  sbuf written once and read twice, 3 x nq x n x 4 B (score pass, count, emit);
  8 B per result written and read (the packed keys: emit, then sort / unpack).
Launch gaps, the one synchronisation per chunk and the copy of the result to the host are NOT in it: `r/pred` says how far the call
lands from the bytes alone.  No time is a pass condition; a verdict counts only beyond the spread, losses are printed as LOSS.
Every step -- one index and one batch size, in a process of its own -- has a time limit (--step-seconds); the first step that fails
or runs out of time ends the run, and what was measured until then is written.

    python tools/time_range.py [--calls 60] [--warmup 3] --out profiles/range_time.txt
"""
import argparse
import os
import subprocess
import sys
import time
from statistics import NormalDist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

HBM_RATE = 6.0e12
D = 384
CHUNK = 1_000_000
BATCHES = (1, 16, 256)
PASSING = ("0", "100", "10000", "1%")


def predicted_us(matrix_bytes, n, nq, chunks, total):
    return (chunks * matrix_bytes + 3 * nq * n * 4 + 2 * 8 * total) / HBM_RATE * 1e6


def threshold(n, passing):
    if passing == "0":
        return 0.9
    share = 0.01 if passing == "1%" else int(passing) / n
    return NormalDist().inv_cdf(1.0 - share) / D ** 0.5


def step(a):
    """One index, one batch size: the four thresholds -> one line each on standard output."""
    import numpy as np
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    dev = torch.device("cuda", 0)
    dtype = torch.float16 if a.dtype == "fp16" else torch.float32
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    V = torch.empty((a.n, D), dtype=dtype, device=dev)
    for r0 in range(0, a.n, CHUNK):
        m = min(CHUNK, a.n - r0)
        V[r0:r0 + m] = torch.randn((m, D), generator=g, device=dev, dtype=torch.float32).to(dtype)
    ix = GpuIndex(V)
    cos = METRIC_IDS["cosine_similarity"]
    Q = np.random.default_rng(7).standard_normal((a.nq, D)).astype(np.float32)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    def before(thr):
        out = []
        for q in range(a.nq):
            s = ix.scores(Q[q], cos)
            rows = torch.nonzero(s >= thr).reshape(-1)
            val, order = torch.sort(s[rows], descending=True, stable=True)
            out.append((rows[order].cpu(), val.cpu()))
        return out

    for passing in PASSING:
        thr = threshold(a.n, passing)
        call = lambda: ix.range(Q, thr, cos)
        lims = call()[0]
        chunks, total = ix.stat("range_chunks"), int(lims[-1])
        cont = [(call, None), (lambda: ix.topk_device(Q, 100, cos, exact=True)[0].cpu(), None), (lambda: before(thr), a.loop_calls), (call, None)]
        for fn, own in cont:
            for _ in range(a.warmup if own is None else 1):
                fn()
        t = [[] for _ in cont]
        for c in range(a.calls):
            for i, (fn, own) in enumerate(cont):
                if own is None or c < own:
                    t[i].append(timed(fn))
        pr, pa, pb, pr2 = (float(np.median(x)) for x in t)
        spread = abs(pr - pr2) / pr
        mark = lambda other: "win" if other > pr * (1 + spread) else "LOSS" if pr > other * (1 + spread) else "tie"
        pred = predicted_us(V.element_size() * V.numel(), a.n, a.nq, chunks, total)
        print(f"  {str(a.n) + ' x 384 ' + a.dtype:<22} {a.nq:>4} {passing:>6} {total:>10} {chunks:>6} {pr:>10.1f} {pr2:>10.1f} {spread:>7.3f} {pred:>10.1f} "
              f"{pr / pred:>7.2f} {pa:>10.1f} {pr / pa:>6.2f} {mark(pa):>4} {pb:>12.1f} {pb / pr:>7.2f} {mark(pb):>4}", flush=True)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-calls", type=int, default=3, help="calls of the per-query loop (b)")
    ap.add_argument("--big-rows", type=int, default=10_000_000)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of one step (one index, one batch size)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", nargs=3, metavar=("N", "DTYPE", "NQ"), help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        a.n, a.dtype, a.nq = int(a.step[0]), a.step[1], int(a.step[2])
        return step(a)
    assert a.calls >= 50, "p50 over at least 50 calls"
    lines = [f"# tools/time_range.py: cosine, sorted, p50 of {a.calls} calls in us (host queries in, host results out), {a.warmup} warm-up calls,",
             "# the contenders alternate call by call; Gaussian rows; one MI355X",
             "# (r), (r') GpuIndex.range at the defaults, two turns (spread = |r - r'| / r); passing: rows per query the threshold aims at; total: entries returned",
             "# pred, written down before measuring: (chunks x matrix + 3 x nq x n x 4 B + 16 B per result) / 6.0 TB/s -- bytes alone, no launch, no synchronisation, no copy out",
             "# (a) topk_exact of the same queries at k = 100 (the floor: same score pass, fixed-size selection; verdict: (r) against (a), beyond the spread)",
             f"# (b) hdb_scores per query + torch.nonzero + torch.sort ({a.loop_calls} calls; verdict: (r) against it)",
             f"# {'index':<22} {'nq':>4} {'pass':>6} {'total':>10} {'chunks':>6} {'(r) us':>10} {'(r) again':>10} {'spread':>7} {'pred':>10} {'r/pred':>7} "
             f"{'(a) us':>10} {'r/a':>6} {'':>4} {'(b) us':>12} {'b/r':>7} {'':>4}"]
    failed = None
    for n, dtype in ((a.big_rows, "fp16"), (a.rows, "fp32")):
        for nq in BATCHES:
            cmd = [sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--warmup", str(a.warmup), "--loop-calls", str(a.loop_calls),
                   "--step", str(n), dtype, str(nq)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_seconds)
                out, rc = done.stdout, done.returncode
                err = done.stderr
            except subprocess.TimeoutExpired as e:
                out, rc, err = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), 124, f"time limit of {a.step_seconds} s"
            lines += [ln for ln in out.splitlines() if ln.startswith("  ")]
            print(out, end="", flush=True)
            if rc != 0:
                failed = f"# STOPPED: step {n} x 384 {dtype}, {nq} queries ended with status {rc}: {err.strip().splitlines()[-1] if err.strip() else ''}"
                break
        if failed:
            break
    if failed:
        lines.append(failed)
        print(failed, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main() or 0)
