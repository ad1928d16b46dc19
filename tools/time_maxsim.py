"""Multi-vector queries (hdb_maxsim_host): call latency on one MI355X, top-10 groups.

Gaussian rows are generated on the device from a seed; a call carries S sets of T Gaussian vectors.  Contenders, alternating call by
call, p50 over --calls synchronous calls (host vectors in, host results out) after --warmup calls:
  (m), (m')  GpuIndex.maxsim at the defaults, two turns per round -- the difference of their medians is the spread every other column
             is read against;
  (a)        topk_exact of the same flat vectors at the same k on the same handle: the floor -- the same score pass, one selection per
             VECTOR over n rows instead of one per SET over the groups, and no reduction;
  (b)        the only way before: hdb_scores per vector + torch scatter_reduce(amax) + sum + topk (--loop-calls calls);
  (t1) .. (t64)  maxsim with maxsim_team fixed to 1 / 4 / 16 / 64 against the rule's choice in (m) (--slow-calls calls where a team
             walks a huge group alone); the rule's own team is marked "same": the same configuration plus two option calls.
Written down BEFORE measuring, from the bytes alone: a call moves the matrix once per chunk (chunks x n x row bytes), stores and
re-loads every score (2 x vectors x n x 4 B) and runs one selection per set over the groups (about 5 passes over n_groups x 4 B),
all at the plain-store / streaming-load rate of 6.0 TB/s (kernel guide: 6.0-6.3 TB/s); `pred` is that many microseconds, `m/pred`
how far the call lands from it (launch gaps, the host round trip and a score pass that is compute- rather than memory-bound are
what the bytes leave out).  No time is a pass condition; a verdict counts only beyond the spread, losses are printed as LOSS.

    python tools/time_maxsim.py [--calls 60] [--warmup 3] --out profiles/maxsim_time.txt
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

K = 10
RATE = 6.0e12
CHUNK = 1_000_000


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


def shape(a, lines, ix, name, groups, n_groups, T, S, slow_teams=False):
    from hyperdb._native import METRIC_IDS, pack_query_sets
    cos = METRIC_IDS["cosine_similarity"]
    n, d = ix.n, ix.d
    rng = np.random.default_rng(7)
    flat, off = pack_query_sets(rng.standard_normal((S, T, d)).astype(np.float32), d)
    ix.set_groups(groups, n_groups)
    gdev = ix._groups.to(torch.int64)
    k = min(K, n_groups)

    def call():
        return ix.maxsim(flat, off, k, cos)

    def floor():
        i, s, _ = ix.topk_device(flat, k, cos, exact=True)
        return i.cpu(), s.cpu()

    def before():
        out = []
        for s in range(S):
            total = torch.zeros(n_groups, device=gdev.device)
            for v in range(off[s], off[s + 1]):
                sc = ix.scores(flat[v], cos)
                total += torch.full((n_groups,), -float("inf"), device=gdev.device).scatter_reduce(0, gdev, sc, "amax")
            out.append(torch.topk(total, k))
        return [(o.indices.cpu(), o.values.cpu()) for o in out]

    def team(t):
        def fn():
            ix.set_option("maxsim_team", t)
            try:
                return ix.maxsim(flat, off, k, cos)
            finally:
                ix.set_option("maxsim_team", 0)
        return fn

    call()
    chunks, rule, sorted_ = ix.stat("maxsim_chunks"), ix.stat("maxsim_team"), ix.stat("maxsim_sorted")
    row_bytes = ix.V.element_size() * ix.V.shape[1]
    pred = (chunks * n * row_bytes + 2 * S * T * n * 4 + S * 5 * n_groups * 4) / RATE * 1e6
    own = a.slow_calls if slow_teams else None
    cont = [(call, None), (floor, None), (before, a.loop_calls)] + [(team(t), own) for t in (1, 4, 16, 64)] + [(call, None)]
    p = rounds(cont, a.calls, a.warmup)
    pm, pa, pb, pt, pm2 = p[0], p[1], p[2], p[3:7], p[7]
    spread = abs(pm - pm2) / pm
    mark = lambda other: "win" if other > pm * (1 + spread) else "LOSS" if pm > other * (1 + spread) else "tie"
    # (the rule's own team is the call itself plus two option calls: no verdict against an identical configuration)
    teams = " ".join(f"{x:>10.1f} {'same' if t == rule else mark(x):>4}" for t, x in zip((1, 4, 16, 64), pt))
    lines.append(f"  {name:<28} {S:>3} {T:>3} {chunks:>6} {rule:>4} {sorted_:>6} {pm:>10.1f} {pm2:>10.1f} {spread:>7.3f} {pred:>9.1f} {pm / pred:>7.2f} "
                 f"{pa:>10.1f} {pm / pa:>6.2f} {mark(pa):>4} {pb:>12.1f} {pb / pm:>7.2f} {teams}")
    print(lines[-1], flush=True)
    ix.set_groups(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-calls", type=int, default=3, help="calls of the per-vector loop (b)")
    ap.add_argument("--slow-calls", type=int, default=3, help="calls of a fixed team on the one-group shape")
    ap.add_argument("--big-rows", type=int, default=10_000_000)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--one-rows", type=int, default=200_000, help="rows of the one-group shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_maxsim.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    from hyperdb._native import GpuIndex
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_maxsim.py: cosine, top-{K} groups, p50 of {a.calls} calls in us (host vectors in, host results out), {a.warmup} warm-up calls, the contenders",
             f"# alternate call by call; Gaussian rows.  {torch.cuda.get_device_name(0)}",
             "# (m), (m') maxsim at the defaults, two turns (spread = |m - m'| / m); chunks / team / sorted: the stats maxsim_chunks, maxsim_team (the rule's choice), maxsim_sorted",
             f"# pred: what the bytes predict at {RATE / 1e12:.1f} TB/s, written down before measuring: chunks x n x row bytes + 2 x vectors x n x 4 B + sets x 5 x n_groups x 4 B",
             "# (a) topk_exact of the same flat vectors at the same k (the floor: same score pass, one selection per vector; verdict: (m) against (a), beyond the spread)",
             f"# (b) hdb_scores per vector + scatter_reduce(amax) + sum + topk ({a.loop_calls} calls); (t1) .. (t64) maxsim_team fixed, verdict: (m) against it"
             f" (one-group shape: {a.slow_calls} calls each)",
             f"# {'shape':<28} {'S':>3} {'T':>3} {'chunks':>6} {'team':>4} {'sorted':>6} {'(m) us':>10} {'(m) again':>10} {'spread':>7} {'pred us':>9} {'m/pred':>7} "
             f"{'(a) us':>10} {'m/a':>6} {'':>4} {'(b) us':>12} {'b/m':>7} {'(t1) us':>10} {'':>4} {'(t4) us':>10} {'':>4} {'(t16) us':>10} {'':>4} {'(t64) us':>10} {'':>4}"]
    # 10M x 128 fp16, contiguous groups of 100 rows, T = 32, 1 and 8 sets
    n = a.big_rows
    ix = GpuIndex(rows_on_device(n, 128, torch.float16, dev))
    g100 = torch.arange(n, device=dev, dtype=torch.int32) // 100
    for S in (1, 8):
        shape(a, lines, ix, f"{n} x 128 fp16, groups of 100", g100, (n + 99) // 100, 32, S)
    ix.close()
    del ix, g100
    # 2M x 384 float32, groups of 4, T = 4
    n = a.rows
    ix = GpuIndex(rows_on_device(n, 384, torch.float32, dev))
    shape(a, lines, ix, f"{n} x 384 fp32, groups of 4", torch.arange(n, device=dev, dtype=torch.int32) // 4, (n + 3) // 4, 4, 1)
    ix.close()
    del ix
    # 2M x 384 fp16: every row its own group, T = 8; shuffled ids (groups of 4); one group holding all rows (fewer rows: a team walks it alone)
    ix = GpuIndex(rows_on_device(n, 384, torch.float16, dev))
    shape(a, lines, ix, f"{n} x 384 fp16, each row a group", torch.arange(n, device=dev, dtype=torch.int32), n, 8, 1)
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    shape(a, lines, ix, f"{n} x 384 fp16, groups of 4 shuffled", (perm // 4).to(torch.int32), (n + 3) // 4, 4, 1)
    ix.close()
    del ix
    n1 = a.one_rows
    ix = GpuIndex(rows_on_device(n1, 384, torch.float16, dev))
    shape(a, lines, ix, f"{n1} x 384 fp16, ONE group", torch.zeros(n1, device=dev, dtype=torch.int32), 1, 4, 1, slow_teams=True)
    ix.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
