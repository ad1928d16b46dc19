"""float8 e4m3 rows wider than 512 elements: call latency of cosine top-100 batches through the opt-in K slices on the bf16 matrix
cores (hdb_mfma_f8_ks.hip, option f8_ks_min_q) against the VALU scan of the same index (f8_ks_min_q = 0: four queries per pass over
the matrix, the default) and against a bfloat16 index over the same values through ITS K slices (twice the bytes, an LDS ring).

One child process per shape, each under a time limit of its own (--limit seconds); the parent never opens the GPU, and the first
shape that fails or runs into its limit ends the run.  In a child: the contenders take turns call by call -- float8 slices, float8
VALU scan, bfloat16 slices, float8 slices AGAIN -- so drift of the clock or of the machine hits all alike; p50 over --calls
synchronous calls (rank_batch: host queries in, host results out) after --warmup calls per contender.  The two p50s of the repeated
contender give the spread a difference has to exceed.  The answers are compared once per shape and query count: float8 slices
against the VALU scan (same rows up to ties inside the float32 contract's band) and against the bfloat16 index (equal bits).

What the table decides: hdb_mfma_f8_ks_min_q(d) in hdb_caps.h (used when f8_ks_min_q = -1) is the smallest measured query count from
which the slices beat the VALU scan by more than the spread, per width.  Where the float8 slices lose to the bfloat16 ones (every 16
queries convert a tile's fragments again) is recorded, not a failure.

    python tools/time_f8_wide.py [--shapes 2000000x768 1500000x1024 1000000x1536 375000x4096] [--queries 5 8 9 12 16 64 128]
                                 [--calls 60] [--warmup 5] [--limit 280] [--out profiles/f8_wide_time.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

HEADER = (f"# {'rows':>10} {'d':>5} {'queries':>7} {'f8 slices':>10} {'f8 VALU':>10} {'bf16 slices':>11} {'f8 again':>10} {'spread':>7} "
          f"{'VALU/f8':>8} {'bf16/f8':>8}  mfma  same as VALU  bits of bf16")


def one_shape(n, d, queries, calls, warmup):
    """-> the table's lines for one shape (a child process runs this)."""
    import numpy as np
    import torch
    import hyperdb.ranking_algorithm as ranking
    from oracle import ranking_oracle as orc
    assert torch.cuda.is_available(), "time_f8_wide.py measures on the GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(n + d)
    chunk = max(1, (1 << 28) // (4 * d))                  # float32 staging of 256 MiB at a time
    V8 = torch.empty((n, d), device=dev, dtype=torch.float8_e4m3fn)
    Vb = torch.empty((n, d), device=dev, dtype=torch.bfloat16)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        x = torch.randn((hi - lo, d), generator=g, device=dev, dtype=torch.float32).to(torch.float8_e4m3fn)      # |x| < 7: no NaN code
        V8[lo:hi] = x
        Vb[lo:hi] = x.float().to(torch.bfloat16)          # a float8 code is a bf16 number: the same values
    h8 = ranking.register_vectors(V8)
    hb = ranking.register_vectors(Vb)
    hb.index.set_option("bf16_ks_min_q", 5)
    rng = np.random.default_rng(7)

    def call(Q, who):
        if who != 2:
            h8.index.set_option("f8_ks_min_q", 0 if who == 1 else 5)
        h = hb if who == 2 else h8
        t0 = time.perf_counter()
        out = ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")        # (returns host arrays: the call has ended)
        return (time.perf_counter() - t0) * 1e6, out

    order = (0, 1, 2, 0)                                  # slices, VALU, bf16, slices again
    lines = []
    for nq in queries:
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        for _ in range(warmup):
            for who in order[:3]:
                call(Q, who)
        _, (mi, ms) = call(Q, 0)
        used = h8.index.stat("mfma")
        _, (vi, vs) = call(Q, 1)
        _, (bi, bs) = call(Q, 2)
        same = all(orc.same_result_modulo_ties(mi[q], ms[q], vi[q], vs[q], 1e-5) for q in range(nq))
        bits = np.array_equal(mi, bi) and np.array_equal(np.asarray(ms).view(np.uint32), np.asarray(bs).view(np.uint32))
        t = [[] for _ in order]
        for _ in range(calls):
            for slot, who in enumerate(order):
                t[slot].append(call(Q, who)[0])
        p = [float(np.median(x)) for x in t]
        spread = abs(p[3] - p[0]) / min(p[0], p[3])
        lines.append(f"  {n:>10} {d:>5} {nq:>7} {p[0]:>10.1f} {p[1]:>10.1f} {p[2]:>11.1f} {p[3]:>10.1f} {100 * spread:>6.1f}% "
                     f"{p[1] / p[0]:>8.2f} {p[2] / p[0]:>8.2f}  {used:>4}  {'yes' if same else 'NO':>12}  {'yes' if bits else 'NO':>12}")
        print(lines[-1], flush=True)
    h8.index.set_option("f8_ks_min_q", 0)
    h8.close()
    hb.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2000000x768", "1500000x1024", "1000000x1536", "375000x4096"])
    ap.add_argument("--queries", type=int, nargs="+", default=[5, 8, 9, 12, 16, 64, 128])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280, help="seconds one shape may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.calls >= 50, "p50 over at least 50 calls"
    if a.child:
        n, d = (int(x) for x in a.child.split("x"))
        for line in one_shape(n, d, a.queries, a.calls, a.warmup):
            print("ROW" + line)
        return 0
    lines = [f"# tools/time_f8_wide.py: cosine top-100, p50 of {a.calls} calls in us (host queries in, host results out), {a.warmup} warm-up calls per contender,",
             "# a float8 e4m3 index through its K slices (f8_ks_min_q = 5), the same index on the VALU scan (f8_ks_min_q = 0, four queries per pass), a bfloat16",
             "# index over the same values through its K slices (bf16_ks_min_q = 5), the float8 slices again; alternating call by call; spread = the two float8-slice p50s apart",
             HEADER]
    failed = None
    for shape in a.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--queries"] + [str(q) for q in a.queries]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            failed = f"{shape}: no answer within {a.limit} s"
            break
        rows = [line[3:] for line in run.stdout.splitlines() if line.startswith("ROW")]
        lines += rows
        print("\n".join(rows), flush=True)
        if run.returncode != 0:
            failed = f"{shape}: exit status {run.returncode}\n{run.stderr[-2000:]}"
            break
    table = [line for line in lines if not line.startswith("#")]
    if failed:
        lines.append("# the run ended early: " + failed.splitlines()[0])
    elif any(" NO" in line for line in table):
        lines.append("# verdict: MISSED -- the float8 slices disagree with the VALU scan or with the bfloat16 index's bits in a row of the table")
    else:
        lines.append("# verdict: the float8 slices agree with the VALU scan and return the bfloat16 index's bits in every row of the table")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if failed:
        print(failed, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
