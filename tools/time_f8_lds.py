"""float8 e4m3 batches on the bf16 matrix cores: call latency of cosine top-100 through the LDS flavour (hdb_mfma_f8_lds.h, option
f8_lds_min_q = 5: a stage of rows expanded to bf16 once per workgroup) against the register flavour of the same index (f8_lds_min_q =
0: every wave converts its own fragments -- the behaviour before the option existed) and against a bfloat16 index over the same
values (twice the bytes, an LDS ring).  Whole rows of 128 .. 512 elements and, with f8_ks_min_q = 5, the K slices of wider rows.

One child process per shape, each under a time limit of its own (--limit seconds); the parent never opens the GPU, and the first
shape that fails or runs into its limit ends the run.  In a child: the contenders take turns call by call -- LDS flavour, register
flavour, bfloat16, LDS flavour AGAIN -- so drift of the clock or of the machine hits all alike; p50 over --calls synchronous calls
(rank_batch: host queries in, host results out) after --warmup calls per contender.  The two p50s of the repeated contender give the
spread a difference has to exceed.  The answers are compared once per shape and query count: the LDS flavour returns the register
flavour's and the bfloat16 index's indices and score bits.  --waves 4 | 8 sets f8_lds_waves (the A/B run behind HDB_F8_LDS_WAVES).

What the table decides: hdb_mfma_f8_lds_min_q(d) in hdb_caps.h (used when f8_lds_min_q = -1) is the smallest measured batch size from
which the LDS flavour beats the register flavour by more than the spread at every larger measured size, 0 where there is none.  The
ratio to bfloat16 is recorded, not gated.

    python tools/time_f8_lds.py [--shapes 10000000x384 2000000x128 2000000x256 2000000x512 2000000x768 375000x4096]
                                [--queries 16 32 64 128 256] [--waves 4] [--calls 60] [--warmup 5] [--limit 280] [--out profiles/f8_lds_time.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

HEADER = (f"# {'rows':>10} {'d':>5} {'queries':>7} {'f8 LDS':>10} {'f8 regs':>10} {'bf16':>11} {'LDS again':>10} {'spread':>7} "
          f"{'regs/LDS':>8} {'bf16/LDS':>8}  f8_lds  bits of regs  bits of bf16")


def one_shape(n, d, queries, calls, warmup, waves):
    """-> the table's lines for one shape (a child process runs this)."""
    import numpy as np
    import torch
    import hyperdb.ranking_algorithm as ranking
    assert torch.cuda.is_available(), "time_f8_lds.py measures on the GPU"
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
    h8.index.set_option("f8_ks_min_q", 5)                 # rows wider than 512 elements: both float8 contenders through the K slices
    h8.index.set_option("f8_lds_waves", waves)
    rng = np.random.default_rng(7)

    def call(Q, who):
        if who != 2:
            h8.index.set_option("f8_lds_min_q", 0 if who == 1 else 5)
        h = hb if who == 2 else h8
        t0 = time.perf_counter()
        out = ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")        # (returns host arrays: the call has ended)
        return (time.perf_counter() - t0) * 1e6, out

    order = (0, 1, 2, 0)                                  # LDS, registers, bf16, LDS again
    lines = []
    for nq in queries:
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        for _ in range(warmup):
            for who in order[:3]:
                call(Q, who)
        _, (mi, ms) = call(Q, 0)
        used = h8.index.stat("f8_lds")
        _, (vi, vs) = call(Q, 1)
        _, (bi, bs) = call(Q, 2)
        same = np.array_equal(mi, vi) and np.array_equal(np.asarray(ms).view(np.uint32), np.asarray(vs).view(np.uint32))
        bits = np.array_equal(mi, bi) and np.array_equal(np.asarray(ms).view(np.uint32), np.asarray(bs).view(np.uint32))
        t = [[] for _ in order]
        for _ in range(calls):
            for slot, who in enumerate(order):
                t[slot].append(call(Q, who)[0])
        p = [float(np.median(x)) for x in t]
        spread = abs(p[3] - p[0]) / min(p[0], p[3])
        lines.append(f"  {n:>10} {d:>5} {nq:>7} {p[0]:>10.1f} {p[1]:>10.1f} {p[2]:>11.1f} {p[3]:>10.1f} {100 * spread:>6.1f}% "
                     f"{p[1] / p[0]:>8.2f} {p[2] / p[0]:>8.2f}  {used:>6}  {'yes' if same else 'NO':>12}  {'yes' if bits else 'NO':>12}")
        print(lines[-1], flush=True)
    h8.close()
    hb.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["10000000x384", "2000000x128", "2000000x256", "2000000x512", "2000000x768", "375000x4096"])
    ap.add_argument("--queries", type=int, nargs="+", default=[16, 32, 64, 128, 256])
    ap.add_argument("--waves", type=int, default=4, choices=(0, 4, 8), help="waves per workgroup of the LDS flavour (f8_lds_waves; 0 = by the launch's queries)")
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=280, help="seconds one shape may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.calls >= 50, "p50 over at least 50 calls"
    if a.child:
        n, d = (int(x) for x in a.child.split("x"))
        for line in one_shape(n, d, a.queries, a.calls, a.warmup, a.waves):
            print("ROW" + line)
        return 0
    lines = [f"# tools/time_f8_lds.py: cosine top-100, p50 of {a.calls} calls in us (host queries in, host results out), {a.warmup} warm-up calls per contender,",
             f"# a float8 e4m3 index with f8_lds_min_q = 5 (rows expanded in LDS, {a.waves} waves per workgroup), the same index with f8_lds_min_q = 0 (converted per fragment in",
             "# registers), a bfloat16 index over the same values, the LDS flavour again; rows wider than 512 elements through the K slices (f8_ks_min_q = 5,",
             "# bf16_ks_min_q = 5); alternating call by call; spread = the two LDS p50s apart",
             HEADER]
    failed = None
    for shape in a.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--waves", str(a.waves), "--calls", str(a.calls), "--warmup", str(a.warmup),
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
        lines.append("# verdict: MISSED -- the LDS flavour disagrees with the register flavour's or the bfloat16 index's bits in a row of the table")
    else:
        lines.append("# verdict: the LDS flavour returns the register flavour's and the bfloat16 index's bits in every row of the table")
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
