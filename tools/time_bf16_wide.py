"""bfloat16 rows wider than 512 elements: call latency of cosine top-100 batches through the K slices on the bf16 matrix cores
(hdb_mfma_bf16_ks.hip) against the VALU scan of the same index (use_mfma = 0: four queries per pass over the matrix, the path
every such call took before the slices existed).

One child process per shape, each under a time limit of its own (--limit seconds); the parent never opens the GPU, and the first
shape that fails or runs into its limit ends the run.  In a child: ONE index, the two settings take turns call by call
(set_option between the calls), so drift of the clock or of the machine hits both alike; p50 over --calls synchronous calls
(rank_batch: host queries in, host results out) after --warmup calls per setting.  The answers of the two settings are compared
once per shape and query count (same rows up to ties inside the float32 contract's band).

Claims checked: from 16 queries on the slices are faster than the VALU scan at every measured point; 5 and 8 queries are recorded
and decide the planner's threshold for the width (hdb_mfma_bf16_ks_min_q in hdb_caps.h; the tool sets bf16_ks_min_q = 5, so the
slices run from 5 queries on whatever that rule says).

    python tools/time_bf16_wide.py [--shapes 1000000x768 1000000x1024 500000x1536] [--queries 5 8 16 64 128] [--calls 60]
                                   [--warmup 5] [--limit 240] [--out profiles/bf16_wide_time.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "local-hyperdb_amd"))
sys.path.insert(0, ROOT)

HEADER = f"# {'rows':>10} {'d':>5} {'queries':>7} {'slices':>10} {'VALU scan':>10} {'VALU/slices':>11}  mfma  same answer  claim"


def one_shape(n, d, queries, calls, warmup):
    """-> the table's lines for one shape (a child process runs this)."""
    import numpy as np
    import torch
    import hyperdb.ranking_algorithm as ranking
    from oracle import ranking_oracle as orc
    assert torch.cuda.is_available(), "time_bf16_wide.py measures on the GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(n + d)
    Vb = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    h = ranking.register_vectors(Vb)
    h.index.set_option("bf16_ks_min_q", 5)               # the slices from 5 queries on at every width: the table is what the planner's rule is read from
    rng = np.random.default_rng(7)

    def call(Q, mfma):
        h.index.set_option("use_mfma", mfma)
        t0 = time.perf_counter()
        out = ranking.rank_batch(h, Q, top_k=100, metric="cosine_similarity")        # (returns host arrays: the call has ended)
        return (time.perf_counter() - t0) * 1e6, out

    lines = []
    for nq in queries:
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        for _ in range(warmup):
            call(Q, 1); call(Q, 0)
        _, (mi, ms) = call(Q, 1)
        used = h.index.stat("mfma")
        _, (vi, vs) = call(Q, 0)
        same = all(orc.same_result_modulo_ties(mi[q], ms[q], vi[q], vs[q], 1e-5) for q in range(nq))
        t = [[], []]
        for _ in range(calls):
            t[0].append(call(Q, 1)[0])
            t[1].append(call(Q, 0)[0])
        p = [float(np.median(x)) for x in t]
        claim = "recorded" if nq < 16 else ("holds" if p[0] < p[1] else "MISSED")
        lines.append(f"  {n:>10} {d:>5} {nq:>7} {p[0]:>10.1f} {p[1]:>10.1f} {p[1] / p[0]:>11.2f}  {used:>4}  {'yes' if same else 'NO':>11}  {claim}")
        print(lines[-1], flush=True)
    h.index.set_option("use_mfma", 1)
    h.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1000000x768", "1000000x1024", "500000x1536"])
    ap.add_argument("--queries", type=int, nargs="+", default=[5, 8, 16, 64, 128])
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds one shape may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.calls >= 50, "p50 over at least 50 calls"
    if a.child:
        n, d = (int(x) for x in a.child.split("x"))
        for line in one_shape(n, d, a.queries, a.calls, a.warmup):
            print("ROW" + line)
        return 0
    lines = [f"# tools/time_bf16_wide.py: cosine top-100 on a bf16 index, p50 of {a.calls} calls in us (host queries in, host results out), "
             f"{a.warmup} warm-up calls per setting,",
             "# K slices on the bf16 matrix cores (bf16_ks_min_q = 5) against use_mfma = 0 (the VALU scan, four queries per pass) on the same index, alternating call by call",
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
    elif any("MISSED" in line or " NO " in line for line in table):
        lines.append("# verdict: MISSED -- a point from 16 queries on is not faster through the slices, or the two settings disagree")
    else:
        lines.append("# verdict: from 16 queries on the K slices are faster than the VALU scan in every row of the table; the two settings agree in every row")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if failed:
        print(failed, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
