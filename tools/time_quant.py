"""p50 per call with and without the int8 shadow (hdb_index_quantize), through the drop-in entry points on a registered handle.

One line per shape: plain (use_quant = 0) and quantized (quant_min_n = 0, i.e. the shadow whatever the dispatch rule says) p50 in
microseconds, measured interleaved (A, B, A, B, ...) on the same handle, the speed-up, the candidate count of the quantized call
and a check that the quantized call returned the indices and score bits of the VALU scan (use_mfma = 0, use_fused = 0).
Usage: python tools/time_quant.py [--reps 40] [--extra] [--only I]  (--extra adds the shapes used to place the dispatch
crossover quant_min_n; --only times shape I alone, for a rocprofv3 run).

--auto times the AUTOMATIC shadow instead (option auto_quant: a default fp16 index builds the shadow on its first eligible call and
the rescoring returns the matrix cores' bits): fp16 shapes from 2M to 10M rows, one and four queries, the check is bit identity
with the default path (use_quant = 0), and the last column is the one-off cost of the first eligible call (allocation + one pass
over the matrix).  The automatic row threshold (HDB_QUANT_AUTO_MIN_ROWS, hdb_api.hip) cites this table.
"""
import argparse
import sys
import time

sys.path.insert(0, "local-hyperdb_amd")
sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hyperdb.ranking_algorithm as ranking  # noqa: E402

SHAPES = [  # (dtype, n, d, queries); "plain" is the default path (matrix cores / single launch where they apply)
    (torch.float16, 10_000_000, 384, 1),
    (torch.float32, 1_000_000, 384, 1),
    (torch.float16, 1_250_000, 384, 1),
    (torch.float16, 100_000, 384, 1),
    (torch.float32, 2_000_000, 384, 4),
]
EXTRA = [
    (torch.float16, 2_500_000, 384, 1),
    (torch.float16, 5_000_000, 384, 1),
    (torch.float16, 10_000_000, 384, 4),
    (torch.float16, 750_000, 384, 1),
    (torch.float16, 1_000_000, 384, 1),
    (torch.float32, 250_000, 384, 1),
    (torch.float32, 500_000, 384, 1),
    (torch.float32, 1_000_000, 384, 4),
]


AUTO = [(torch.float16, n, 384, nq) for n in (2_000_000, 2_500_000, 3_000_000, 5_000_000, 10_000_000) for nq in (1, 4)]


def call(h, Q, k):
    if Q.shape[0] == 1:
        return ranking.hyperDB_ranking_algorithm_sort(h, Q[0], top_k=k, metric="cosine_similarity")
    return ranking.rank_batch(h, Q, top_k=k, metric="cosine_similarity")


def flat(r):
    if isinstance(r, tuple):
        return [np.asarray(r[0]), np.asarray(r[1])]
    return [np.asarray(x) for pair in r for x in pair]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--extra", action="store_true")
    ap.add_argument("--only", type=int, default=-1, help="time only shape number ONLY of the list (profiling runs)")
    ap.add_argument("--auto", action="store_true", help="the automatic shadow (matrix-core bits) instead of the explicit one")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(5)
    print(f"{'dtype':8s} {'rows':>10s} {'d':>4s} {'nq':>3s} {'plain us':>9s} {'int8 us':>9s} {'speed-up':>8s} {'cands':>6s} same"
          + ("  first call ms" if args.auto else ""), flush=True)
    shapes = AUTO if args.auto else SHAPES + (EXTRA if args.extra else [])
    if args.only >= 0:
        shapes = [shapes[args.only]]
    for dt, n, d, nq in shapes:
        V = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(dt)
        h = ranking.register_vectors(V, quantize=None if args.auto else "int8")
        ix = h.index
        Q = np.random.default_rng(n + nq).standard_normal((nq, d)).astype(np.float32)
        k = 100

        def plain():
            ix.set_option("use_quant", 0)
            return call(h, Q, k)

        def quant():
            ix.set_option("use_quant", 1)
            ix.set_option("quant_min_n", 0)
            return call(h, Q, k)

        first_ms = 0.0
        if args.auto:
            plain()                               # (workspace, pinned record: not part of the shadow's first call)
            torch.cuda.synchronize()
            t0 = time.perf_counter(); b = quant(); first_ms = (time.perf_counter() - t0) * 1e3
            took = ix.stat("quant") & ix.stat("quant_auto") & ix.stat("mfma")
            cands = ix.stat("quant_cands")
            a = plain()                           # the default path's answer, which the automatic shadow reproduces bit for bit
        else:
            b = quant()
            took = ix.stat("quant")
            cands = ix.stat("quant_cands")
            ix.set_option("use_quant", 0); ix.set_option("use_mfma", 0); ix.set_option("use_fused", 0)
            a = call(h, Q, k)                     # the VALU scan's answer, which the shadow reproduces bit for bit
            ix.set_option("use_mfma", 1); ix.set_option("use_fused", 1)
        same = all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))
        for _ in range(5):
            plain(); quant()
        ta, tb = [], []
        for _ in range(args.reps):
            ix.set_option("use_quant", 0)
            t0 = time.perf_counter(); call(h, Q, k); ta.append(time.perf_counter() - t0)
            ix.set_option("use_quant", 1)
            t0 = time.perf_counter(); call(h, Q, k); tb.append(time.perf_counter() - t0)
        pa, pb = np.median(ta) * 1e6, np.median(tb) * 1e6
        print(f"{str(dt)[6:]:8s} {n:10d} {d:4d} {nq:3d} {pa:9.1f} {pb:9.1f} {pa / pb:8.2f} {cands:6d} {same and took == 1}"
              + (f"  {first_ms:8.2f}" if args.auto else ""), flush=True)
        h.close()
        del V, h, ix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
