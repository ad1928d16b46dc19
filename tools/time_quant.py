"""p50 per call with and without the int8 shadow (hdb_index_quantize), through the drop-in entry points on a registered handle.

One line per shape: plain (use_quant = 0) and quantized (quant_min_n = 0, i.e. the shadow whatever the dispatch rule says) p50 in
microseconds, measured interleaved (A, B, A, B, ...) on the same handle, the speed-up, the candidate count of the quantized call
and a check that the quantized call returned the indices and score bits of the VALU scan (use_mfma = 0, use_fused = 0).
Usage: python tools/time_quant.py [--reps 40] [--extra] [--only I]  (--extra adds the shapes used to place the dispatch
crossover quant_min_n; --only times shape I alone, for a rocprofv3 run).

--auto times the AUTOMATIC shadow instead (option auto_quant: a default fp16 index builds the shadow on its first eligible call and
the rescoring returns the matrix cores' bits): fp16 shapes from 2M to 10M rows, one and four queries, the check is bit identity
with the default path (use_quant = 0), and the last column is the one-off cost of the first eligible call (allocation + one pass
over the matrix).  The automatic row threshold (HDB_QUANT_AUTO_MIN_ROWS, hdb_api.hip) cites this table.  The int8 column is the
shadow WITHOUT the 5-bit plane (use_plane = 0); one-query shapes get two more columns, the shadow behind the plane (plane_min_n =
0) and the rows its first pass kept (plane_survivors), all columns interleaved in one process on one index.  The plane's row rule
(HDB_PLANE_MIN_ROWS, hdb_api.hip) cites that table, profiles/quant_plane_time.txt.

--auto --plane-grid [--rows ...] [--dims ...] [--wg 4 5 6 7] times the one-query call behind the plane at several grids of its pass
(option plane_wg_per_cu; plane_grid_table below); the table HDB_PLANE_WG_PER_CU (hdb_caps.h) cites it, profiles/plane_occupancy_time.txt.

--auto --batch [--rows ...] [--dims ...] [--queries ...] times batches of 5+ queries through the automatic shadow (batch_table
below); the row rule of batches (quant_batch_rule, hdb_api.hip) cites that table, profiles/quant_batch_time.txt.
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


def batch_table(args):
    """--auto --batch: batches of 5+ queries through the automatic shadow (hdb_quant_mfma.hip).  Per (rows, d): one matrix, one
    index, one process; per query count the parent path (use_quant = 0), the shadow with the int8 matrix-core filter
    (quant_batch_kernel = 1) and the shadow with the v_dot4 scan (quant_batch_kernel = 0) alternate, p50 of --reps calls each (the
    v_dot4 column takes a quarter of the repetitions: it reads the shadow once per four queries).  Lists: min / median / max
    candidates per query of the matrix-core call.  same: indices and score bits of both shadow calls equal the parent's.  The
    first shadow call of an index builds the shadow; its wall time is the last column of that row."""
    g = torch.Generator(device="cuda").manual_seed(5)
    print(f"{'rows':>10s} {'d':>4s} {'nq':>4s} {'parent us':>10s} {'i8 mfma us':>10s} {'speed-up':>8s} {'v_dot4 us':>10s} "
          f"{'lists min/med/max':>18s} same  first call ms", flush=True)
    for n in args.rows:
        for d in args.dims:
            V = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
            h = ranking.register_vectors(V)
            ix = h.index
            ix.set_option("quant_batch_min_n", 0)
            first = True
            for nq in args.queries:
                Q = np.random.default_rng(n + nq).standard_normal((nq, d)).astype(np.float32)
                k = 100

                def run(use_quant, kernel):
                    ix.set_option("use_quant", use_quant)
                    ix.set_option("quant_batch_kernel", kernel)
                    return call(h, Q, k)

                a = run(0, 1)
                torch.cuda.synchronize()
                t0 = time.perf_counter(); b = run(1, 1); first_ms = (time.perf_counter() - t0) * 1e3
                took = ix.stat("quant") & ix.stat("quant_auto") & ix.stat("mfma")
                lists = (ix.stat("quant_cands_min"), ix.stat("quant_cands_median"), ix.stat("quant_cands"))
                c = run(1, 0)
                took &= ix.stat("quant")
                same = all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b))) and all(np.array_equal(x, y) for x, y in zip(flat(a), flat(c)))
                for _ in range(3):
                    run(0, 1); run(1, 1)
                ta, tb, tc = [], [], []
                for r in range(args.reps):
                    t0 = time.perf_counter(); run(0, 1); ta.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); run(1, 1); tb.append(time.perf_counter() - t0)
                    if r % 4 == 0:
                        t0 = time.perf_counter(); run(1, 0); tc.append(time.perf_counter() - t0)
                pa, pb, pc = np.median(ta) * 1e6, np.median(tb) * 1e6, np.median(tc) * 1e6
                print(f"{n:10d} {d:4d} {nq:4d} {pa:10.1f} {pb:10.1f} {pa / pb:8.2f} {pc:10.1f} "
                      f"{'%d/%d/%d' % lists:>18s} {same and took == 1}" + (f"  {first_ms:8.2f}" if first else ""), flush=True)
                first = False
            h.close()
            del V, h, ix
            torch.cuda.empty_cache()


def plane_grid_table(args):
    """--auto --plane-grid [--rows ...] [--dims ...] [--wg 4 5 6 7]: the one-query call behind the 5-bit plane at several grids of its
    pass (option plane_wg_per_cu, workgroups per CU; 0 = the table of hdb_caps.h).  Per (rows, d): one matrix, one index, one
    process; the settings alternate call by call.  Per setting: p50 of --reps calls (wall, us) and p50 of the plane pass alone (us,
    HIP events around its launch: option profile, stat scan_time_ns -- taken in calls of their own, the events cost the call a few
    us), the workgroups of the pass (plane_blocks).  same: every setting returned the indices and score bits of the first and kept
    the same rows (plane_survivors, quant_cands).  HDB_PLANE_WG_PER_CU (hdb_caps.h) cites this table,
    profiles/plane_occupancy_time.txt."""
    g = torch.Generator(device="cuda").manual_seed(5)
    print(f"{'rows':>10s} {'d':>4s} " + " ".join(f"{'wg ' + str(w) + ': call / pass us (blocks)':>34s}" for w in args.wg) + "  same", flush=True)
    for d in args.dims:
        for n in args.rows:
            V = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
            h = ranking.register_vectors(V)
            ix = h.index
            ix.set_option("quant_min_n", 0)
            ix.set_option("plane_min_n", 0)
            Q = np.random.default_rng(n + 1).standard_normal((1, d)).astype(np.float32)
            k = 100

            def run(w):
                ix.set_option("plane_wg_per_cu", w)
                return call(h, Q, k)

            first, same, blocks = None, True, {}
            for w in args.wg:
                r = flat(run(w))
                same = same and ix.stat("quant") == 1 and ix.stat("plane") == 1
                blocks[w] = ix.stat("plane_blocks")
                kept = (ix.stat("plane_survivors"), ix.stat("quant_cands"))
                if first is None:
                    first = (r, kept)
                same = same and kept == first[1] and all(np.array_equal(x, y) for x, y in zip(r, first[0]))
            for _ in range(5):
                for w in args.wg:
                    run(w)
            tc = {w: [] for w in args.wg}
            tp = {w: [] for w in args.wg}
            for _ in range(args.reps):
                for w in args.wg:
                    t0 = time.perf_counter(); run(w); tc[w].append(time.perf_counter() - t0)
            for _ in range(args.reps):
                for w in args.wg:
                    ix.set_option("profile", 1)
                    run(w)
                    tp[w].append(ix.stat("scan_time_ns") * 1e-3)
            ix.set_option("profile", 0)
            print(f"{n:10d} {d:4d} " + " ".join(f"{np.median(tc[w]) * 1e6:15.1f} / {np.median(tp[w]):7.1f} ({blocks[w]:5d})" for w in args.wg)
                  + f"  {same}", flush=True)
            h.close()
            del V, h, ix
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane-grid", action="store_true", help="with --auto: the plane pass at several grids (plane_wg_per_cu)")
    ap.add_argument("--wg", type=int, nargs="+", default=[4, 5, 6, 7], help="with --plane-grid: the workgroups per CU to compare")
    ap.add_argument("--batch", action="store_true", help="with --auto: batches of 5+ queries (parent path, int8 matrix cores, v_dot4 scan)")
    ap.add_argument("--rows", type=int, nargs="+", default=[2_000_000, 5_000_000, 10_000_000])
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 384, 512])
    ap.add_argument("--queries", type=int, nargs="+", default=[5, 8, 16, 64, 128, 256])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--extra", action="store_true")
    ap.add_argument("--only", type=int, default=-1, help="time only shape number ONLY of the list (profiling runs)")
    ap.add_argument("--auto", action="store_true", help="the automatic shadow (matrix-core bits) instead of the explicit one")
    args = ap.parse_args()
    if args.batch:
        return batch_table(args)
    if args.plane_grid:
        return plane_grid_table(args)
    g = torch.Generator(device="cuda").manual_seed(5)
    print(f"{'dtype':8s} {'rows':>10s} {'d':>4s} {'nq':>3s} {'plain us':>9s} {'int8 us':>9s} {'speed-up':>8s} {'cands':>6s} same"
          + ("  first call ms  plane us  vs int8  survivors" if args.auto else ""), flush=True)
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

        def quant(plane=0):
            ix.set_option("use_quant", 1)
            ix.set_option("quant_min_n", 0)
            ix.set_option("use_plane", plane)
            ix.set_option("plane_min_n", 0)
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
        with_plane = args.auto and nq == 1
        surv = 0
        if with_plane:
            c = quant(1)
            took &= ix.stat("plane")
            surv = ix.stat("plane_survivors")
            same = same and all(np.array_equal(x, y) for x, y in zip(flat(a), flat(c))) and ix.stat("quant_cands") == cands
        for _ in range(5):
            plain(); quant(0)
            if with_plane:
                quant(1)
        ta, tb, tc = [], [], []
        for _ in range(args.reps):
            ix.set_option("use_quant", 0)
            t0 = time.perf_counter(); call(h, Q, k); ta.append(time.perf_counter() - t0)
            ix.set_option("use_quant", 1); ix.set_option("use_plane", 0)
            t0 = time.perf_counter(); call(h, Q, k); tb.append(time.perf_counter() - t0)
            if with_plane:
                ix.set_option("use_plane", 1)
                t0 = time.perf_counter(); call(h, Q, k); tc.append(time.perf_counter() - t0)
        pa, pb = np.median(ta) * 1e6, np.median(tb) * 1e6
        tail = ""
        if args.auto:
            tail = f"  {first_ms:8.2f}"
            if with_plane:
                pc = np.median(tc) * 1e6
                tail += f"      {pc:9.1f} {pb / pc:8.2f} {surv:10d}"
        print(f"{str(dt)[6:]:8s} {n:10d} {d:4d} {nq:3d} {pa:9.1f} {pb:9.1f} {pa / pb:8.2f} {cands:6d} {same and took == 1}" + tail, flush=True)
        h.close()
        del V, h, ix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
