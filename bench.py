#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native HyperDB ranking path.

Metric (BASELINE.json): queries/sec + p50 latency, N=10M d=384 fp16 top-100 at 1/2/4/8 MI355X.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A step is one query call of the hot path over the whole stored matrix: metric scoring of all N rows
+ top-100, results copied back to the host (what HyperDB.query() does per call).  The matrix is
resident in HBM before the timed region (synthetic standard-normal rows, seeded per 250k-row block so
shards are identical for every GPU count).  With N GPUs the 10M rows are row-sharded (strong
scaling: total work fixed); each rank scans its shard and the per-shard top-100 records (1.2 KB) are exchanged ONCE per
query and merged on every rank: on one node through a shared-memory swap of the host records every rank produces anyway
(hyperdb/sharded.py HostExchange + hdb_merge_topk_host), records above 64 KiB (the Q=256 leg) and HDB_EXCHANGE=collective
through ONE RCCL all-gather + the merge kernel.

HDB_BENCH_REHEARSAL=1 rehearses the N > 1 control flow on ONE GPU (every rank on device 0, gloo for the bookkeeping
collectives): it checks that the multi-rank path runs end to end; its timings mean nothing.

One JSON line is printed by rank 0.  A plain run sets up, warms up, times the --steps query calls and prints the line: the
contract fields (metric, value, unit, higher_is_better, dtype, ms_per_step = milliseconds of one timed step) and
  roofline      -- dominant kernel (the pass over all of V) timed with HIP events on its launch
                   stream inside the timed region; algorithmic bytes = rows * d * sizeof(elem).
--dump-outputs DIR writes what the last timed step returned to its caller (top-k row indices as float64, scores as float32)
to DIR/indices.npy and DIR/scores.npy; with the same arguments the inputs are the same from run to run.
Everything else is measured only with --full (the keys below are null or absent without it):
  cpu_baseline  -- the numpy restatement of the reference (oracle/), timed on this host on a bounded
                   row prefix and scaled linearly to N (rank 0, --gpus 1 only).
  batched       -- config 3 of BASELINE.json (Q=256 dot-product) measured in the same run.
  api           -- (--gpus 1) p50 of the SAME query stream through the drop-in entry points, numpy queries on the host:
                   ranking.hyperDB_ranking_algorithm_sort(handle, q, top_k) and HyperDB.query(q, top_k) (reference
                   ranking_algorithm.py:149, hyperdb.py:1584), beside the p50 of the kernel path the headline times.
  exchange_alt  -- (--gpus N > 1) both transports of the per-query exchange are timed in the same run: `value` uses the one
                   named in config.exchange (chosen by a calibration inside the warm-up), exchange_alt reports the other.
  extra         -- (--gpus 1, default legs c2,c5,hamming,shard,f32batch,small) the other BASELINE.json configs and the supplementary
                   workloads, each with workload / kernel / kernel_us / roofline{achieved, peak, frac, algorithmic_bytes_per_launch}:
                   c2 = config 2 (N=1M fp32 cosine), c5 = config 5 (N=10M d=768 euclidean + time decay, Q=64), hamming = the
                   headline matrix through hamming_distance, shard = the per-GPU share of the headline at 8 GPUs (N=1.25M),
                   f32batch = 64 cosine queries on a float32 2M x 384 matrix (rows multiplied as bf16 parts; + roofline_mfma),
                   small = p50 of the drop-in entry point on reference-sized matrices (1k / 10k / 100k rows, host numpy queries).
  rccl          -- (--gpus N > 1) {backend, world, devices: [(rank, host, local device, pci bus id) all-gathered from the ranks],
                   exchange, record_bytes} and `parity`: the sharded answer on a 1M-row prefix of the same matrix against rank 0's
                   single-index answer (identical: bool, crc32 of the index lists) -- N ranks on N devices and index parity in one line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "local-hyperdb_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# dmabuf IPC for RCCL / cross-process GPU buffers on this driver; read when the HIP runtime initialises, so set it
# before torch is imported (it is normally exported already)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16 MFMA
BLOCK_ROWS = 250_000
DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: all arrays together


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--n", "--rows", dest="n", type=int, default=10_000_000)      # (--rows: torch.distributed.run takes a bare --n for its own options)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--metric", default="cosine_similarity")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's top-k indices and scores to DIR/indices.npy, DIR/scores.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg besides the headline: batched, api, cpu baseline, extra legs, exchange_alt, rccl")
    ap.add_argument("--batch-q", type=int, default=256, help="(--full) batched leg (config 3); 0 disables")
    ap.add_argument("--batch-steps", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-rows", type=int, default=1_000_000, help="(--full) row prefix the CPU baseline is timed on (BASELINE.md section 4)")
    ap.add_argument("--extra", default="c2,c5,hamming,shard,f32batch,small",
                    help="(--full) comma list of extra legs timed after the headline (one GPU): c2,c5,hamming,shard,f32batch,small; '' = none")
    ap.add_argument("--pmc-traffic", type=float, default=None,
                    help="HBM bytes per launch of the dominant kernel from a separate rocprofv3 --pmc run")
    return ap.parse_args(argv)


def dump_outputs(out_dir, idx, sc):
    """What the timed path returned in its last step: row indices (int64, exact in float64) and scores (float32).  Above
    DUMP_MAX_BYTES (a --k near N) a fixed, seeded sample of the ranks is written, the same columns of both arrays."""
    idx, sc = np.asarray(idx), np.asarray(sc)
    per_rank = idx.shape[0] * (8 + 4)
    if idx.shape[1] * per_rank > DUMP_MAX_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(idx.shape[1], DUMP_MAX_BYTES // per_rank, replace=False))
        idx, sc = idx[:, keep], sc[:, keep]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "indices.npy"), idx.astype(np.float64))
    np.save(os.path.join(out_dir, "scores.npy"), sc.astype(np.float32))


def make_shard(n_total, d, dtype, rank, world, device):
    """Rows [lo, hi) of the global matrix; block b is N(0,1) from torch.Generator(seed=1234+b)."""
    nblk = (n_total + BLOCK_ROWS - 1) // BLOCK_ROWS
    b_lo = rank * nblk // world
    b_hi = (rank + 1) * nblk // world
    lo, hi = b_lo * BLOCK_ROWS, min(b_hi * BLOCK_ROWS, n_total)
    V = torch.empty((hi - lo, d), dtype=dtype, device=device)
    for b in range(b_lo, b_hi):
        g = torch.Generator(device=device).manual_seed(1234 + b)
        r0 = b * BLOCK_ROWS
        r1 = min(r0 + BLOCK_ROWS, n_total)
        V[r0 - lo:r1 - lo] = torch.randn((r1 - r0, d), generator=g, device=device, dtype=torch.float32).to(dtype)
    return V, lo, hi


def make_queries(nq, d, dtype, device):
    g = torch.Generator(device=device).manual_seed(4321)
    return torch.randn((nq, d), generator=g, device=device, dtype=torch.float32).to(dtype)


def cpu_baseline(args, V_dev, Q_dev):
    """Reference op sequence (oracle.rank == hyperDB_ranking_algorithm_sort) on a 1M-row prefix, scaled linearly to N
    (BASELINE.md section 4), and beside it "numpy_best": rows pre-normalised once, float32 BLAS GEMV + argpartition per
    query -- clearly NOT the reference, shown so that the speed-up is not only the reference's redundant passes."""
    from oracle import ranking_oracle as orc
    rows = min(args.cpu_rows, V_dev.shape[0])
    Vh = V_dev[:rows].cpu().numpy()
    q = Q_dev[0].cpu().numpy()
    orc.rank(Vh[:1000], q, top_k=args.k, metric=args.metric)       # warm numpy
    times = []
    t_end = time.perf_counter() + 22.0
    while len(times) < 3 and (time.perf_counter() < t_end or not times):
        t0 = time.perf_counter()
        orc.rank(Vh, q, top_k=args.k, metric=args.metric)
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    scale = args.n / rows
    try:
        from threadpoolctl import threadpool_info
        blas_threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    except Exception:
        blas_threads = os.cpu_count()
    cores = 1 if Vh.dtype == np.float16 else blas_threads   # fp16 np.dot has no BLAS kernel: single core
    # numpy-best: what a tuned numpy user could do (not the reference): normalise once, sgemv per query
    V32 = Vh.astype(np.float32)
    if args.metric == "cosine_similarity":
        V32 /= np.maximum(np.linalg.norm(V32, axis=1, keepdims=True), 1e-30)
    q32 = q.astype(np.float32)
    bt = []
    for _ in range(5):
        t0 = time.perf_counter()
        sc = V32 @ q32
        top = np.argpartition(sc, -args.k)[-args.k:]
        top = top[np.argsort(-sc[top])]
        bt.append(time.perf_counter() - t0)
    tb = float(np.median(bt))
    return {
        "value": 1.0 / (t * scale), "unit": "queries/s", "cores": int(cores), "kind": "port",
        "sample": f"oracle.rank ({args.metric}, top-{args.k}) on the first {rows} rows, median of {len(times)} "
                  f"queries = {t:.3f} s, scaled x{scale:.0f} to N={args.n}; host has {os.cpu_count()} cpus, "
                  f"BLAS threads {blas_threads}",
        "numpy_best": {"value": 1.0 / (tb * scale), "unit": "queries/s", "cores": int(blas_threads),
                       "note": f"NOT the reference: rows pre-normalised once (untimed), float32 sgemv + argpartition, "
                               f"median of 5 = {tb:.4f} s on {rows} rows, scaled x{scale:.0f}"},
    }


def extra_leg(name, device):
    """Other BASELINE.json configs, single GPU: returns a dict for the JSON line."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    if name == "c2":      # N=1M d=384 fp32 single-query cosine top-100 (HBM-bound GEMV path)
        n, d, dt, elem, q, metric, steps, bias = 1_000_000, 384, torch.float32, 4, 1, "cosine_similarity", 200, False
    elif name == "c5":    # N=10M d=768 fp16 euclidean + time-decay re-rank, batch-Q=64
        n, d, dt, elem, q, metric, steps, bias = 10_000_000, 768, torch.float16, 2, 64, "euclidean_metric", 10, True
    elif name == "hamming":   # supplementary: the headline matrix through hamming_distance
        n, d, dt, elem, q, metric, steps, bias = 10_000_000, 384, torch.float16, 2, 1, "hamming_distance", 200, False
    elif name == "shard":     # what one GPU of an 8-GPU node holds of the headline matrix (strong scaling): the call that bounds the 8-GPU QPS
        n, d, dt, elem, q, metric, steps, bias = 1_250_000, 384, torch.float16, 2, 1, "cosine_similarity", 300, False
    elif name == "f32batch":  # the reference's default precision (hyperdb.py:51) in batches: float32 rows as bf16 parts on the matrix cores (hdb_mfma_f32s.hip)
        n, d, dt, elem, q, metric, steps, bias = 2_000_000, 384, torch.float32, 4, 64, "cosine_similarity", 30, False
    elif name == "small":
        return small_leg(device)
    else:
        raise SystemExit(f"unknown extra config {name}")
    V, lo, hi = make_shard(n, d, dt, 0, 1, device)
    ix = GpuIndex(V, device=device)
    if bias:
        g = torch.Generator(device=device).manual_seed(99)
        ts = 1.7e9 + torch.rand(n, generator=g, device=device, dtype=torch.float64) * 30 * 86400.0
        ix.set_recency(ts, 0.5)
    Q = make_queries(q * 4, d, dt, device).to(torch.float32)
    mid = METRIC_IDS[metric]
    for i in range(3):
        ix.topk(Q[:q], 100, mid)
    ix.set_option("profile", 1)
    torch.cuda.synchronize()
    lat = []
    t0 = time.perf_counter()
    for i in range(steps):
        t1 = time.perf_counter()
        ix.topk(Q[(i % 4) * q:(i % 4 + 1) * q], 100, mid)
        lat.append(time.perf_counter() - t1)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ns, nl = ix.stat("scan_time_ns"), ix.stat("scan_launches")
    kern_s = ns * 1e-9 / max(nl, 1)
    alg = n * d * elem
    if metric == "hamming_distance":
        alg = n * ((d + 31) // 32) * 4              # packed sign bits, word-major: what the scan reads (one-time pack excluded)
    traffic = None
    try:                                                     # HBM bytes per launch from separate rocprofv3 --pmc passes (profiles/hbm_traffic.json)
        tj = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
        traffic = tj.get(f"n={n},d={d},{'fp32' if elem == 4 else 'fp16'},q={q},{metric}", {}).get("hbm_bytes_per_launch")
    except Exception:
        traffic = None
    fused = ix.stat("fused")
    kernel = {1: "hdb_mfma_fused_kernel", 2: "hdb_mfma_kernel MODE 2", 3: "hdb_bits_fused_kernel"}.get(fused, "hdb_mfma_kernel / hdb_scan_kernel filter pass")
    out = {"config": name, "workload": f"N={n} d={d} {'fp32' if elem == 4 else 'fp16'} Q={q} {metric}{' + recency bias' if bias else ''} top-100",
           "qps": q * steps / el, "ms_per_call": 1e3 * el / steps, "p50_ms": 1e3 * float(np.median(lat)),
           "kernel": kernel + (" (single launch: the whole call)" if fused else ""), "launches_timed": nl,
           "kernel_us": kern_s * 1e6, "mfma_path": bool(ix.stat("mfma")), "single_launch": bool(fused),
           "roofline": {"bound": "hbm", "achieved": alg / kern_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": alg / kern_s / 1e9 / HBM_PEAK_GBS, "traffic": traffic, "algorithmic_bytes_per_launch": alg}}
    if name == "f32batch":     # the matrix-pipe side of the same launch: algorithmic flops (2 Q d per row) and what the pipe multiplies for them
        parts = bool(ix.stat("f32_split"))
        flops = 2.0 * n * q * d
        out["bf16_parts"] = parts
        out["roofline_mfma"] = {"bound": "mfma", "achieved": flops / kern_s / 1e12, "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                                "frac": flops / kern_s / 1e12 / MFMA_F16_PEAK_TFLOPS, "algorithmic_flops_per_launch": flops,
                                "products_per_flop": 5 if parts else 1,
                                "pipe_tflops": (5 if parts else 1) * flops / kern_s / 1e12}
    ix.close()
    del V
    torch.cuda.empty_cache()
    return out


def small_leg(device):
    """Reference-sized matrices (the reference's perf test uses 10 000 documents, its demo 151: tests/perf_hyperdb.py:15): p50 of
    hyperDB_ranking_algorithm_sort(handle, q_numpy, top_k=100) -- the drop-in entry point, host query in, host result out."""
    import hyperdb.ranking_algorithm as ranking
    rows = []
    for dt, npdt in ((torch.float16, np.float16), (torch.float32, np.float32)):
        for n in (1_000, 10_000, 100_000):
            V, _, _ = make_shard(n, 384, dt, 0, 1, device)
            h = ranking.register_vectors(V)
            qs = make_queries(32, 384, dt, device).cpu().numpy().astype(npdt)
            for metric in ("cosine_similarity", "hamming_distance"):
                for i in range(10):
                    ranking.hyperDB_ranking_algorithm_sort(h, qs[i].copy(), top_k=100, metric=metric)
                t = np.empty(200)
                for i in range(200):
                    q = qs[i % 32].copy()
                    t0 = time.perf_counter()
                    ranking.hyperDB_ranking_algorithm_sort(h, q, top_k=100, metric=metric)
                    t[i] = time.perf_counter() - t0
                rows.append({"rows": n, "dtype": "fp16" if dt == torch.float16 else "fp32", "metric": metric,
                             "p50_us": 1e6 * float(np.median(t)), "p99_us": 1e6 * float(np.percentile(t, 99)),
                             "single_launch": h.index.stat("fused"), "local_flavour": bool(h.index.stat("local"))})
            h.close()
            del V
    torch.cuda.empty_cache()
    return {"config": "small", "workload": "d=384 Q=1 top-100 through hyperDB_ranking_algorithm_sort(handle, q_numpy), host to host",
            "p50_by_rows": rows}


def rccl_block(args, dist, rank, world, device, sharded_kind, tdtype, mid):
    """N > 1: which ranks sat on which devices (all-gathered), what the exchange moved, and index parity of the sharded path against
    rank 0's single index on a 1M-row prefix of the same matrix (block seeds make the prefix identical for every GPU count)."""
    import socket
    import zlib
    from hyperdb._native import GpuIndex, packed_bytes
    from hyperdb.sharded import ShardedIndex
    props = torch.cuda.get_device_properties(device)
    mine = {"rank": rank, "host": socket.gethostname(), "device": device.index,
            "pci_bus_id": getattr(props, "pci_bus_id", None), "uuid": str(getattr(props, "uuid", "")) or None}
    devs = [None] * world
    dist.all_gather_object(devs, mine)
    n_pre = min(1_000_000, args.n)
    Vp, plo, phi = make_shard(n_pre, args.d, tdtype, rank, world, device)
    loc = GpuIndex(Vp, device=device, row_base=plo)
    sh = ShardedIndex(loc, n_total=n_pre, group=dist.group.WORLD, exchange="host" if "shared-memory" in sharded_kind else "collective")
    Qp = make_queries(8, args.d, tdtype, device).to(torch.float32)
    got_i, got_s = sh.query(Qp, args.k, mid)
    ident, crc = None, zlib.crc32(np.ascontiguousarray(got_i).tobytes())
    if rank == 0:                                           # (no collective in here: a failure must not leave the other ranks waiting)
        try:
            Vw, _, _ = make_shard(n_pre, args.d, tdtype, 0, 1, device)
            whole = GpuIndex(Vw, device=device)
            wi, ws = whole.topk(Qp, args.k, mid)
            ident = bool(np.array_equal(wi, got_i) and np.array_equal(ws, got_s))
            whole.close()
            del Vw
        except Exception as e:                               # noqa: BLE001
            ident = f"not checked: {e!r}"[:200]
    crcs = [None] * world
    dist.all_gather_object(crcs, crc)
    sh.close(); loc.close()
    del Vp
    torch.cuda.empty_cache()
    return {"backend": str(dist.get_backend()), "world": world, "devices": devs,
            "distinct_devices": len({(d_["host"], d_["pci_bus_id"] or d_["device"]) for d_ in devs}),
            "exchange": sharded_kind, "record_bytes": int(packed_bytes(1, args.k)),
            "parity": {"rows": n_pre, "queries": 8, "top_k": args.k, "sharded_equals_single_index_on_rank0": ident,
                       "index_crc32_per_rank": crcs, "ranks_agree": len(set(crcs)) == 1}}


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    if os.environ.get("HDB_BENCH_REHEARSAL") == "1":     # control-flow rehearsal of the N > 1 path on ONE GPU: every rank on
        local_rank = 0                                    # device 0, gloo for the bookkeeping collectives (timings meaningless)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or os.environ.get("HDB_FORCE_DIST") == "1":     # HDB_FORCE_DIST: exercise the RCCL path on one GPU
        import torch.distributed as dist_mod
        dist = dist_mod
        if os.environ.get("HDB_BENCH_REHEARSAL") == "1":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)

    from hyperdb._native import GpuIndex, METRIC_IDS
    from hyperdb.sharded import ShardedIndex

    tdtype = torch.float16 if args.dtype == "fp16" else torch.float32
    elem = 2 if args.dtype == "fp16" else 4
    V, lo, hi = make_shard(args.n, args.d, tdtype, rank, world, device)
    local = GpuIndex(V, device=device, row_base=lo)
    grp = dist.group.WORLD if dist else None
    force = os.environ.get("HDB_FORCE_DIST") == "1"
    sharded = ShardedIndex(local, n_total=args.n, group=grp, force_exchange=force)
    # Both transports of the per-query exchange (N > 1): the RCCL all-gather of the packed device records (+ merge kernel) and,
    # where every rank sits on this node, the shared-memory swap of the host records.  A calibration inside the warm-up picks
    # the one `value` is timed with (unless HDB_EXCHANGE names one); the other is timed afterwards as exchange_alt.
    alt = None
    if world > 1 and not os.environ.get("HDB_EXCHANGE"):
        other = "collective" if sharded._hx is not None else "host"
        try:
            alt = ShardedIndex(local, n_total=args.n, group=grp, force_exchange=force, exchange=other)
        except Exception:
            alt = None
    # queries: fp16/fp32 values as the config says, staged in the C ABI's query type (float32: exact for fp16)
    Q = make_queries(max(args.steps + args.warmup, 1), args.d, tdtype, device).to(torch.float32)
    mid = METRIC_IDS[args.metric]
    torch.cuda.synchronize()

    def barrier():
        if dist:
            dist.barrier()
        torch.cuda.synchronize()

    def kind_of(sh):
        return ("none" if world == 1 else
                "shared-memory swap of the ranks' host records + host merge, once per query" if sh._hx is not None
                else "1 RCCL all-gather of packed top-k per query + merge kernel")

    def p50_of(sh, count):
        ts = np.empty(count)
        for j in range(count):
            t0 = time.perf_counter()
            sh.query(Q[j % Q.shape[0]:j % Q.shape[0] + 1], args.k, mid)
            ts[j] = time.perf_counter() - t0
        t = torch.tensor([float(np.median(ts))], dtype=torch.float64, device=device if not (dist and dist.get_backend() == "gloo") else "cpu")
        if dist:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # ---------------- single-query leg: the headline metric --------------------------------------
    for i in range(args.warmup):
        sharded.query(Q[i:i + 1], args.k, mid)
    calib = None
    if alt is not None:                                  # calibration (untimed): every rank takes the same decision
        for i in range(min(args.warmup, 5)):
            alt.query(Q[i:i + 1], args.k, mid)
        calib = {kind_of(sharded): p50_of(sharded, 30), kind_of(alt): p50_of(alt, 30)}
        if calib[kind_of(alt)] < calib[kind_of(sharded)]:
            sharded, alt = alt, sharded
    local.set_option("profile", 1)
    barrier()
    lat = np.empty(args.steps)
    last = None
    t_start = time.perf_counter()
    for i in range(args.steps):
        t0 = time.perf_counter()
        last = sharded.query(Q[args.warmup + i:args.warmup + i + 1], args.k, mid)   # ends with D2H + sync
        lat[i] = time.perf_counter() - t0
    barrier()
    elapsed = time.perf_counter() - t_start
    if args.dump_outputs and rank == 0 and last is not None:
        dump_outputs(args.dump_outputs, *last)
    scan_ns = local.stat("scan_time_ns")
    scan_launches = local.stat("scan_launches")
    local.set_option("profile", 0)
    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    if dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    qps = args.steps / elapsed
    kern_s = scan_ns * 1e-9 / max(scan_launches, 1)
    headline_kernel = ("hdb_mfma_fused_kernel (single launch: query prep + row sample + threshold + filter pass over all rows + top-k)"
                       if local.stat("fused") == 1 else
                       "hdb_mfma_kernel MODE 2 (single launch: query prep + row sample + thresholds + filter pass over all rows + top-k)"
                       if local.stat("fused") == 2 else
                       "hdb_mfma_kernel (MFMA row scan, filter pass over all rows)" if local.stat("mfma")
                       else "hdb_scan_kernel (VALU row scan, filter pass over all rows)")
    alg_bytes = (hi - lo) * args.d * elem                    # per launch of the dominant kernel, per GPU
    achieved = alg_bytes / kern_s / 1e9 if kern_s > 0 else 0.0

    # ---------------- batched leg: config 3 (Q=256 dot product) ----------------------------------
    batched = None
    if args.full and args.batch_q > 0:
        bq = args.batch_q
        QB = make_queries(bq, args.d, tdtype, device).to(torch.float32)
        bmid = METRIC_IDS["dot_product"]
        for _ in range(2):
            sharded.query(QB, args.k, bmid)
        local.set_option("profile", 1)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.batch_steps):
            sharded.query(QB, args.k, bmid)
        barrier()
        bel = time.perf_counter() - t0
        b_ns, b_l = local.stat("scan_time_ns"), local.stat("scan_launches")
        local.set_option("profile", 0)
        tb = torch.tensor([bel], dtype=torch.float64, device=device)
        if dist:
            dist.all_reduce(tb, op=dist.ReduceOp.MAX)
        bel = float(tb.item())
        per_batch_kernel_s = b_ns * 1e-9 / args.batch_steps      # all scan launches of one batch
        flops = 2.0 * bq * (hi - lo) * args.d
        # matrix-pipe counters of this kernel come from separate rocprofv3 --pmc passes (profiles/summarize.py mfma)
        pmc = {}
        ppath = os.path.join(ROOT, "profiles", "mfma_pmc.json")
        if os.path.exists(ppath):
            try:
                pmc = json.load(open(ppath)).get(f"n={hi - lo},d={args.d},{args.dtype},q={bq},dot_product", {})
            except Exception:
                pmc = {}
        # what the matrix pipes of this chip sustain on this loop shape (tools/mfma_ceiling.hip: the same MFMA / ds_read_b128 / LDS-DMA
        # cadence with random operands and nothing else -- no epilogue, no filter, no sample, no sorts), measured once per round
        sustained = {}
        cpath = os.path.join(ROOT, "profiles", "r4_mfma_ceiling.jsonl")
        if os.path.exists(cpath):
            try:
                for line in open(cpath):
                    if line.startswith("{"):
                        j = json.loads(line)
                        sustained[j["variant"].split(":")[0]] = j["pflops"] * 1e3
            except Exception:
                sustained = {}
        ach_tf = flops / per_batch_kernel_s / 1e12 if per_batch_kernel_s else 0.0
        batched = {
            "workload": f"N={args.n} d={args.d} {args.dtype} Q={bq} dot_product top-{args.k}",
            "qps": bq * args.batch_steps / bel, "ms_per_batch": 1e3 * bel / args.batch_steps,
            "scan_launches_per_batch": b_l / args.batch_steps,
            "roofline_mfma": {"bound": "mfma", "achieved": flops / per_batch_kernel_s / 1e12 if per_batch_kernel_s else 0.0,
                              "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                              "frac": flops / per_batch_kernel_s / 1e12 / MFMA_F16_PEAK_TFLOPS if per_batch_kernel_s else 0.0,
                              "sustained_tflops": {"registers_only": sustained.get("regs"), "with_lds_fragment_reads": sustained.get("lds"),
                                                   "with_lds_reads_and_hbm_stream": sustained.get("dma"),
                                                   "source": "profiles/r4_mfma_ceiling.jsonl (tools/mfma_ceiling.hip, random fp16 operands, 2 waves per SIMD, in-kernel clock 1.66 / 1.69 / 1.47 GHz)"},
                              "frac_of_sustained": (ach_tf / sustained["dma"]) if sustained.get("dma") else None,
                              "mfma_busy_frac": pmc.get("mfma_busy_frac"), "clock_ghz": pmc.get("clock_ghz"),
                              "clock_ghz_in_kernel": pmc.get("clock_ghz_in_kernel"), "pmc_source": pmc.get("source")},
            "roofline_hbm": {"bound": "hbm", "achieved": alg_bytes / per_batch_kernel_s / 1e9 if per_batch_kernel_s else 0.0,
                             "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": alg_bytes / per_batch_kernel_s / 1e9 / HBM_PEAK_GBS if per_batch_kernel_s else 0.0},
        }

    # HBM traffic of the dominant kernel comes from separate rocprofv3 --pmc passes (counters cannot be read
    # inside this process); the corrected per-launch figure is committed under profiles/ by profiles/summarize.py
    traffic = args.pmc_traffic
    tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if traffic is None and os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            key = f"n={hi - lo},d={args.d},{args.dtype},q=1,{args.metric}"
            if key in tj:
                traffic = tj[key]["hbm_bytes_per_launch"]
        except Exception:
            traffic = None

    exchange_desc = kind_of(sharded)
    rccl = None
    if args.full and dist and world > 1:
        barrier()
        try:
            rccl = rccl_block(args, dist, rank, world, device, exchange_desc, tdtype, mid)
        except Exception as e:                                   # noqa: BLE001 -- a diagnostics block must not take the line down
            rccl = {"error": repr(e)[:300]}
    exchange_alt = None
    if alt is not None:
        if args.full:
            barrier()
            exchange_alt = {"kind": kind_of(alt), "p50_ms": 1e3 * p50_of(alt, min(args.steps, 50)),
                            "calibration_p50_ms": {k: 1e3 * v for k, v in (calib or {}).items()}}
        alt.close()
    sharded.close()

    # ---------------- the drop-in API on the same matrix (one GPU) ----------------------------------
    api = None
    if args.full and rank == 0 and world == 1:
        import hyperdb.ranking_algorithm as ranking
        from hyperdb import HyperDB
        steps_api = min(args.steps, 200)
        qs = [Q[args.warmup + (i % args.steps)].cpu().numpy() for i in range(steps_api)]      # host float32 queries
        for i in range(5):
            ranking.hyperDB_ranking_algorithm_sort(local, qs[i % steps_api], top_k=args.k, metric=args.metric)
        t_sort = np.empty(steps_api)
        for i in range(steps_api):
            t0 = time.perf_counter()
            ranking.hyperDB_ranking_algorithm_sort(local, qs[i], top_k=args.k, metric=args.metric)
            t_sort[i] = time.perf_counter() - t0
        db = HyperDB(fp_precision="float16" if args.dtype == "fp16" else "float32")
        db._index = local                                 # the resident matrix of this run: documents are their own row numbers
        db.documents = range(hi - lo)
        db.source_indices = range(hi - lo)
        for i in range(5):
            db.query(qs[i % steps_api] + 1e-3, top_k=args.k, metric=args.metric)
        t_query = np.empty(steps_api)
        for i in range(steps_api):
            t0 = time.perf_counter()
            db.query(qs[i], top_k=args.k, metric=args.metric)
            t_query[i] = time.perf_counter() - t0
        # the same with both recency decays (hyperdb.py:1310-1346, :1555): the timestamps of the key are what the facade would
        # extract from the documents once (30 days, seeded); first call = column upload + decay kernel, later calls = cached bias
        db.metadata_keys = ["timestamp"]
        db._ts_cache["timestamp"] = 1.7e9 + np.random.default_rng(7).random(hi - lo) * 30 * 86400.0
        t0 = time.perf_counter()
        db.query(qs[0] + 2e-3, top_k=args.k, metric=args.metric, recency_bias=0.5, timestamp_key="timestamp")
        t_first = time.perf_counter() - t0
        t_rec = np.empty(steps_api)
        for i in range(steps_api):
            t0 = time.perf_counter()
            db.query(qs[i], top_k=args.k, metric=args.metric, recency_bias=0.5, timestamp_key="timestamp")
            t_rec[i] = time.perf_counter() - t0
        host_passes = db.host_row_passes
        db._index = None
        api = {"sort_p50_ms": 1e3 * float(np.median(t_sort)), "query_p50_ms": 1e3 * float(np.median(t_query)),
               "query_recency_p50_ms": 1e3 * float(np.median(t_rec)), "query_recency_first_call_ms": 1e3 * t_first,
               "query_recency_host_row_passes": host_passes,
               "kernel_path_p50_ms": 1e3 * float(np.median(lat)), "queries": "numpy float32 on the host",
               "entry_points": "hyperdb.ranking_algorithm.hyperDB_ranking_algorithm_sort(handle, q, top_k) / HyperDB.query(q, top_k)"}

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, V, Q)

    extras = []
    if args.full and rank == 0 and world == 1 and args.extra:
        local.close()
        del sharded, local, V
        torch.cuda.empty_cache()
        for name in [x for x in args.extra.split(",") if x]:
            extras.append(extra_leg(name, device))

    if rank == 0:
        out = {
            "metric": f"queries/sec, N={args.n // 1_000_000}M d={args.d} {args.dtype} top-{args.k} (single-query stream; p50 latency alongside)",
            "value": qps, "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "p50_latency_ms": 1e3 * float(np.median(lat)),
            "p99_latency_ms": 1e3 * float(np.percentile(lat, 99)),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32" if args.dtype == "fp32" else "f16", "data": "synthetic",
            "config": {"workload": f"N={args.n} d={args.d} {args.dtype} Q=1 {args.metric} top-{args.k}, row-sharded x{world}",
                       "rows_per_gpu": hi - lo, "accumulate": "f32", "exchange": exchange_desc},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "kernel": headline_kernel, "kernel_us": kern_s * 1e6,
                         "algorithmic_bytes_per_launch": alg_bytes, "launches_timed": scan_launches},
            "cpu_baseline": cpu,
            "batched": batched,
            "api": api,
        }
        if exchange_alt is not None:
            out["exchange_alt"] = exchange_alt
        if rccl is not None:
            out["rccl"] = rccl
        if extras:
            out["extra"] = extras
        print(json.dumps(out))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
