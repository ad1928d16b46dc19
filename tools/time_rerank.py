"""Rerank (hdb_rerank) and two-stage search (hdb_two_stage_host): call latency on one MI355X, cosine top-100.

One set of Gaussian embeddings (--rows x --dim float32, generated on the device from a seed, never kept whole) is stored three ways:
storage="bits" (x > 0), storage="int8" (round(40 x), clipped to +-127) and float16.  The exact float32 top-100 of every query is
taken while the embeddings are generated; recall@100 is read against it.  Recall is a property of the data: printed, never asserted.

(a) Rerank alone, on the int8 and the fp16 index, nq x m.  Candidates: m random rows per query.  (r), (r') GpuIndex.rerank, two turns
    per round -- the difference of their medians is the spread the other column is read against.  (y) the only way to do this
    before hdb_rerank: a per-query loop of set_row_subset + topk on the same handle.  Beside each time the algorithmic bytes
    nq x m x (row_bytes + 8) and the rate they imply.  The expectation to compare with is the row-list scan's own gather:
    156 k rows x 768 B in a 69 us call, about 35 us of it fixed (README, "Filters").
(b) Two-stage: bits index in front of the int8 index, oversample x nq.  (t), (t') rank_two_stage with a hamming first stage on
    packed queries, two turns per round; (c) the same with a cosine first stage on the float queries; (i) the int8 index alone and
    (f) the fp16 index alone, rank_batch at their defaults.  recall@100 against the exact float32 ranking beside every contender.

p50 over --calls synchronous calls (host queries and candidates in, host results out) after --warmup calls; the contenders alternate
call by call.  The loop (y) costs nq host round trips per call: from --loop-max-q queries on it is timed over --loop-calls calls.
A cell counts as a win only when it is ahead by more than the repeated contender's spread.

    python tools/time_rerank.py [--rows 10000000] [--dim 384] [--calls 60] [--warmup 5] --out profiles/rerank_time.txt
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

CHUNK = 500_000
K = 100


def build(n, d, Q, dev):
    """-> (packed bits uint8 [n, d/8] little order, int8 [n, d], float16 [n, d], exact float32 cosine top-K ids [nq, K]) on the device."""
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    bits = torch.empty((n, d // 8), dtype=torch.uint8, device=dev)
    i8 = torch.empty((n, d), dtype=torch.int8, device=dev)
    f16 = torch.empty((n, d), dtype=torch.float16, device=dev)
    Qn = torch.from_numpy(Q / np.linalg.norm(Q, axis=1, keepdims=True)).to(dev)
    best_s = torch.full((Q.shape[0], K), -float("inf"), device=dev)
    best_i = torch.full((Q.shape[0], K), -1, dtype=torch.int64, device=dev)
    w = (1 << torch.arange(8, device=dev, dtype=torch.int32))
    for r0 in range(0, n, CHUNK):
        m = min(CHUNK, n - r0)
        x = torch.randn((m, d), generator=g, device=dev, dtype=torch.float32)
        bits[r0:r0 + m] = ((x > 0).to(torch.int32).reshape(m, d // 8, 8) * w).sum(-1).to(torch.uint8)
        i8[r0:r0 + m] = torch.clamp(torch.round(x * 40), -127, 127).to(torch.int8)
        f16[r0:r0 + m] = x.to(torch.float16)
        s = Qn @ (x / x.norm(dim=1, keepdim=True)).T
        ks, ki = torch.topk(s, min(K, m), dim=1)
        cs, ci = torch.cat([best_s, ks], 1), torch.cat([best_i, ki + r0], 1)
        best_s, o = torch.topk(cs, K, dim=1)
        best_i = torch.gather(ci, 1, o)
        del x, s
    return bits, i8, f16, best_i.cpu().numpy()


def recall(idx, truth):
    return float(np.mean([len(np.intersect1d(idx[q], truth[q])) / truth.shape[1] for q in range(truth.shape[0])]))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


def rounds(contenders, calls, warmup):
    """contenders: list of (callable, calls or None).  They alternate call by call; -> (p50 us per contender, last results)."""
    for fn, _ in contenders:
        for _ in range(warmup):
            fn()
    t = [[] for _ in contenders]
    last = [None] * len(contenders)
    for c in range(calls):
        for i, (fn, own) in enumerate(contenders):
            if own is not None and c >= own:
                continue
            us, last[i] = timed(fn)
            t[i].append(us)
    return [float(np.median(x)) for x in t], last


def rerank_alone(a, lines, ix, name, row_bytes, Q, rng):
    from hyperdb._native import METRIC_IDS
    cos = METRIC_IDS["cosine_similarity"]
    n = ix.n
    for nq in a.queries:
        for m in a.lists:
            cand = np.stack([rng.choice(n, size=m, replace=False) for _ in range(nq)]).astype(np.int64)
            Qq = Q[:nq]

            def loop():
                out = []
                for q in range(nq):
                    rows = np.sort(cand[q])
                    mask = np.zeros(n, np.uint8)
                    mask[rows] = 1
                    ix.set_row_subset(mask, rows)
                    out.append(ix.topk(Qq[q:q + 1], K, cos)[0])
                ix.set_row_mask(None)
                return np.concatenate(out)

            rr = lambda: ix.rerank(Qq, cand, K, cos)[0]
            own = a.loop_calls if nq >= a.loop_max_q else None
            (pr, py, pr2), (ri, yi, _) = rounds([(rr, None), (loop, own), (rr, None)], a.calls, a.warmup if own is None else 1)
            same = bool(np.array_equal(np.sort(ri, 1), np.sort(yi, 1)))
            nbytes = nq * m * (row_bytes + 8)
            spread = abs(pr - pr2) / pr
            verdict = "win" if py > pr * (1 + spread) else "LOSS" if pr > py * (1 + spread) else "tie"
            lines.append(f"  {name:>5} {nq:>7} {m:>6} {pr:>10.1f} {pr2:>10.1f} {spread:>7.3f} {py:>12.1f} {py / pr:>8.2f} {nbytes / 1e6:>9.2f} {nbytes / pr / 1e3:>8.2f} {verdict:>5} {'yes' if same else 'NO':>5}"
                         + (f"   (loop: {own} calls)" if own is not None else ""))
            print(lines[-1], flush=True)


def two_stage(a, lines, first, second, f16, Q, truth):
    import hyperdb.ranking_algorithm as ranking
    Qp = np.packbits(Q > 0, axis=1, bitorder="little")
    for nq in a.queries:
        Qq, Pq, tq = Q[:nq], Qp[:nq], truth[:nq]
        base = None
        for ov in a.oversample:
            th = lambda: ranking.rank_two_stage(first, second, Qq, top_k=K, oversample=ov, metric="cosine_similarity",
                                                first_metric="hamming_distance", first_queries=Pq)[0]
            tc = lambda: ranking.rank_two_stage(first, second, Qq, top_k=K, oversample=ov, metric="cosine_similarity")[0]
            cont = [(th, None), (tc, None)]
            if base is None:             # the single indexes do not depend on the oversampling: timed once per query count
                cont += [(lambda: ranking.rank_batch(second, Qq, top_k=K, metric="cosine_similarity")[0], None),
                         (lambda: ranking.rank_batch(f16, Qq, top_k=K, metric="cosine_similarity")[0], None)]
            cont.append((th, None))
            p, last = rounds(cont, a.calls, a.warmup)
            if base is None:
                base = (p[2], recall(last[2], tq), p[3], recall(last[3], tq))
            pt, pt2 = p[0], p[-1]
            spread = abs(pt - pt2) / pt
            pi, ri, pf, rf = base
            mark = lambda other: "win" if other > pt * (1 + spread) else "LOSS" if pt > other * (1 + spread) else "tie"
            lines.append(f"  {nq:>7} {ov:>4} {K * ov:>6} {pt:>10.1f} {pt2:>10.1f} {spread:>7.3f} {recall(last[0], tq):>7.4f} {p[1]:>10.1f} {recall(last[1], tq):>7.4f} "
                         f"{pi:>10.1f} {ri:>7.4f} {pf:>10.1f} {rf:>7.4f} {mark(pi):>6} {mark(pf):>6}")
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--lists", type=int, nargs="+", default=[100, 400, 1000, 4000])
    ap.add_argument("--oversample", type=int, nargs="+", default=[2, 4, 10])
    ap.add_argument("--loop-max-q", type=int, default=16, help="from this many queries on the per-query loop is timed over --loop-calls calls")
    ap.add_argument("--loop-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_rerank.py measures on the GPU"
    assert a.calls >= 50, "p50 over at least 50 calls"
    import hyperdb.ranking_algorithm as ranking
    dev = torch.device("cuda", 0)
    n, d = a.rows, a.dim
    Q = np.random.default_rng(7).standard_normal((max(a.queries), d)).astype(np.float32)
    bits, i8, f16, truth = build(n, d, Q, dev)
    first = ranking.register_vectors(bits, storage="bits", bitorder="little")
    second = ranking.register_vectors(i8, storage="int8")
    half = ranking.register_vectors(f16)
    lines = [f"# tools/time_rerank.py: cosine top-{K}, p50 of {a.calls} calls in us (host queries and candidates in, host results out), {a.warmup} warm-up calls, "
             f"the contenders alternate call by call; {n} x {d} Gaussian embeddings",
             f"# {torch.cuda.get_device_name(0)}",
             "# (a) rerank alone.  (r), (r') GpuIndex.rerank, two turns per round (spread = |r - r'| / r)   (y) per-query loop of set_row_subset + topk on the same handle",
             "#     MB = nq x m x (row_bytes + 8) algorithmic bytes, GB/s = MB / (r); verdict: (r) against (y), beyond the spread; same = both return the same rows",
             f"# {'index':>5} {'queries':>7} {'m':>6} {'(r) us':>10} {'(r) again':>10} {'spread':>7} {'(y) loop us':>12} {'(y)/(r)':>8} {'MB':>9} {'GB/s':>8} {'':>5} {'same':>5}"]
    rng = np.random.default_rng(11)
    rerank_alone(a, lines, second.index, "int8", d, Q, rng)
    rerank_alone(a, lines, half.index, "fp16", 2 * d, Q, rng)
    lines += ["# (b) two-stage: bits index (its defaults) in front of the int8 index.  (t), (t') rank_two_stage, hamming first stage on packed queries, two turns per round;",
              "#     (c) rank_two_stage, cosine first stage on the float queries; (i) int8 index alone; (f) fp16 index alone (rank_batch, defaults).  rec = recall@100 against",
              "#     the exact float32 ranking (a property of the data).  verdicts: (t) against (i) and against (f), beyond the spread",
              f"# {'queries':>7} {'over':>4} {'k1':>6} {'(t) us':>10} {'(t) again':>10} {'spread':>7} {'rec':>7} {'(c) us':>10} {'rec':>7} {'(i) us':>10} {'rec':>7} {'(f) us':>10} {'rec':>7} {'vs i8':>6} {'vs f16':>6}"]
    two_stage(a, lines, first, second, half, Q, truth)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
