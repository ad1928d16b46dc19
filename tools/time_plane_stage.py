"""The plane pass with stage A (use_plane = 3) against the one-stage pass (use_plane = 2) on one handle.

One fp16 index with its automatic shadow per size; one cosine query, top-100; the two settings alternate call by call at every grid
asked for (plane_wg_per_cu, 0: each pass's own default), p50 of a call in us (host clock around a call that ends in a synchronise).
The first line of a size gives plane_survivors and quant_cands of both settings, the status words, and whether indices and score
bits agree -- compared only where both status words are zero (a list that overflowed HDB_CAND_CAP leaves a failed attempt's partial
device list, which the host entry discards for the exact re-run; `overflow` marks such a size, whose timings include that path).

  python tools/time_plane_stage.py --rows 2000000 5000000 10000000 --wg 3 5 6 --d 384
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
import hyperdb.ranking_algorithm as ranking
from hyperdb._native import METRIC_IDS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2_000_000, 5_000_000, 10_000_000])
    ap.add_argument("--wg", type=int, nargs="+", default=[0])
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--reps", type=int, default=60)
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(1)
    d = args.d
    for n in args.rows:
        V = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        h = ranking.register_vectors(V)
        ix = h.index
        Q = np.random.default_rng(n).standard_normal((1, d)).astype(np.float32)
        ix.set_option("plane_min_n", 0)
        ix.set_option("quant_min_n", 0)

        def call():
            out = ix.topk_device(Q, 100, METRIC_IDS["cosine_similarity"])
            torch.cuda.synchronize()
            return out

        res = {}
        for up in (3, 2):
            ix.set_option("use_plane", up)
            o = call()
            res[up] = (o[0].cpu().numpy(), o[1].cpu().numpy(), int(o[2].cpu().numpy()[0]), ix.stat("plane"), ix.stat("plane_survivors"),
                       ix.stat("quant_cands"))
        a, b = res[3], res[2]
        if a[2] == 0 and b[2] == 0:
            same = str(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)))
        else:
            same = "overflow" if a[2] == b[2] else "STATUS DIFFERS"
        print(f"n={n} d={d} plane {a[3]} {b[3]} survivors {a[4]} / {b[4]} cands {a[5]} / {b[5]} status {a[2]} / {b[2]} same {same}", flush=True)
        for wg in args.wg:
            ix.set_option("plane_wg_per_cu", wg)
            t = {3: [], 2: []}
            for it in range(args.reps + 5):
                for up in (3, 2):
                    ix.set_option("use_plane", up)
                    t0 = time.perf_counter(); call(); dt = time.perf_counter() - t0
                    if it >= 5:
                        t[up].append(dt)
            p1, p2 = np.median(t[3]) * 1e6, np.median(t[2]) * 1e6
            print(f"  wg_per_cu {wg}: stage A {p1:8.1f} us   one stage {p2:8.1f} us   ratio {p1 / p2:.3f}", flush=True)
        h.close()
        del V, h, ix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
