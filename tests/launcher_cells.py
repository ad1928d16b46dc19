"""One shard launcher of the matrix-core scan x {dot, cosine, euclidean} x {no bias, bias}, against the float64 model of
oracle/ranking_oracle.py: the helper behind test_every_*_launcher_metric_and_bias in test_gpu_parity.py (fp16, float32),
test_bf16.py, test_f8.py, test_i8.py and test_b1_mfma.py.  profiles/mfma_launch_coverage.txt lists the launchers and their cases.

The device code of the kernels is pinned elsewhere (tools/device_code_identity.sh); what these cases pin is the WIRING of the launch
layer (csrc/hdb_mfma_kernel.h: hdb_metric_ladder, hdb_mode_ladder; csrc/hdb_common.h: MfmaLaunch): a swapped per-row array (cosine
takes 1/||v||, euclidean ||v||^2), a lost bias flavour, a dropped qscl, a wrong padded or slice width shows only when a shard runs.

Shape: the matrix cores are planned above the candidate capacity of 8192 rows only, so N = 8192 + 3 x 64 + 5 = 8389 rows -- the
smallest matrix that reaches a launcher, plus three of the tallest tiles (64 rows) and five rows: the last tile is ragged at every
tile height (8389 = 5 mod 16, 32 and 64).  k = 10.  Query 0 is a stored row of that last tile (the euclidean re-score acts on it);
queries 0 and nq - 1 are checked (nq - 1 sits in a partial query group at 5, 17 and 129 queries).  A sampled call runs a launcher's
score mode on the row sample and its filter mode on all rows, and the K slices their partial-sum mode before both.
The tolerance is the caller's: the file's own band for its row type."""
import numpy as np

N = 8192 + 3 * 64 + 5
K = 10
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric")


def make_index(kind, d, rng):
    """-> (GpuIndex, the stored values widened exactly to float32 -- float16 for fp16 rows, which the oracle widens itself)."""
    import torch
    from hyperdb._native import GpuIndex
    X = rng.standard_normal((N, d)).astype(np.float32)
    if kind == "f16":
        V = X.astype(np.float16)
        return GpuIndex(V), V
    if kind == "f32":
        return GpuIndex(X), X
    if kind == "bf16":
        t = torch.from_numpy(X).to(torch.bfloat16)
        return GpuIndex(t.cuda()), t.float().numpy()
    if kind == "f8":
        t = torch.from_numpy(X).to(torch.float8_e4m3fn)          # |x| < 6: far from the format's 448, no NaN code
        return GpuIndex(t), t.float().numpy()
    if kind == "i8":
        I = np.clip(np.rint(X * 40.0), -128, 127).astype(np.int8)
        return GpuIndex(I, storage="int8"), I.astype(np.float32)
    if kind == "b1":
        bits = X > 0
        return GpuIndex(np.packbits(bits, axis=1), storage="bits"), bits.astype(np.float32)
    raise ValueError(kind)


def check_launcher_cells(orc, kind, d, nq, options, tol, stats):
    """Six sampled top-k calls on one index; `stats`: statistic -> the value every call must report (mfma = 1 among them), or a dict
    metric -> value where the plan depends on the metric."""
    from hyperdb._native import METRIC_IDS
    rng = np.random.default_rng(100_003 * d + nq)
    ix, Vw = make_index(kind, d, rng)
    try:
        for name, value in options.items():
            ix.set_option(name, value)
        Q = rng.standard_normal((nq, d)).astype(np.float32)
        Q[0] = Vw[N - 2].astype(np.float32)
        bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
        checked = (0, nq - 1)
        for metric in METRICS:
            exact = {qi: orc.exact_scores(Vw, Q[qi], metric) for qi in checked}          # once per metric, shared by both bias cells
            for b in (None, bias):
                ix.set_bias(b)
                idx, sc, st = ix.topk_device(Q, K, METRIC_IDS[metric])
                tag = (kind, d, nq, metric, b is not None)
                want = {name: v[metric] if isinstance(v, dict) else v for name, v in stats.items()}
                got = {name: ix.stat(name) for name in stats}
                assert got == want, (tag, got)
                assert int(st.abs().sum().item()) == 0, tag
                idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
                for qi in checked:
                    ref = exact[qi] if b is None else exact[qi] + b.astype(np.float64)
                    err = np.abs(sc[qi].astype(np.float64) - ref[idx[qi]]) / np.maximum(1.0, np.abs(ref[idx[qi]]))
                    print(f"{tag} query {qi}: largest score error {err.max():.3e} of the band {tol:g}")
                    orc.check_topk(idx[qi], sc[qi], Vw, Q[qi], metric, K, bias=None if b is None else b.astype(np.float64), tol=tol, exact=ref)
                if metric == "euclidean_metric" and b is None:
                    assert idx[0][0] == N - 2, tag                                      # the stored row finds itself
    finally:
        ix.close()
