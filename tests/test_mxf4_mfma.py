"""GPU tests (-m gpu) of MXFP4 batches on the bf16 matrix cores (csrc/hdb_mfma_f4.h), the opt-in set_option("b1_mfma_min_q", n) on a
storage="mxfp4" index.  Reference: oracle/ranking_oracle.py, plain float64 numpy, on mxfp4_to_float(codes, scales); band: the
project's 1e-5 * max(1, |s|).  Inputs as tests/test_mxf4.py: codes uniform over all 16 values, scale bytes uniform in [121, 127] PER
BLOCK (a lane that picks a neighbour's scale byte is off by a power of two), Gaussian queries.
N = 8192 + 3 * 64 + 5 rows: the smallest matrix the plan sends to the matrix cores, with a ragged last tile; k = 10."""
import numpy as np
import pytest
from oracle import ranking_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 8192 + 3 * 64 + 5
K = 10
MM_METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "pearson_correlation")
_MADE = {}


def _index(d, n=N):
    """(a fresh index, codes, scales, the float32 widening) of a shape; the arrays are made once and never modified."""
    from hyperdb._native import GpuIndex, mxfp4_to_float
    if (d, n) not in _MADE:
        rng = np.random.default_rng(1000 * d + n)
        c = rng.integers(0, 256, size=(n, d // 2), dtype=np.uint8)
        s = rng.integers(121, 128, size=(n, d // 32), dtype=np.uint8)
        _MADE[(d, n)] = (c, s, mxfp4_to_float(c, s))
    c, s, W = _MADE[(d, n)]
    return GpuIndex((c, s), storage="mxfp4"), c, s, W


def _call(ix, Q, metric, mfma, exact=False):
    from hyperdb._native import METRIC_IDS
    gi, gs, st = (t.cpu().numpy() for t in ix.topk_device(Q, K, METRIC_IDS[metric], exact=exact))
    assert ix.stat("mfma") == mfma and ix.stat("fused") in ((0,) if mfma else (0, 3)), (metric, Q.shape, exact)
    return gi, gs, st


@pytest.mark.parametrize("nq", [5, 17, 65])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_parity(d, nq):
    """One to four block loads per lane x a partial query group, two groups per workgroup, two grid rows: every metric with and without
    a bias, sampled (MODE 0 + MODE 1) and once per width exact; query 0 is stored row N - 2, which the euclidean re-score puts first."""
    ix, _, _, W = _index(d)
    rng = np.random.default_rng(31 * d + nq)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[0] = W[N - 2]
    bias = rng.uniform(-0.05, 0.05, N).astype(np.float32)
    worst = 0.0
    try:
        ix.set_option("b1_mfma_min_q", 5)
        for b in (None, bias):
            ix.set_bias(b)
            for metric in MM_METRICS:
                for exact in ((False, True) if (nq == 5 and metric == "cosine_similarity") else (False,)):
                    gi, gs, st = _call(ix, Q, metric, 1, exact)
                    assert (st == 0).all(), (metric, exact, st)
                    for qi in (0, nq - 1):
                        ref = orc.check_topk(gi[qi], gs[qi], W, Q[qi], metric, K, bias=None if b is None else b.astype(np.float64), tol=TOL)
                        worst = max(worst, float(np.max(np.abs(gs[qi] - ref[gi[qi]]) / np.maximum(1.0, np.abs(ref[gi[qi]])))))
                    if metric == "euclidean_metric":
                        assert gi[0][0] == N - 2 and gs[0][0] == np.float32(1.0) + (0 if b is None else b[N - 2])
        print(f"d {d} nq {nq}: largest error {worst:.3e} of the band {TOL:.0e} * max(1, |s|)")
    finally:
        ix.close()


def test_what_keeps_the_valu_scan():
    """With the option at 5: 4 queries, manhattan and the bit metrics, d = 544, use_mfma = 0 and a matrix with one overflowing block
    (scale byte 254, code 6) stay on the VALU scan -- indices, score bits and status of the same call with the option at 0."""
    from hyperdb._native import GpuIndex
    ix, c, s, _ = _index(384)
    odd = _index(544)[0]
    c2, s2 = c.copy(), s.copy()
    c2[100, 48:64], s2[100, 3] = 0x66, 254
    inf = GpuIndex((c2, s2), storage="mxfp4")
    rng = np.random.default_rng(3)
    Q, Q544 = rng.standard_normal((16, 384)).astype(np.float32), rng.standard_normal((16, 544)).astype(np.float32)
    cos = "cosine_similarity"
    cases = [(ix, Q[:4], cos, {}), (ix, Q[:4], "euclidean_metric", {}), (ix, Q, "manhattan_distance", {}), (ix, Q, "hamming_distance", {}),
             (ix, Q, "jaccard_similarity", {}), (odd, Q544, cos, {}), (ix, Q, cos, {"use_mfma": 0}), (inf, Q, cos, {}), (inf, Q, "dot_product", {})]
    try:
        for h, q, metric, opts in cases:
            got = []
            for name, value in opts.items():
                h.set_option(name, value)
            for option in (5, 0):
                h.set_option("b1_mfma_min_q", option)
                got.append(_call(h, q, metric, 0))
            for name in opts:
                h.set_option(name, 1)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*got)), (metric, q.shape, opts)      # (indices, score bits, status)
        ix.set_option("b1_mfma_min_q", 5)
        _call(ix, Q, cos, 1)                              # (the same handle and queries do take the cores once nothing holds them back)
    finally:
        for h in (ix, odd, inf):
            h.close()


def test_the_options_reading():
    ix, odd = _index(256)[0], _index(544)[0]
    Q = np.random.default_rng(6).standard_normal((16, 256)).astype(np.float32)
    try:
        assert ix.stat("b1_mfma_min_q") == 0
        _call(ix, Q, "cosine_similarity", 0)
        for value, reads in ((3, 5), (-1, 0), (16, 16)):
            ix.set_option("b1_mfma_min_q", value)
            odd.set_option("b1_mfma_min_q", value)
            assert ix.stat("b1_mfma_min_q") == reads and odd.stat("b1_mfma_min_q") == 0, value
        _call(ix, Q[:15], "cosine_similarity", 0)
        _call(ix, Q, "cosine_similarity", 1)
    finally:
        ix.close()
        odd.close()
