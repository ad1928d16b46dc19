"""GPU tests (-m gpu) of MXFP4 rows wider than 512 elements on the bf16 matrix cores (csrc/hdb_mfma_f4_wide.h): the waves of a
workgroup split K and add through LDS, one launch.  Opt-in: set_option("b1_mfma_min_q", n >= 1) together with
set_option("f8_ks_min_q", != 0) on a storage="mxfp4" index.  Reference, band, inputs, N and k as tests/test_mxf4_mfma.py (scale bytes
PER BLOCK: a wave that reads a neighbour slice's scale word is off by a power of two).  Widths: 768 = 3 x 256, 1152 = 3 x 384,
2048 = 4 x 512, 3072 = 8 x 384, 640 = 5 x 128, 2560 = 5 x 512 -- every slice width, three to eight waves."""
import numpy as np
import pytest
from oracle import ranking_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 8192 + 3 * 64 + 5
K = 10
MM_METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "pearson_correlation")
COS = "cosine_similarity"
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


def _wide(ix, b1=5, ks=5):
    ix.set_option("b1_mfma_min_q", b1)
    ix.set_option("f8_ks_min_q", ks)


def _call(ix, Q, metric, mfma, exact=False):
    from hyperdb._native import METRIC_IDS
    gi, gs, st = (t.cpu().numpy() for t in ix.topk_device(Q, K, METRIC_IDS[metric], exact=exact))
    assert ix.stat("mfma") == mfma and ix.stat("fused") in ((0,) if mfma else (0, 3)), (metric, Q.shape, exact)
    return gi, gs, st


@pytest.mark.parametrize("nq", [5, 17, 65])
@pytest.mark.parametrize("d", [768, 1152, 2048, 3072, 640, 2560])
def test_parity(d, nq):
    """Every slice width, 3 / 4 / 5 / 8 waves x a partial query group, two groups, several grid rows: every metric with and without a bias,
    sampled (MODE 0 + MODE 1) and once per width exact; query 0 is stored row N - 2, which the euclidean re-score puts first."""
    ix, _, _, W = _index(d)
    rng = np.random.default_rng(31 * d + nq)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[0] = W[N - 2]
    bias = rng.uniform(-0.05, 0.05, N).astype(np.float32)
    worst = 0.0
    try:
        _wide(ix)
        for b in (None, bias):
            ix.set_bias(b)
            for metric in MM_METRICS:
                for exact in ((False, True) if (nq == 5 and metric == COS) else (False,)):
                    gi, gs, st = _call(ix, Q, metric, 1, exact)
                    assert (st == 0).all(), (metric, exact, st)
                    for qi in (0, (37 * nq) // 65, nq - 1):          # (a lane in the middle of a later query group too: 37 of 65)
                        ref = orc.check_topk(gi[qi], gs[qi], W, Q[qi], metric, K, bias=None if b is None else b.astype(np.float64), tol=TOL)
                        worst = max(worst, float(np.max(np.abs(gs[qi] - ref[gi[qi]]) / np.maximum(1.0, np.abs(ref[gi[qi]])))))
                    if metric == "euclidean_metric":
                        assert gi[0][0] == N - 2 and gs[0][0] == np.float32(1.0) + (0 if b is None else b[N - 2])
        print(f"d {d} nq {nq}: largest error {worst:.3e} of the band {TOL:.0e} * max(1, |s|)")
    finally:
        ix.close()


def test_same_bits_in_every_grid_and_batch():
    """The partial sums are added in slice order whoever adds them: one workgroup, the default grid and the same queries inside a
    65-query batch give a row the same score bits (d = 1280 = 5 x 256: the reducer rotates through five waves)."""
    d = 1280
    ix, _, _, _ = _index(d)
    Q = np.random.default_rng(9).standard_normal((65, d)).astype(np.float32)
    try:
        _wide(ix)
        gi, gs, _ = _call(ix, Q[:16], COS, 1)
        ix.set_option("max_blocks", 1)
        one = _call(ix, Q[:16], COS, 1)
        ix.set_option("max_blocks", 0)
        big = _call(ix, Q, COS, 1)
        assert gi.tobytes() == one[0].tobytes() and gs.tobytes() == one[1].tobytes()
        assert gi.tobytes() == big[0][:16].tobytes() and gs.tobytes() == big[1][:16].tobytes()
    finally:
        ix.close()


def test_what_keeps_the_valu_scan():
    """With both options on: 4 queries, manhattan, hamming, d = 1408, use_mfma = 0 and a matrix with one overflowing block (scale byte 254,
    code 6) in slice 2 stay on the VALU scan, and so does either option alone -- indices, score bits and status with both options off."""
    from hyperdb._native import GpuIndex
    ix, c, s, _ = _index(768)
    odd = _index(1408)[0]
    c2, s2 = c.copy(), s.copy()
    c2[100, 16 * 17:16 * 18], s2[100, 17] = 0x66, 254            # (block 17: elements 544 .. 575, slice 2 of 3)
    inf = GpuIndex((c2, s2), storage="mxfp4")
    rng = np.random.default_rng(3)
    Q, Q1408 = rng.standard_normal((16, 768)).astype(np.float32), rng.standard_normal((16, 1408)).astype(np.float32)
    cases = [(ix, Q[:4], COS, {}, (5, 5)), (ix, Q, "manhattan_distance", {}, (5, 5)), (ix, Q, "hamming_distance", {}, (5, 5)), (odd, Q1408, COS, {}, (5, 5)),
             (ix, Q, COS, {"use_mfma": 0}, (5, 5)), (inf, Q, COS, {}, (5, 5)), (ix, Q, COS, {}, (5, 0)), (ix, Q, COS, {}, (0, 5))]
    try:
        for h, q, metric, opts, on in cases:
            got = []
            for name, value in opts.items():
                h.set_option(name, value)
            for b1, ks in (on, (0, 0)):
                _wide(h, b1, ks)
                got.append(_call(h, q, metric, 0))
            for name in opts:
                h.set_option(name, 1)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*got)), (metric, q.shape, opts, on)      # (indices, score bits, status)
        _wide(ix)
        _call(ix, Q, COS, 1)                              # (the same handle and queries do take the cores once nothing holds them back)
    finally:
        for h in (ix, odd, inf):
            h.close()


def test_the_options_reading():
    d = 1024
    ix = _index(d)[0]
    Q = np.random.default_rng(6).standard_normal((16, d)).astype(np.float32)
    try:
        for b1, ks, reads in ((5, 0, 0), (0, 5, 0), (3, -1, 5), (5, 16, 16)):
            _wide(ix, b1, ks)
            assert ix.stat("b1_mfma_min_q") == reads, (b1, ks)
        _call(ix, Q[:15], COS, 0)
        _call(ix, Q, COS, 1)
    finally:
        ix.close()
