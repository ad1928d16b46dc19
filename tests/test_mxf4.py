"""GPU tests (-m gpu) of MXFP4 storage (storage="mxfp4", HDB_MXF4 = 13, hdb_f4scan.hip).  Reference: oracle/ranking_oracle.py, plain
float64 numpy, on mxfp4_to_float(codes, scales).  Band: 1e-5 * max(1, |s|) on every returned row, hamming exact (the float32 band once
a float32 bias is added to an integer of up to d), jaccard 1e-6; index sets equal modulo ties inside the band (check_topk).  Inputs:
codes uniform over all 16 values, scale bytes uniform in [121, 127] (a float32 sum stays 9x inside the band), unit-norm Gaussian queries.
d: 32 the scale sits in the second chunk, 384 idle lanes, 512 a 17th chunk, 544 a ragged second step, 1024 two register steps, 2080 LDS."""
import numpy as np
import pytest
from oracle import ranking_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "hamming_distance", "manhattan_distance",
           "jaccard_similarity", "pearson_correlation")
SHAPES = [(d, n) for d in (32, 384, 512, 544, 1024, 2080) for n in (1003, 5003, 70001)]
_DATA = {}


def _data(d, n):
    """(codes, scales, the float32 widening, six unit-norm queries) of a shape: made once (one shape kept), never modified."""
    if (d, n) not in _DATA:
        from hyperdb._native import mxfp4_to_float
        _DATA.clear()
        rng = np.random.default_rng(1000 * d + n)
        c = rng.integers(0, 256, size=(n, d // 2), dtype=np.uint8)
        s = rng.integers(121, 128, size=(n, d // 32), dtype=np.uint8)
        Q = rng.standard_normal((6, d))
        _DATA[(d, n)] = (c, s, mxfp4_to_float(c, s), (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32))
    return _DATA[(d, n)]


def _check(idx, sc, exact, k, tol):      # check_topk against a precomputed float64 score vector (bias and mask already in it)
    orc.check_topk(idx, sc, np.zeros((exact.shape[0], 1), dtype=np.float32), None, "dot_product", k, tol=tol, exact=exact)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _topk(ix, Q, k, mid, exact=False):
    if exact:                                 # hdb_topk_exact
        gi, gs, st = (t.cpu().numpy() for t in ix.topk_device(Q, k, mid, exact=True))
        assert (st == 0).all(), st
    else:                                     # the host call, which re-runs a query whose sampled threshold missed
        gi, gs = ix.topk(Q, k, mid)
    assert ix.stat("mfma") == ix.stat("quant") == ix.stat("subset") == 0 and ix.stat("fused") in (0, 3)
    return gi, gs


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n", SHAPES)
def test_parity(d, n, metric):
    """One-query calls inside the band; 2, 4 and 6 queries per call and hdb_topk_exact return their bits; again with bias and mask."""
    from hyperdb._native import GpuIndex, HDB_MXF4, METRIC_IDS, mxfp4_pitch
    c, s, W, Q = _data(d, n)
    mid, k = METRIC_IDS[metric], 100
    ref = [orc.exact_scores(W, Q[qi], metric) for qi in range(6)]
    rng = np.random.default_rng(11)
    bias = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    ix = GpuIndex((c, s), storage="mxfp4")
    assert ix.dtype == HDB_MXF4 and (ix.n, ix.d) == (n, d) and tuple(ix.V.shape) == (n, mxfp4_pitch(d)) and not ix.has_nan
    for biased in (False, True):
        if biased:
            ix.set_bias(bias)
            ix.set_row_mask(mask)
            ref = [np.where(mask != 0, r + bias.astype(np.float64), -np.inf) for r in ref]
        tol = (TOL if biased else 0.0) if metric == "hamming_distance" else 1e-6 if metric == "jaccard_similarity" else TOL
        one = [_topk(ix, Q[qi:qi + 1], k, mid) for qi in range(6)]
        for qi in range(6):
            _check(one[qi][0][0], one[qi][1][0], ref[qi], k, tol)
        for nq, exact in ((2, False), (4, False), (6, False), (4, True)):
            gi, gs = _topk(ix, Q[:nq], k, mid, exact=exact)
            for qi in range(nq):
                assert _same((gi[qi], gs[qi]), (one[qi][0][0], one[qi][1][0])), (biased, nq, exact, qi)
    if (d, n, metric) == (384, 70001, "cosine_similarity"):      # k > 2048 once: the full sort (bias and mask still set)
        gi, gs = _topk(ix, Q[:2], 3000, mid)
        for qi in range(2):
            _check(gi[qi], gs[qi], ref[qi], 3000, TOL)
    ix.close()


def test_lifecycle_append_update_compact():
    """After each step the index answers as a fresh one over the resulting pairs, bit for bit; a refused append stores nothing."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    c, s, _, Q = _data(384, 5003)

    def same_as_fresh(ix, cc, ss):
        hc, hs = ix.host_mxfp4()
        assert ix.n == len(cc) and np.array_equal(hc, cc) and np.array_equal(hs, ss)
        fresh = GpuIndex((cc, ss), storage="mxfp4")
        for metric in ("cosine_similarity", "pearson_correlation", "hamming_distance", "manhattan_distance"):
            assert _same(_topk(ix, Q[:3], 50, METRIC_IDS[metric]), _topk(fresh, Q[:3], 50, METRIC_IDS[metric])), metric
        fresh.close()

    ix = GpuIndex((c[:3000], s[:3000]), storage="mxfp4")
    _topk(ix, Q[:1], 50, METRIC_IDS["hamming_distance"])            # (the lazy caches exist before the matrix grows)
    ix.append((c[3000:4500], s[3000:4500]))
    same_as_fresh(ix, c[:4500], s[:4500])
    with pytest.raises(ValueError, match="to_mxfp4"):
        ix.append(np.zeros((3, 384), dtype=np.float32))
    assert ix.n == 4500
    ix.update((c[1000:], s[1000:]))
    same_as_fresh(ix, c[1000:], s[1000:])
    keep = np.arange(0, 4003, 3)
    ix.compact(keep)
    same_as_fresh(ix, c[1000:][keep], s[1000:][keep])
    ix.close()


def test_nan_block_raises():
    import hyperdb.ranking_algorithm as ranking
    c, s, _, Q = _data(384, 1003)
    s = s.copy()
    s[777, 5] = 255
    h = ranking.register_vectors((c, s), storage="mxfp4")
    assert h.index.has_nan and h.shape == (1003, 384)
    with pytest.raises(ValueError, match="NaN"):
        ranking.hyperDB_ranking_algorithm_sort(h, Q[0], top_k=5, metric="cosine_similarity")
    h.close()


def test_two_stage_onto_fp16():
    """Onto an fp16 index over the widened values (exact in fp16), generous k1: that index's own top-k, the VALU scan's bits."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    c, s, W, Q = _data(384, 70001)
    mid = METRIC_IDS["cosine_similarity"]
    first, second = GpuIndex((c, s), storage="mxfp4"), GpuIndex(W.astype(np.float16))
    assert np.array_equal(second.host_matrix().astype(np.float32), W)
    gi, gs = second.two_stage(first, Q[:4], mid, 1000, Q[:4], mid, 20)
    for name in ("use_mfma", "use_fused", "use_quant", "use_l1_tile"):
        second.set_option(name, 0)
    assert _same((gi, gs), _topk(second, Q[:4], 20, mid, exact=True))
    first.close()
    second.close()
