"""GPU tests (-m gpu) of the bfloat16 storage dtype (HDB_BF16): a torch.bfloat16 matrix stays 2 bytes per element on the device,
the VALU scans serve every metric on it, batches of 5+ dot / cosine / euclidean / pearson queries run on the bf16 matrix cores
(hdb_mfma_bf16.hip) with the float32 queries split into three exact bf16 parts.

Reference: oracle/ranking_oracle.py on the exactly widened float32 matrix.  A bf16 value IS a float32 value and every path
computes in float32 on it, so the tolerance is the project's float32 contract, 1e-5 applied as tol * max(1, |s|)
(tolerance_for); hamming is bit-exact, jaccard (a ratio of two integers <= d evaluated in float32) 1e-6.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "hamming_distance", "manhattan_distance",
           "jaccard_similarity", "pearson_correlation")
N = 20_003                                             # 8 workgroups x many tiles, ragged last tile for every tile height


@pytest.fixture(scope="module")
def orc():
    from oracle import ranking_oracle
    return ranking_oracle


@pytest.fixture(scope="module")
def ranking():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import hyperdb.ranking_algorithm as r
    return r


def _tol(metric):
    return 0.0 if metric == "hamming_distance" else 1e-6 if metric == "jaccard_similarity" else TOL


def _bf16(a32):
    """float32 array -> (bf16 CUDA tensor, its exact float32 widening on the host)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.bfloat16)
    return t.cuda(), t.float().numpy()


_MATS = {}


def _matrix(d, seed=0):
    """One (bf16 device tensor, widened host matrix) per width, shared by the tests and never modified."""
    key = (d, seed)
    if key not in _MATS:
        rng = np.random.default_rng(1000 * d + seed)
        _MATS[key] = _bf16(rng.standard_normal((N, d)).astype(np.float32))
    return _MATS[key]


# ------------------------------------------------------------------------------------------------
# 1. storage
# ------------------------------------------------------------------------------------------------
def test_storage_is_two_bytes_per_element():
    import torch
    from hyperdb._native import GpuIndex, HDB_BF16
    Vb, Vw = _matrix(100)
    ix = GpuIndex(Vb)
    try:
        assert ix.dtype == HDB_BF16 == 3
        assert ix.V.dtype == torch.bfloat16 and ix.V.element_size() * ix.n * ix.d == N * 100 * 2
        host = ix.host_matrix()
        assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), Vw.view(np.uint32))
        assert not ix.has_nan
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 2. VALU paths: every metric, 16-byte rows (d = 384, 100 -> 768 / 200 bytes) and the generic scan (d = 7 -> 14 bytes)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [384, 100, 7])
def test_valu_scans_all_metrics(ranking, orc, d):
    Vb, Vw = _matrix(d)
    rng = np.random.default_rng(d)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    Q[1] = Vw[N - 2] + 0.05 * rng.standard_normal(d).astype(np.float32)
    k = 20
    h = ranking.register_vectors(Vb)
    try:
        h.index.set_option("max_blocks", 8)
        for metric in METRICS:
            tol = _tol(metric)
            oracle = [orc.rank(Vw, Q[qi].copy(), top_k=k, metric=metric) for qi in range(3)]
            idx, sc = ranking.hyperDB_ranking_algorithm_sort(h, Q[0].copy(), top_k=k, metric=metric)
            assert h.index.stat("mfma") == 0
            orc.check_topk(idx, sc, Vw, Q[0], metric, k, tol=tol)
            assert orc.same_result_modulo_ties(idx, sc, oracle[0][0], oracle[0][1], tol), metric
            bi, bs = ranking.rank_batch(h, Q.copy(), top_k=k, metric=metric)
            assert h.index.stat("mfma") == 0
            for qi in range(3):
                orc.check_topk(bi[qi], bs[qi], Vw, Q[qi], metric, k, tol=tol)
                assert orc.same_result_modulo_ties(bi[qi], bs[qi], oracle[qi][0], oracle[qi][1], tol), (metric, qi)
            # the per-metric function: all N scores
            got = getattr(ranking, metric)(h, Q[1].copy()).astype(np.float64)
            want = orc.exact_scores(Vw, Q[1], metric)
            assert got.shape == (N,)
            if metric == "hamming_distance":
                assert np.array_equal(got, want)
            else:
                err = np.abs(got - want)
                print(f"d={d} {metric}: largest score error {err.max():.3e}")
                assert np.all(err <= tol * np.maximum(1.0, np.abs(want))), (metric, err.max())
        dist = ranking.euclidean_metric(h, Q[1].copy(), get_similarity_score=False).astype(np.float64)
        want = np.sqrt(((Vw.astype(np.float64) - Q[1].astype(np.float64)) ** 2).sum(axis=1))
        assert np.all(np.abs(dist - want) <= TOL * np.maximum(1.0, want))
    finally:
        h.close()


@pytest.mark.parametrize("n", [1, 300])
def test_small_path(ranking, orc, n):
    Vb, Vw = _matrix(100)
    q = np.random.default_rng(n).standard_normal(100).astype(np.float32)
    h = ranking.register_vectors(Vb[:n].clone())
    try:
        for metric in METRICS:
            idx, sc = ranking.hyperDB_ranking_algorithm_sort(h, q.copy(), top_k=10, metric=metric)
            oi, osc = orc.rank(Vw[:n], q.copy(), top_k=10, metric=metric)
            if n == 1:                                   # the reference's single-row return: (array([0]), array([scores]))
                got, want = float(np.ravel(sc)[0]), float(np.ravel(osc)[0])
                assert list(idx) == [0] and abs(got - want) <= _tol(metric) * max(1.0, abs(want)), metric
            else:
                assert h.index.stat("path") == 0 and h.index.stat("mfma") == 0
                orc.check_topk(idx, sc, Vw[:n], q, metric, 10, tol=_tol(metric))
                assert orc.same_result_modulo_ties(idx, sc, oi, osc, _tol(metric)), metric
    finally:
        h.close()


def test_exact_path_full_sort_mask_and_recency(orc):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 100
    Vb, Vw = _matrix(d)
    rng = np.random.default_rng(77)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    ix = GpuIndex(Vb)
    try:
        ix.set_option("max_blocks", 8)
        mid = METRIC_IDS["cosine_similarity"]
        # the exact selection against the sampled one
        si, ss, st = ix.topk_device(Q, 20, mid)
        ei, es, est = ix.topk_device(Q, 20, mid, exact=True)
        assert ix.stat("path") == 2 and ix.stat("mfma") == 0 and int(st.abs().sum().item()) == 0 and int(est.abs().sum().item()) == 0
        assert torch.equal(si, ei) and torch.equal(ss, es)
        # k > HDB_MAX_K: all scores + the full sort
        k = 9_000
        fi, fs = ix.topk(Q[:1], k, METRIC_IDS["euclidean_metric"])
        assert ix.stat("path") == 3
        orc.check_topk(fi[0], fs[0], Vw, Q[0], "euclidean_metric", k, tol=TOL)
        # a row mask that keeps 2 % of the rows
        mask = (rng.random(N) < 0.02).astype(np.uint8)
        mask[:3] = 1
        ix.set_row_mask(mask)
        mi, ms = ix.topk(Q, 20, METRIC_IDS["dot_product"])
        ix.set_row_mask(None)
        kept = np.flatnonzero(mask)
        for qi in range(3):
            assert mask[mi[qi]].all()
            orc.check_topk(np.searchsorted(kept, mi[qi]), ms[qi], Vw[kept], Q[qi], "dot_product", 20, tol=TOL)
        # a recency bias
        ts = 1.7e9 + rng.uniform(0, 30 * 86400.0, size=N)
        ix.set_recency(ts, 0.5)
        ri, rs = ix.topk(Q, 20, mid)
        ix.set_bias(None)
        b = 0.5 * np.exp(ts - ts.max())
        for qi in range(3):
            orc.check_topk(ri[qi], rs[qi], Vw, Q[qi], "cosine_similarity", 20, bias=b, tol=TOL)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 3. matrix-core batches (5+ queries, d = 128 / 256 / 384 / 512)
# ------------------------------------------------------------------------------------------------
_CASES = {}


def _mfma_case(d, dot):
    """Matrix with the special rows of the float32 bf16-parts test, as bf16: one row scaled by 1e-3 and -- not for the dot
    product, where a score against such a row cancels to 1e-2 of |v||q| and float32 itself is no better than 1e-5 of THAT
    score -- one by 3e3."""
    key = (d, dot)
    if key not in _CASES:
        rng = np.random.default_rng(977 * d)
        V32 = rng.standard_normal((N, d)).astype(np.float32)
        V32[1234] *= 1.0e-3
        if not dot:
            V32[4321] *= 3.0e3
        Vb, Vw = _bf16(V32)
        Q = rng.standard_normal((130, d)).astype(np.float32)
        Q[0] = Vw[N - 2]                                 # exact duplicate of a row in the ragged last tile
        Q[1] = Vw[77] + 0.05 * rng.standard_normal(d).astype(np.float32)
        ts = 1.7e9 + rng.uniform(0, 30 * 86400.0, size=N)
        _CASES[key] = (Vb, Vw, Q, ts)
    return _CASES[key]


@pytest.mark.parametrize("nq", [5, 16, 33, 128, 130])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_matrix_core_batches(orc, d, nq):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    k = 50
    for metrics in (("dot_product",), ("cosine_similarity", "euclidean_metric")):
        Vb, Vw, Qall, ts = _mfma_case(d, metrics[0] == "dot_product")
        Q = Qall[:nq]
        ix = GpuIndex(Vb)
        try:
            ix.set_option("max_blocks", 8)
            for metric in metrics:
                mid = METRIC_IDS[metric]
                for bias in (False, True):
                    b = None
                    if bias:
                        ix.set_recency(ts, 0.5)
                        b = 0.5 * np.exp(ts - ts.max())
                    else:
                        ix.set_bias(None)
                    tag = (d, nq, metric, bias)
                    mi, ms, mst = ix.topk_device(Q, k, mid)
                    assert ix.stat("mfma") == 1 and ix.stat("fused") == 0 and ix.stat("path") == 1, tag
                    assert int(mst.abs().sum().item()) == 0, tag
                    ne = min(16, nq)
                    ei, es, est = ix.topk_device(Q[:ne], k, mid, exact=True)
                    assert ix.stat("mfma") == 1 and ix.stat("path") == 2 and int(est.abs().sum().item()) == 0, tag
                    assert torch.equal(ei, mi[:ne]) and torch.equal(es, ms[:ne]), tag
                    ix.set_option("use_mfma", 0)
                    vi, vs, _ = ix.topk_device(Q, k, mid)
                    ix.set_option("use_mfma", 1)
                    assert ix.stat("mfma") == 0, tag
                    mi_h, ms_h, vi_h, vs_h = mi.cpu().numpy(), ms.cpu().numpy(), vi.cpu().numpy(), vs.cpu().numpy()
                    for qi in range(nq):
                        assert orc.same_result_modulo_ties(mi_h[qi], ms_h[qi], vi_h[qi], vs_h[qi], TOL), (tag, qi)
                    for qi in (0, 1, nq // 2, nq - 1):
                        orc.check_topk(mi_h[qi], ms_h[qi], Vw, Q[qi], metric, k, bias=b, tol=TOL)
                    if metric == "euclidean_metric" and not bias:
                        assert mi_h[0][0] == N - 2 and abs(ms_h[0][0] - 1.0) < 1e-6 and mi_h[1][0] == 77, tag
        finally:
            ix.close()


def test_matrix_core_pearson_and_few_queries_stay_on_the_valu_scan(orc):
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw, Qall, _ = _mfma_case(384, False)
    Q, k = Qall[:40], 50
    ix = GpuIndex(Vb)
    try:
        ix.set_option("max_blocks", 8)
        mid = METRIC_IDS["pearson_correlation"]
        pi, ps, pst = ix.topk_views(Q, k, mid)
        pi, ps = pi.copy(), ps.copy()
        assert ix.stat("mfma") == 1 and ix.stat("fused") == 0 and int(np.abs(pst).sum()) == 0
        ix.set_option("use_mfma", 0)
        vi, vs, _ = ix.topk_views(Q, k, mid)
        ix.set_option("use_mfma", 1)
        assert ix.stat("mfma") == 0
        for qi in range(40):
            assert orc.same_result_modulo_ties(pi[qi], ps[qi], vi[qi], vs[qi], TOL), qi
        for qi in (0, 1, 20, 39):
            orc.check_topk(pi[qi], ps[qi], Vw, Q[qi], "pearson_correlation", k, tol=TOL)
        for nq in (1, 4):                                 # one VALU pass, unrounded float32 queries
            ix.topk_views(Q[:nq], k, METRIC_IDS["cosine_similarity"])
            assert ix.stat("mfma") == 0 and ix.stat("fused") == 0
        ix.topk_views(Q[:5], k, METRIC_IDS["cosine_similarity"])
        assert ix.stat("mfma") == 1
        ix.topk_views(Q[:16], k, METRIC_IDS["manhattan_distance"])      # no tile kernel for bf16: the 4-query scan
        assert ix.stat("mfma") == 0
    finally:
        ix.close()


def test_matrix_core_other_widths_stay_on_the_valu_scan(orc):
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(100)
    Q = np.random.default_rng(5).standard_normal((16, 100)).astype(np.float32)
    ix = GpuIndex(Vb)
    try:
        i1, s1, st = ix.topk_views(Q, 20, METRIC_IDS["cosine_similarity"])
        assert ix.stat("mfma") == 0 and int(np.abs(st).sum()) == 0
        for qi in (0, 15):
            orc.check_topk(i1[qi], s1[qi], Vw, Q[qi], "cosine_similarity", 20, tol=TOL)
    finally:
        ix.close()


def test_matrix_core_row_mask_equals_valu(orc):
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw, Qall, ts = _mfma_case(256, False)
    rng = np.random.default_rng(11)
    Q, k = Qall[:16], 40
    mask = (rng.random(N) < 0.02).astype(np.uint8)
    mask[:3] = 1
    ix = GpuIndex(Vb)
    try:
        ix.set_option("max_blocks", 8)
        ix.set_row_mask(mask)
        for metric in ("cosine_similarity", "euclidean_metric"):
            mi, ms = ix.topk(Q, k, METRIC_IDS[metric])
            assert ix.stat("mfma") == 1
            ix.set_option("use_mfma", 0)
            vi, vs = ix.topk(Q, k, METRIC_IDS[metric])
            ix.set_option("use_mfma", 1)
            assert ix.stat("mfma") == 0
            for qi in range(16):
                assert mask[mi[qi]].all() and np.isfinite(ms[qi]).all()
                assert orc.same_result_modulo_ties(mi[qi], ms[qi], vi[qi], vs[qi], TOL), (metric, qi)
    finally:
        ix.close()


def test_matrix_core_bf16_exact_queries(orc):
    """Queries that ARE bf16 numbers: their second and third parts are zero, every product and the VALU scan's are the same
    exact numbers, only the order of the float32 additions differs."""
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw, Qall, _ = _mfma_case(384, True)
    Q = torch.from_numpy(Qall[:16]).to(torch.bfloat16).float().numpy()
    ix = GpuIndex(Vb)
    try:
        ix.set_option("max_blocks", 8)
        mid = METRIC_IDS["dot_product"]
        mi, ms = ix.topk(Q, 50, mid)
        assert ix.stat("mfma") == 1
        ix.set_option("use_mfma", 0)
        vi, vs = ix.topk(Q, 50, mid)
        assert ix.stat("mfma") == 0
        for qi in range(16):
            assert orc.same_result_modulo_ties(mi[qi], ms[qi], vi[qi], vs[qi], TOL), qi
            ma, mb = orc.canonical(mi[qi], ms[qi]), orc.canonical(vi[qi], vs[qi])
            same = ma[0] == mb[0]
            assert same.sum() >= 45 and np.all(np.abs(ma[1][same] - mb[1][same]) <= 2e-5 * np.abs(mb[1][same])), qi
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 4. non-finite values are inputs, not faults
# ------------------------------------------------------------------------------------------------
def test_infinite_row_keeps_the_matrix_off_the_matrix_cores(orc):
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(384)
    Wb, Ww = Vb.clone(), Vw.copy()
    Wb[777, 5] = float("inf"); Ww[777, 5] = np.inf
    Q = np.random.default_rng(8).standard_normal((16, 384)).astype(np.float32)
    ix = GpuIndex(Wb)
    try:
        with np.errstate(invalid="ignore"):
            i1, s1, st = ix.topk_views(Q, 20, METRIC_IDS["dot_product"])
            assert ix.stat("mfma") == 0 and int(np.abs(st).sum()) == 0
            for qi in (0, 7, 15):
                orc.check_topk(i1[qi], s1[qi], Ww, Q[qi], "dot_product", 20, tol=TOL)
    finally:
        ix.close()


def test_infinite_query_elements_on_the_matrix_cores(orc):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(384)
    rng = np.random.default_rng(9)
    Q = rng.standard_normal((16, 384)).astype(np.float32)
    bad = list(range(0, 16, 2))
    for j, qi in enumerate(bad):
        Q[qi, 11 + 37 * j] = np.inf if j % 2 == 0 else -np.inf
    mid, k = METRIC_IDS["dot_product"], 20
    ix = GpuIndex(Vb)
    try:
        ix.set_option("max_blocks", 8)
        mi, ms, mst = ix.topk_views(Q, k, mid)           # (a list that overflowed is answered by the exact re-run inside the call)
        mi, ms, mst = mi.copy(), ms.copy(), mst.copy()
        assert int(np.abs(mst).sum()) == 0
        ei, es, est = ix.topk_device(Q, k, mid, exact=True)
        assert ix.stat("mfma") == 1 and int(est.abs().sum().item()) == 0
        ix.set_option("use_mfma", 0)
        vi, vs, vst = ix.topk_views(Q, k, mid)
        vi, vs = vi.copy(), vs.copy()
        xi, xs, _ = ix.topk_device(Q, k, mid, exact=True)
        assert ix.stat("mfma") == 0 and int(np.abs(vst).sum()) == 0
        for qi in bad:
            assert np.isinf(vs[qi]).all() and (vs[qi] > 0).all()             # +inf on every row whose element has the query's sign
            assert np.array_equal(mi[qi], vi[qi]) and np.array_equal(ms[qi], vs[qi]), qi
            assert torch.equal(ei[qi], xi[qi]) and torch.equal(es[qi], xs[qi]), qi
            assert np.array_equal(ei[qi].cpu().numpy(), vi[qi])
        for qi in (1, 15):
            orc.check_topk(mi[qi], ms[qi], Vw, Q[qi], "dot_product", k, tol=TOL)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 5. lifecycle
# ------------------------------------------------------------------------------------------------
def test_append_compact_quantize_and_auto_quant():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 128
    Vb, Vw = _matrix(d)
    rng = np.random.default_rng(12)
    extra32 = rng.standard_normal((3_001, d)).astype(np.float32)           # float32 rows: rounded to bf16 on the way in
    extra_b, extra_w = _bf16(extra32)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    n0 = 9_000
    ix = GpuIndex(Vb[:n0].clone())
    try:
        ix.topk(Q[:1], 5, METRIC_IDS["hamming_distance"])                  # builds the sign-bit cache that append must extend
        ix.append(extra32[:1])
        ix.append(extra32[1:])
        assert ix.n == n0 + 3_001 and ix.V.dtype == torch.bfloat16
        assert np.array_equal(ix.host_matrix()[n0:], extra_w)
        keep = np.flatnonzero(rng.random(ix.n) < 0.9)
        ix.compact(keep)
        assert ix.n == keep.size and ix.V.dtype == torch.bfloat16
        fresh = GpuIndex(torch.cat([Vb[:n0], extra_b])[torch.from_numpy(keep).cuda()].contiguous())
        try:
            assert np.array_equal(ix.host_matrix(), fresh.host_matrix())
            for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "hamming_distance", "pearson_correlation"):
                for sl in (slice(0, 1), slice(0, 16)):
                    i1, s1 = ix.topk(Q[sl], 30, METRIC_IDS[metric])
                    m1 = ix.stat("mfma")
                    i2, s2 = fresh.topk(Q[sl], 30, METRIC_IDS[metric])
                    assert m1 == fresh.stat("mfma") == (1 if (sl.stop == 16 and metric != "hamming_distance") else 0), (metric, sl)
                    assert np.array_equal(i1, i2) and np.array_equal(s1, s2), (metric, sl)
        finally:
            fresh.close()
        with pytest.raises(NotImplementedError, match="bf16"):
            ix.quantize("int8")
        ix.set_option("quant_min_n", 0)
        ix.topk(Q[:1], 30, METRIC_IDS["cosine_similarity"])
        assert ix.stat("quant_auto") == 0 and ix.stat("quant") == 0
        # update: float32 data into a bf16 index is rounded the same way
        ix.update(torch.from_numpy(extra32).cuda())
        assert ix.n == 3_001 and np.array_equal(ix.host_matrix(), extra_w)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 6. the facade
# ------------------------------------------------------------------------------------------------
def _facade_data():
    rng = np.random.default_rng(21)
    n, d = 9_001, 128
    V32 = rng.standard_normal((n, d)).astype(np.float32)
    _, Vw = _bf16(V32)
    docs = [{"id": i, "text": f"doc {i}"} for i in range(n)]
    Q = rng.standard_normal((8, d)).astype(np.float32)
    return V32, Vw, docs, Q


def _same_answers(got, want):
    assert len(got) == len(want)
    for (gd, gs, gi), (wd, ws, wi) in zip(got, want):
        assert gd == wd and gi == wi
        assert abs(float(gs) - float(ws)) <= TOL * max(1.0, abs(float(ws)))


def test_facade_bfloat16(tmp_path):
    import torch
    from hyperdb import HyperDB
    V32, Vw, docs, Q = _facade_data()
    db = HyperDB(docs, V32, fp_precision="bfloat16")
    ref = HyperDB(docs, Vw, fp_precision="float32")
    assert db._index.V.dtype == torch.bfloat16 and db._index.dtype == 3
    assert db.vectors.dtype == np.float32 and np.array_equal(db.vectors, Vw)
    for metric in ("cosine_similarity", "euclidean_metric"):
        _same_answers(db.query(Q[0], top_k=10, metric=metric), ref.query(Q[0], top_k=10, metric=metric))
        for got, want in zip(db.query_batch(Q, top_k=10, metric=metric), ref.query_batch(Q, top_k=10, metric=metric)):
            _same_answers(got, want)
    db.add([{"id": -1}], V32[:1] * 2.0)                     # appended through the facade: rounded like the first upload
    assert db._index.V.dtype == torch.bfloat16 and db.vectors.shape == (len(docs) + 1, 128)
    for fmt, name in (("pickle", "db.pickle"), ("json", "db.json")):
        path = str(tmp_path / name)
        db.save(path, format=fmt)
        back = HyperDB(fp_precision="bfloat16")
        back.load(path, format=fmt)
        assert back._index.V.dtype == torch.bfloat16
        assert back.vectors.dtype == np.float32 and np.array_equal(back.vectors, db.vectors)
        _same_answers(back.query(Q[1], top_k=10), db.query(Q[1], top_k=10))


def test_facade_bfloat16_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    from hyperdb import HyperDB
    V32, Vw, docs, Q = _facade_data()
    one = HyperDB(docs, V32, fp_precision="bfloat16")
    two = HyperDB(docs, V32, fp_precision="bfloat16", devices=[0, 1])
    assert all(s.V.dtype == torch.bfloat16 for s in two._index.shards)
    assert np.array_equal(two.vectors, Vw)
    _same_answers(two.query(Q[0], top_k=10), one.query(Q[0], top_k=10))
    for got, want in zip(two.query_batch(Q, top_k=10), one.query_batch(Q, top_k=10)):
        _same_answers(got, want)


# every bfloat16 shard launcher of the matrix-core scan x {dot, cosine, euclidean} x {no bias, bias} (tests/launcher_cells.py;
# profiles/mfma_launch_coverage.txt): whole rows 128 / 256 and 384 / 512, K slices of 256 / 384 (d = 640) and of 512 (d = 1024, 4096)
@pytest.mark.parametrize("d", [128, 256, 384, 512, 640, 1024, 4096])
def test_every_bf16_launcher_metric_and_bias(orc, d):
    import launcher_cells
    launcher_cells.check_launcher_cells(orc, "bf16", d, 5, {"bf16_ks_min_q": 5}, TOL, {"mfma": 1, "fused": 0})
