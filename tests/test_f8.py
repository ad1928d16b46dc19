"""GPU tests (-m gpu) of the float8 e4m3 storage dtype (HDB_F8E4M3 = 5): a torch.float8_e4m3fn matrix stays one byte per element on
the device, the VALU scans serve every metric on it, and batches of 5+ dot / cosine / euclidean / pearson queries run on the bf16
matrix cores (hdb_mfma_f8.hip): rows converted per fragment in registers, the float32 queries split into three exact bf16 parts.

Reference: oracle/ranking_oracle.py on the exactly widened float32 matrix.  Every finite e4m3 code IS a float32 value and every
path computes in float32 on it, so the tolerance is the project's float32 contract, 1e-5 applied as tol * max(1, |s|); hamming is
bit-exact, jaccard (a ratio of two integers <= d evaluated in float32) 1e-6.  Matrices are standard_normal float32 converted with
torch (largest magnitude about 5, far from 448).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "hamming_distance", "manhattan_distance",
           "jaccard_similarity", "pearson_correlation")
N = 20_003                                             # many tiles per workgroup, ragged last 16-row tile


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


def _dev(t8):
    """host float8 tensor -> the same bytes on the GPU."""
    import torch
    return t8.contiguous().view(torch.uint8).cuda().view(torch.float8_e4m3fn)


def _f8(a32):
    """float32 array -> (float8 CUDA tensor, its exact float32 widening on the host); torch's conversion, on the host."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.float8_e4m3fn)
    return _dev(t), t.float().numpy()


def _rows(Vb, sel):
    """rows of a device float8 tensor, through its bytes."""
    import torch
    idx = torch.as_tensor(sel, device=Vb.device) if not isinstance(sel, slice) else sel
    return Vb.view(torch.uint8)[idx].contiguous().view(torch.float8_e4m3fn)


_MATS = {}


def _matrix(d, n=N):
    """One (float8 device tensor, widened host matrix) per shape, shared by the tests and never modified."""
    key = (d, n)
    if key not in _MATS:
        rng = np.random.default_rng(1000 * d + n)
        _MATS[key] = _f8(rng.standard_normal((n, d)).astype(np.float32))
    return _MATS[key]


# ------------------------------------------------------------------------------------------------
# 1. storage and codes
# ------------------------------------------------------------------------------------------------
def test_storage_is_one_byte_per_element():
    import torch
    from hyperdb._native import GpuIndex, HDB_F8E4M3
    Vb, Vw = _matrix(100)
    ix = GpuIndex(Vb)
    try:
        assert ix.dtype == HDB_F8E4M3 == 5
        assert ix.V.dtype == torch.float8_e4m3fn and ix.V.element_size() * ix.n * ix.d == N * 100
        host = ix.host_matrix()
        assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), Vw.view(np.uint32))
        assert not ix.has_nan
    finally:
        ix.close()


def _code_matrix():
    """1 024 x 48 random finite codes with every one of the 254 finite codes present, as (uint8 array, widened float32)."""
    import torch
    finite = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)
    rng = np.random.default_rng(48)
    codes = finite[rng.integers(0, 254, size=(1024, 48))]
    codes.reshape(-1)[rng.permutation(codes.size)[:254]] = finite           # every finite code, at random places
    wide = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    return codes, wide


def test_every_code_and_every_byte_position(ranking):
    """One-hot queries: the dot product with e_j is column j of the widening, exactly -- pins the byte order of all 16 positions
    of a chunk (48 bytes = three chunks, the lanes past the third idle) and the widening of every finite code."""
    import torch
    codes, wide = _code_matrix()
    present = set(codes.reshape(-1).tolist())
    assert len(present) == 254 and {0x00, 0x80, 0x01, 0x81, 0x07, 0x87, 0x7E, 0xFE} <= present      # +-0, the subnormal ends, +-448
    assert np.isfinite(wide).all() and wide.max() == 448.0 and wide.min() == -448.0
    h = ranking.register_vectors(_dev(torch.from_numpy(codes).view(torch.float8_e4m3fn)))
    try:
        assert not h.index.has_nan
        for j in range(48):
            q = np.zeros(48, dtype=np.float32)
            q[j] = 1.0
            got = np.asarray(ranking.dot_product(h, q))
            assert got.shape == (1024,) and np.all(got == wide[:, j]), j      # (== : -0 equals +0)
    finally:
        h.close()


def test_nan_codes_raise_the_flag():
    import torch
    from hyperdb._native import GpuIndex
    codes, _ = _code_matrix()
    for code in (0x7F, 0xFF):
        bad = codes.copy()
        bad[1000, 47] = code
        ix = GpuIndex(_dev(torch.from_numpy(bad).view(torch.float8_e4m3fn)))
        try:
            assert ix.has_nan, hex(code)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------
# 2. VALU scans: every metric at d = 384 / 256 / 512 (the unrolled kernels of 24 / 16 / 32 chunks), 272 (17 chunks: one past a
#    full step of the runtime loop), 100 and 7 (the element-wise scan)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [384, 256, 512, 272, 100, 7])
def test_valu_scans_all_metrics(ranking, orc, d):
    Vb, Vw = _matrix(d)
    rng = np.random.default_rng(d)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    Q[1] = Vw[N - 2] + 0.05 * rng.standard_normal(d).astype(np.float32)
    k = 20
    h = ranking.register_vectors(Vb)
    try:
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
    h = ranking.register_vectors(_rows(Vb, slice(0, n)))
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
    d = 384
    Vb, Vw = _matrix(d)
    rng = np.random.default_rng(77)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    ix = GpuIndex(Vb)
    try:
        # the exact selection against the sampled one, bit for bit: one query (the unrolled kernel) and three (the four-query kernel)
        for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "manhattan_distance", "pearson_correlation"):
            mid = METRIC_IDS[metric]
            for nq in (1, 3):
                si, ss, st = ix.topk_device(Q[:nq], 20, mid)
                assert ix.stat("path") == 1 and ix.stat("mfma") == 0 and ix.stat("fused") == 0
                ei, es, est = ix.topk_device(Q[:nq], 20, mid, exact=True)
                assert ix.stat("path") == 2 and ix.stat("mfma") == 0 and int(st.abs().sum().item()) == 0 and int(est.abs().sum().item()) == 0
                assert torch.equal(si, ei) and torch.equal(ss.view(torch.int32), es.view(torch.int32)), (metric, nq)
        mid = METRIC_IDS["cosine_similarity"]
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
# 3. the row list: indices, score bits and status words of a fresh float8 index over V[rows] with bias[rows]
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1_000, 20_001])
def test_row_list_equals_a_fresh_index(m):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    n, d, k = 60_001, 384, 30
    Vb, _ = _matrix(d, n)
    rng = np.random.default_rng(m)
    rows = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    mask = np.zeros(n, dtype=np.uint8)
    mask[rows] = 1
    bias = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    Q = rng.standard_normal((4, d)).astype(np.float32)
    ix = GpuIndex(Vb)
    fresh = GpuIndex(_rows(Vb, rows))
    try:
        ix.set_option("subset_min_n", 0)
        ix.set_option("subset_ratio", 1)
        for name in ("use_mfma", "use_fused", "use_quant", "use_l1_tile"):
            fresh.set_option(name, 0)
        for with_bias in (False, True):
            ix.set_bias(bias if with_bias else None)
            fresh.set_bias(bias[rows] if with_bias else None)
            ix.set_row_subset(mask, rows)
            for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "manhattan_distance", "pearson_correlation"):
                for nq in (1, 4):
                    for exact in ((False, True) if m > 8192 and nq == 1 else (False,)):
                        gi, gs, gst = ix.topk_device(Q[:nq], k, METRIC_IDS[metric], exact=exact)
                        assert ix.stat("subset") == 1 and ix.stat("subset_rows") == m and ix.stat("mfma") == 0 and ix.stat("fused") == 0
                        wi, ws, wst = fresh.topk_device(Q[:nq], k, METRIC_IDS[metric], exact=exact)
                        assert ix.stat("path") == fresh.stat("path") == (0 if m <= 8192 else 2 if exact else 1)
                        tag = (m, with_bias, metric, nq, exact)
                        assert np.array_equal(gi.cpu().numpy(), rows[wi.cpu().numpy()]), tag
                        assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), tag
    finally:
        ix.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------
# 4. matrix-core batches (5+ queries, d = 128 / 256 / 384 / 512)
# ------------------------------------------------------------------------------------------------
_CASES = {}


def _batch_case(d, dot):
    """Matrix with one row scaled by 2^-4 and -- not for the dot product, where a score against such a row cancels to a small
    share of |v||q| and float32 itself is no better than 1e-5 of THAT score -- one by 32 (powers of two: the scaled rows are
    float8 numbers again, largest magnitude ~160)."""
    key = (d, dot)
    if key not in _CASES:
        rng = np.random.default_rng(977 * d)
        _, W = _f8(rng.standard_normal((N, d)).astype(np.float32))
        W = W.copy()
        W[1234] *= 2.0 ** -4
        if not dot:
            W[4321] *= 32.0
        Vb, Vw = _f8(W)
        Q = rng.standard_normal((130, d)).astype(np.float32)
        Q[0] = Vw[N - 2]                                 # exact duplicate of a row in the ragged last tile
        Q[1] = Vw[77] + 0.05 * rng.standard_normal(d).astype(np.float32)
        _CASES[key] = (Vb, Vw, Q)
    return _CASES[key]


@pytest.mark.parametrize("nq", [5, 16, 17, 130])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_matrix_core_batches(orc, d, nq):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    k = 50
    for metrics in (("dot_product",), ("cosine_similarity", "euclidean_metric", "pearson_correlation")):
        Vb, Vw, Qall = _batch_case(d, metrics[0] == "dot_product")
        Q = Qall[:nq]
        ix = GpuIndex(Vb)
        try:
            for metric in metrics:
                mid = METRIC_IDS[metric]
                tag = (d, nq, metric)
                mi, ms, mst = ix.topk_device(Q, k, mid)
                assert ix.stat("mfma") == 1 and ix.stat("fused") == 0 and ix.stat("path") == 1 and ix.stat("quant") == 0, tag
                assert int(mst.abs().sum().item()) == 0, tag
                ne = min(17, nq)
                ei, es, est = ix.topk_device(Q[:ne], k, mid, exact=True)
                assert ix.stat("mfma") == 1 and ix.stat("path") == 2 and int(est.abs().sum().item()) == 0, tag
                assert torch.equal(ei, mi[:ne]) and torch.equal(es.view(torch.int32), ms[:ne].view(torch.int32)), tag
                mi_h, ms_h = mi.cpu().numpy(), ms.cpu().numpy()
                for qi in sorted({0, 1, nq // 2, nq - 1}):
                    orc.check_topk(mi_h[qi], ms_h[qi], Vw, Q[qi], metric, k, tol=TOL)
                if metric == "euclidean_metric":
                    assert mi_h[0][0] == N - 2 and abs(ms_h[0][0] - 1.0) < 1e-6 and mi_h[1][0] == 77, tag
        finally:
            ix.close()


def test_matrix_core_one_hot_batch_returns_the_columns():
    """The 128 one-hot float32 queries as ONE batch at d = 128: the second and third query parts are zero, every product is exact,
    so query j's top-k are the k largest entries of column j, exactly -- pins the k slot of every lane and k-step."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(128)
    ix = GpuIndex(Vb)
    try:
        Q = np.eye(128, dtype=np.float32)
        idx, sc, st = ix.topk_views(Q, 10, METRIC_IDS["dot_product"])
        assert ix.stat("mfma") == 1 and ix.stat("fused") == 0 and int(np.abs(st).sum()) == 0
        for j in range(128):
            col = Vw[:, j]
            assert np.array_equal(sc[j], np.sort(col)[::-1][:10]) and np.array_equal(col[idx[j]], sc[j]), j
    finally:
        ix.close()


def test_matrix_core_bits_equal_a_bfloat16_index():
    """The K walk is the bfloat16 flavour's (k-steps in order, smallest query part first, the same fragment map and epilogue) and a
    float8 code is a bf16 number: indices and scores of a bfloat16 index over the widened matrix, bit for bit."""
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(256)
    Q = np.random.default_rng(256).standard_normal((16, 256)).astype(np.float32)
    f8 = GpuIndex(Vb)
    bf = GpuIndex(torch.from_numpy(Vw).to(torch.bfloat16).cuda())
    try:
        assert np.array_equal(bf.host_matrix(), Vw)
        for metric in ("cosine_similarity", "dot_product", "euclidean_metric"):
            i1, s1 = f8.topk(Q, 50, METRIC_IDS[metric])
            i2, s2 = bf.topk(Q, 50, METRIC_IDS[metric])
            assert f8.stat("mfma") == 1 and bf.stat("mfma") == 1
            assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32)), metric
    finally:
        f8.close()
        bf.close()


def test_nan_code_stays_on_the_valu_scan_and_infinite_query_keeps_status_zero():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(384)
    W = Vb.view(torch.uint8).clone()
    W[777, 5] = 0x7F
    Ww = Vw.copy()
    Ww[777, 5] = np.nan
    rng = np.random.default_rng(8)
    Q = rng.standard_normal((16, 384)).astype(np.float32)
    ix = GpuIndex(W.view(torch.float8_e4m3fn))
    try:
        assert ix.has_nan
        i1, s1, st = ix.topk_views(Q, 20, METRIC_IDS["dot_product"])
        assert ix.stat("mfma") == 0 and int(np.abs(st).sum()) == 0
        with np.errstate(invalid="ignore"):
            want = Ww.astype(np.float64) @ Q.astype(np.float64).T
        want[np.isnan(want)] = -np.inf                                   # NaN -> -inf, like the reference
        for qi in range(16):
            assert 777 not in i1[qi]
            top = np.sort(want[:, qi])[::-1][:20]
            assert np.all(np.abs(s1[qi] - top) <= TOL * np.maximum(1.0, np.abs(top))), qi
    finally:
        ix.close()
    Qi = Q.copy()
    bad = list(range(0, 16, 2))
    for j, qi in enumerate(bad):
        Qi[qi, 11 + 37 * j] = np.inf if j % 2 == 0 else -np.inf
    mid, k = METRIC_IDS["dot_product"], 20
    ix = GpuIndex(Vb)
    try:
        mi, ms, mst = ix.topk_views(Qi, k, mid)           # (a list that overflowed is answered by the exact re-run inside the call)
        mi, ms, mst = mi.copy(), ms.copy(), mst.copy()
        assert int(np.abs(mst).sum()) == 0
        ei, es, est = ix.topk_device(Qi, k, mid, exact=True)
        assert ix.stat("mfma") == 1 and int(est.abs().sum().item()) == 0
        ix.set_option("use_mfma", 0)
        vi, vs, vst = ix.topk_views(Qi, k, mid)
        vi, vs = vi.copy(), vs.copy()
        assert ix.stat("mfma") == 0 and int(np.abs(vst).sum()) == 0
        for qi in bad:
            assert np.isinf(vs[qi]).all() and (vs[qi] > 0).all()          # +inf on every row whose element has the query's sign
            assert np.array_equal(mi[qi], vi[qi]) and np.array_equal(ms[qi], vs[qi]), qi
            assert np.array_equal(ei[qi].cpu().numpy(), vi[qi])
    finally:
        ix.close()


def test_other_widths_and_manhattan_batches_stay_on_the_valu_scan(orc):
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, Vw = _matrix(100)
    Q = np.random.default_rng(5).standard_normal((16, 100)).astype(np.float32)
    ix = GpuIndex(Vb)
    try:
        for metric in ("cosine_similarity", "manhattan_distance"):
            i1, s1, st = ix.topk_views(Q, 20, METRIC_IDS[metric])
            assert ix.stat("mfma") == 0 and int(np.abs(st).sum()) == 0
            for qi in (0, 15):
                orc.check_topk(i1[qi], s1[qi], Vw, Q[qi], metric, 20, tol=TOL)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 5. lifecycle
# ------------------------------------------------------------------------------------------------
def test_append_compact_update_and_no_shadow():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 128
    Vb, Vw = _matrix(d)
    rng = np.random.default_rng(12)
    extra32 = rng.standard_normal((3_001, d)).astype(np.float32)           # float32 rows: converted to float8 on the way in
    extra_b, extra_w = _f8(extra32)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    n0 = 9_000
    ix = GpuIndex(_rows(Vb, slice(0, n0)))
    try:
        ix.topk(Q[:1], 5, METRIC_IDS["hamming_distance"])                  # builds the sign-bit cache that append must extend
        ix.append(extra32[:1])
        assert ix.n == n0 + 1 and np.array_equal(ix.host_matrix()[n0:], extra_w[:1])
        ix.append(extra32[1:])
        assert ix.n == n0 + 3_001 and ix.V.dtype == torch.float8_e4m3fn and ix.V.element_size() == 1
        assert np.array_equal(ix.host_matrix()[n0:], extra_w) and np.array_equal(ix.host_matrix()[:n0], Vw[:n0])
        keep = np.flatnonzero(rng.random(ix.n) < 0.9)
        ix.compact(keep)
        assert ix.n == keep.size and ix.V.dtype == torch.float8_e4m3fn
        whole = torch.cat([Vb.view(torch.uint8)[:n0], extra_b.view(torch.uint8)])
        fresh = GpuIndex(whole[torch.from_numpy(keep).cuda()].contiguous().view(torch.float8_e4m3fn))
        try:
            assert np.array_equal(ix.host_matrix(), fresh.host_matrix())
            assert np.array_equal(ix.host_matrix(), np.concatenate([Vw[:n0], extra_w])[keep])
            for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "hamming_distance", "pearson_correlation"):
                for sl in (slice(0, 1), slice(0, 16)):
                    i1, s1 = ix.topk(Q[sl], 30, METRIC_IDS[metric])
                    m1 = ix.stat("mfma")
                    i2, s2 = fresh.topk(Q[sl], 30, METRIC_IDS[metric])
                    assert m1 == fresh.stat("mfma") == (1 if (sl.stop == 16 and metric != "hamming_distance") else 0), (metric, sl)
                    assert np.array_equal(i1, i2) and np.array_equal(s1, s2), (metric, sl)
        finally:
            fresh.close()
        with pytest.raises(NotImplementedError, match="float8"):
            ix.quantize("int8")
        ix.set_option("quant_min_n", 0)
        ix.topk(Q[:1], 30, METRIC_IDS["cosine_similarity"])
        assert ix.stat("quant_auto") == 0 and ix.stat("quant") == 0
        # update: float32 data into a float8 index is converted the same way
        ix.update(torch.from_numpy(extra32).cuda())
        assert ix.n == 3_001 and ix.V.dtype == torch.float8_e4m3fn and np.array_equal(ix.host_matrix(), extra_w)
        ix.update(extra32[:100])
        assert ix.n == 100 and np.array_equal(ix.host_matrix(), extra_w[:100])
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 6. the facade and the group
# ------------------------------------------------------------------------------------------------
def _facade_data():
    rng = np.random.default_rng(21)
    n, d = 9_001, 128
    V32 = rng.standard_normal((n, d)).astype(np.float32)
    _, Vw = _f8(V32)
    t0 = 1.7e9
    docs = [{"id": i, "text": f"doc {i}", "timestamp": t0 + 3600.0 * i, "info": {"type": "even" if i % 2 == 0 else "odd"}} for i in range(n)]
    Q = rng.standard_normal((8, d)).astype(np.float32)
    return V32, Vw, docs, Q


def _same_answers(got, want):
    assert len(got) == len(want)
    for (gd, gs, gi), (wd, ws, wi) in zip(got, want):
        assert gd == wd and gi == wi
        assert abs(float(gs) - float(ws)) <= TOL * max(1.0, abs(float(ws)))


def test_facade_float8(tmp_path, orc):
    import torch
    from hyperdb import HyperDB
    V32, Vw, docs, Q = _facade_data()
    keys = ["timestamp", "info.type"]
    db = HyperDB([dict(x) for x in docs], V32, fp_precision="float8_e4m3fn", metadata_keys=keys)
    assert db._index.V.dtype == torch.float8_e4m3fn and db._index.dtype == 5 and db._index.V.element_size() == 1
    assert db.vectors.dtype == np.float32 and np.array_equal(db.vectors, Vw)
    # a metadata filter with a recency bias, against the oracle on the widened vectors (both decays over the kept documents)
    keep = np.array([i % 2 == 1 for i in range(len(docs))])
    res = db.query(Q[0], top_k=10, recency_bias=0.8, timestamp_key="timestamp", metric="cosine_similarity",
                   filters=[("metadata", {"info.type": "odd"})])
    ts = np.array([docs[i]["timestamp"] for i in np.flatnonzero(keep)])
    first = 0.8 * np.exp(ts - ts.max())
    oi, osc = orc.rank(Vw[keep], Q[0], top_k=10, metric="cosine_similarity", timestamps=first, recency_bias=0.8)
    assert [r[2] for r in res] == list(np.flatnonzero(keep)[oi])
    assert np.all(np.abs(np.array([r[1] for r in res]) - osc) <= TOL * np.maximum(1.0, np.abs(osc)))
    # ... and plain calls against a float32 database over the widened vectors
    ref = HyperDB([dict(x) for x in docs], Vw, fp_precision="float32", metadata_keys=keys)
    for metric in ("cosine_similarity", "euclidean_metric"):
        _same_answers(db.query(Q[0], top_k=10, metric=metric), ref.query(Q[0], top_k=10, metric=metric))
        for got, want in zip(db.query_batch(Q, top_k=10, metric=metric), ref.query_batch(Q, top_k=10, metric=metric)):
            _same_answers(got, want)
    # add / remove keep the dtype; the appended row is converted like the first upload
    db.add([{"id": -1}], V32[:1] * 2.0)
    assert db._index.V.dtype == torch.float8_e4m3fn and db.vectors.shape == (len(docs) + 1, 128)
    assert np.array_equal(db.vectors[-1], _f8(V32[:1] * 2.0)[1][0])
    db.remove_document(3)
    assert db.size() == len(docs) and np.array_equal(db.vectors[3], Vw[4])
    with pytest.raises(ValueError, match="448"):
        db.add([{"id": -2}], np.full((1, 128), 500.0, dtype=np.float32))
    assert db.size() == len(docs)
    path = str(tmp_path / "db.pickle")
    db.save(path, format="pickle")
    back = HyperDB(fp_precision="float8_e4m3fn")
    back.load(path, format="pickle")
    assert back._index.V.dtype == torch.float8_e4m3fn
    assert back.vectors.dtype == np.float32 and np.array_equal(back.vectors, db.vectors)
    _same_answers(back.query(Q[1], top_k=10), db.query(Q[1], top_k=10))


def test_two_shards_on_one_device(ranking):
    """GpuGroup over a float8 tensor (shards are GpuIndexes): the merged answer is the single index's."""
    import torch
    Vb, Vw = _matrix(384)
    Q = np.random.default_rng(31).standard_normal((5, 384)).astype(np.float32)
    one = ranking.register_vectors(Vb)
    two = ranking.register_vectors(Vb.view(torch.uint8).cpu().view(torch.float8_e4m3fn), devices=[0, 0])
    try:
        assert all(s.V.dtype == torch.float8_e4m3fn and s.dtype == 5 for s in two.index.shards)
        assert np.array_equal(two.index.host_matrix(), Vw)
        for metric in ("cosine_similarity", "euclidean_metric", "hamming_distance"):
            a = ranking.rank_batch(one, Q.copy(), top_k=15, metric=metric)
            b = ranking.rank_batch(two, Q.copy(), top_k=15, metric=metric)
            assert np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1])), metric
    finally:
        one.close()
        two.close()


# every float8 shard launcher of the matrix-core scan x {dot, cosine, euclidean} x {no bias, bias} (tests/launcher_cells.py;
# profiles/mfma_launch_coverage.txt): registers and LDS, whole rows and K slices (d = 640: slices of 384 / 256, d = 1024: of 512);
# 5 queries and 17, where the register kernels' query groups per workgroup go from one to two
_F8_LAUNCHERS = [("regs", d, nq, {}, 0) for d in (128, 256, 384, 512) for nq in (5, 17)] + \
                [("regs-kslice", d, nq, {"f8_ks_min_q": 5}, 0) for d in (640, 1024) for nq in (5, 17)] + \
                [("lds", d, 5, {"f8_lds_min_q": 5}, 1) for d in (128, 256, 384, 512)] + \
                [("lds-kslice", d, 17, {"f8_ks_min_q": 5, "f8_lds_min_q": 5}, 1) for d in (640, 1024)]


@pytest.mark.parametrize("launcher,d,nq,opts,lds", _F8_LAUNCHERS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in _F8_LAUNCHERS])
def test_every_f8_launcher_metric_and_bias(orc, launcher, d, nq, opts, lds):
    import launcher_cells
    launcher_cells.check_launcher_cells(orc, "f8", d, nq, opts, TOL, {"mfma": 1, "fused": 0, "f8_lds": lds})
