"""GPU tests (-m gpu) of float8 e4m3 matrices wider than 512 elements on the bf16 matrix cores: with the option f8_ks_min_q set,
batches of 5+ dot / cosine / euclidean / pearson queries go through K slices of 256 / 384 / 512 elements (hdb_mfma_f8_ks.hip, the
slice lists are ks_geom_f8 in hdb_caps.h), one launch per slice, rows converted per fragment in registers, partial sums carried in
a [query][rows] float32 buffer.  The option is 0 by default: without it every call takes the path it took before the slices existed.

References: oracle/ranking_oracle.py on the exactly widened float32 matrix; the same call with use_mfma = 0 (the VALU scan, four
queries per pass); and a bfloat16 index over the widened matrix through ITS K slices.  A finite e4m3 code IS a float32 value (and a
bf16 value) and every path computes in float32 on it, so the tolerance against the first two is the project's float32 contract,
1e-5 applied as tol * max(1, |s|), and the third is an identity: the slice list, the K walk and the epilogue are the bfloat16
kernel's, so indices and score bits are equal.

The float64 scores that check_topk compares against are computed once per matrix and metric for the queries the cases look at (0,
1, nq // 2 and nq - 1 of every batch size) and handed to it through its `exact` argument.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 20_003                                             # above the 8192-row small path; 8 workgroups x many 16-row tiles, the last one ragged
NQS = (5, 20, 33, 130)                                 # one, two and four query groups per workgroup; a second chunk behind 128 queries
CHECKED = sorted({qi for nq in NQS for qi in (0, 1, nq // 2, nq - 1)})


@pytest.fixture(scope="module")
def orc():
    from oracle import ranking_oracle
    return ranking_oracle


def _dev(t8):
    """host float8 tensor -> the same bytes on the GPU."""
    import torch
    return t8.contiguous().view(torch.uint8).cuda().view(torch.float8_e4m3fn)


def _f8(a32):
    """float32 array -> (float8 CUDA tensor, its exact float32 widening on the host); torch's conversion, on the host.  No code of
    the uploaded tensor is NaN."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.float8_e4m3fn)
    Vb = _dev(t)
    assert int(((Vb.view(torch.uint8) & 0x7F) == 0x7F).sum().item()) == 0, "a NaN code (0x7F / 0xFF) in the matrix"
    return Vb, t.float().numpy()


def _exact_many(Vw, Q, metric):
    """float64 scores [len(Q)][N] of `metric` on the stored values (oracle.exact_scores' arithmetic, a row block widened once for
    all queries)."""
    Q64 = np.asarray(Q, dtype=np.float64)
    out = np.empty((Q64.shape[0], Vw.shape[0]), dtype=np.float64)
    qn2 = (Q64 * Q64).sum(axis=1)
    for lo in range(0, Vw.shape[0], 4096):
        V = Vw[lo:lo + 4096].astype(np.float64)
        dots = Q64 @ V.T
        vn2 = (V * V).sum(axis=1)
        if metric == "dot_product":
            s = dots
        elif metric == "cosine_similarity":
            vn, qn = np.sqrt(vn2), np.sqrt(qn2)
            vn[vn == 0] = 1.0
            qn[qn == 0] = 1.0
            s = dots / (vn[None, :] * qn[:, None])
        else:
            d2 = np.maximum(vn2[None, :] + qn2[:, None] - 2.0 * dots, 0.0)
            for qi, r in zip(*np.nonzero(d2 < 0.25 * qn2[:, None])):      # near a query: the direct difference, as the oracle forms it
                diff = V[r] - Q64[qi]
                d2[qi, r] = (diff * diff).sum()
            s = 1.0 / (1.0 + np.sqrt(d2))
        out[:, lo:lo + V.shape[0]] = s
    return out


_CASE = {}


def _case(d, dot):
    """The matrix of test_bf16_wide's _case at width d, as float8: rows and queries N(0, 1), one row scaled by 0.05 and -- not for the
    dot product, where a score against such a row cancels to a small share of |v||q| and float32 itself is no better than 1e-5 of
    THAT score -- one by 50, clipped to the float8 range (+-448), so that torch's conversion produces no NaN code.  One width at a
    time is kept (the parametrisation runs width by width), shared by its cases and never modified."""
    if _CASE.get("d") != d:
        _CASE.clear()
        _CASE["d"] = d
    if dot not in _CASE:
        rng = np.random.default_rng(977 * d)
        V32 = rng.standard_normal((N, d)).astype(np.float32)
        V32[1234] *= 0.05
        if not dot:
            V32[4321] *= 50.0
        np.clip(V32, -448.0, 448.0, out=V32)
        Vb, Vw = _f8(V32)
        del V32
        Q = rng.standard_normal((130, d)).astype(np.float32)
        Q[0] = Vw[N - 2]                                 # exact duplicate of a row in the ragged last tile
        Q[1] = Vw[77] + 0.05 * rng.standard_normal(d).astype(np.float32)
        ts = 1.7e9 + rng.uniform(0, 30 * 86400.0, size=N)
        metrics = ("dot_product",) if dot else ("cosine_similarity", "euclidean_metric")
        exact = {m: dict(zip(CHECKED, _exact_many(Vw, Q[CHECKED], m))) for m in metrics}
        _CASE[dot] = (Vb, Vw, Q, ts, exact)
    return _CASE[dot]


def _index(Vb, min_q=5):
    from hyperdb._native import GpuIndex
    ix = GpuIndex(Vb)
    ix.set_option("max_blocks", 8)                       # a workgroup walks many tiles
    if min_q is not None:
        ix.set_option("f8_ks_min_q", min_q)              # unknown before the slices existed: every test that sets it fails there
    return ix


# ------------------------------------------------------------------------------------------------
# 1. paths and parity: mixed slices (640 = 384 + 256), two equal (768), three mixed (1280 = 512 + 2 x 384), eight slices (4096)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d", [640, 768, 1280, 4096])
def test_k_slice_batches(orc, d, nq):
    import torch
    from hyperdb._native import METRIC_IDS
    k = 50
    for metrics in (("dot_product",), ("cosine_similarity", "euclidean_metric")):
        Vb, Vw, Qall, ts, exact = _case(d, metrics[0] == "dot_product")
        Q = Qall[:nq]
        ix = _index(Vb)
        try:
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
                        ref = exact[metric][qi] if b is None else exact[metric][qi] + b
                        err = np.abs(ms_h[qi].astype(np.float64) - ref[mi_h[qi]]) / np.maximum(1.0, np.abs(ref[mi_h[qi]]))
                        print(f"{tag} query {qi}: largest score error {err.max():.3e} of the band {TOL:g}")
                        orc.check_topk(mi_h[qi], ms_h[qi], Vw, Q[qi], metric, k, bias=b, tol=TOL, exact=ref)
                    if metric == "euclidean_metric" and not bias:
                        assert mi_h[0][0] == N - 2 and abs(ms_h[0][0] - 1.0) < 1e-6 and mi_h[1][0] == 77, tag
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------
# 2. the contract: the bits of a bfloat16 index over the widened matrix through its K slices
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [640, 1280])
def test_bits_equal_a_bfloat16_index_through_its_slices(d):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    nq, k = 33, 50
    for metrics in (("dot_product",), ("cosine_similarity", "euclidean_metric")):
        Vb, Vw, Qall, _, _ = _case(d, metrics[0] == "dot_product")
        Q = Qall[:nq]
        f8 = _index(Vb)
        bf = GpuIndex(torch.from_numpy(Vw).to(torch.bfloat16).cuda())
        try:
            bf.set_option("max_blocks", 8)
            bf.set_option("bf16_ks_min_q", 5)
            assert np.array_equal(bf.host_matrix(), Vw)   # a float8 code is a bf16 number
            for metric in metrics:
                mid = METRIC_IDS[metric]
                for exact in (False, True):
                    i1, s1, st1 = f8.topk_device(Q, k, mid, exact=exact)
                    i2, s2, st2 = bf.topk_device(Q, k, mid, exact=exact)
                    assert f8.stat("mfma") == 1 and bf.stat("mfma") == 1 and f8.stat("path") == bf.stat("path") == (2 if exact else 1), (d, metric, exact)
                    assert int(st1.abs().sum().item()) == 0 and int(st2.abs().sum().item()) == 0, (d, metric, exact)
                    assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32)), (d, metric, exact)
        finally:
            f8.close()
            bf.close()


# ------------------------------------------------------------------------------------------------
# 3. off by default; the threshold; few queries, manhattan, pearson
# ------------------------------------------------------------------------------------------------
def test_off_by_default_and_the_threshold(orc):
    from hyperdb._native import METRIC_IDS
    Vb, Vw, Qall, _, _ = _case(768, False)
    mid, k = METRIC_IDS["cosine_similarity"], 50
    ix = _index(Vb, min_q=None)
    try:
        ix.topk(Qall[:16], k, mid)                       # a fresh index: four VALU passes
        assert ix.stat("mfma") == 0 and ix.stat("path") == 1
        ix.set_option("f8_ks_min_q", 9)
        i8, s8 = ix.topk(Qall[:8], k, mid)
        assert ix.stat("mfma") == 0
        i9, s9 = ix.topk(Qall[:9], k, mid)
        assert ix.stat("mfma") == 1
        for qi in range(8):
            assert orc.same_result_modulo_ties(i8[qi], s8[qi], i9[qi], s9[qi], TOL), qi
        ix.set_option("f8_ks_min_q", 1)
        for nq in (1, 4):                                 # one VALU pass, whatever the option says
            ix.topk(Qall[:nq], k, mid)
            assert ix.stat("mfma") == 0 and ix.stat("fused") == 0, nq
        ix.set_option("f8_ks_min_q", 5)
        ix.topk(Qall[:16], k, METRIC_IDS["manhattan_distance"])
        assert ix.stat("mfma") == 0
        Q = Qall[:40]
        pid = METRIC_IDS["pearson_correlation"]
        pi, ps, pst = ix.topk_views(Q, k, pid)
        pi, ps = pi.copy(), ps.copy()
        assert ix.stat("mfma") == 1 and ix.stat("fused") == 0 and int(np.abs(pst).sum()) == 0
        ix.set_option("use_mfma", 0)
        vi, vs, _ = ix.topk_views(Q, k, pid)
        assert ix.stat("mfma") == 0
        for qi in range(40):
            assert orc.same_result_modulo_ties(pi[qi], ps[qi], vi[qi], vs[qi], TOL), qi
        for qi in (0, 1, 20, 39):
            orc.check_topk(pi[qi], ps[qi], Vw, Q[qi], "pearson_correlation", k, tol=TOL)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 4. a row mask; the full sort
# ------------------------------------------------------------------------------------------------
def test_row_mask_equals_valu(orc):
    from hyperdb._native import METRIC_IDS
    Vb, Vw, Qall, ts, _ = _case(1024, False)
    rng = np.random.default_rng(11)
    Q, k = Qall[:16], 40
    mask = (rng.random(N) < 0.02).astype(np.uint8)
    mask[:3] = 1
    ix = _index(Vb)
    try:
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


def test_full_sort_equals_valu(orc):
    from hyperdb._native import METRIC_IDS
    Vb, Vw, Qall, _, _ = _case(768, False)
    Q, k = Qall[:8], 2049
    ix = _index(Vb)
    try:
        mid = METRIC_IDS["cosine_similarity"]
        fi, fs = ix.topk(Q, k, mid)
        assert ix.stat("path") == 3
        ix.set_option("use_mfma", 0)
        vi, vs = ix.topk(Q, k, mid)
        assert ix.stat("path") == 3 and ix.stat("mfma") == 0
        for qi in range(8):
            assert orc.same_result_modulo_ties(fi[qi], fs[qi], vi[qi], vs[qi], TOL), qi
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 5. non-finite values are inputs, not faults
# ------------------------------------------------------------------------------------------------
def _plain(d):
    rng = np.random.default_rng(1000 * d)
    return _f8(rng.standard_normal((N, d)).astype(np.float32))


def test_nan_code_keeps_the_matrix_off_the_matrix_cores():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, _ = _plain(768)
    W = Vb.view(torch.uint8).clone()
    W[777, 500] = 0x7F                                   # (in the second slice)
    Q = np.random.default_rng(8).standard_normal((16, 768)).astype(np.float32)
    ix = GpuIndex(W.view(torch.float8_e4m3fn))
    try:
        ix.set_option("max_blocks", 8)
        ix.set_option("f8_ks_min_q", 5)
        assert ix.has_nan
        i1, s1, st = ix.topk_views(Q, 20, METRIC_IDS["dot_product"])
        i1, s1 = i1.copy(), s1.copy()
        assert ix.stat("mfma") == 0 and int(np.abs(st).sum()) == 0
        ix.set_option("use_mfma", 0)
        i2, s2, _ = ix.topk_views(Q, 20, METRIC_IDS["dot_product"])
        assert ix.stat("mfma") == 0
        assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
        assert not (i1 == 777).any()                      # NaN -> -inf: the row is never among the best
    finally:
        ix.close()


def test_infinite_query_elements_on_the_matrix_cores(orc):
    import torch
    from hyperdb._native import METRIC_IDS
    Vb, Vw = _plain(768)
    rng = np.random.default_rng(9)
    Q = rng.standard_normal((16, 768)).astype(np.float32)
    bad = list(range(0, 16, 2))
    cols = [11 + 97 * j for j in range(len(bad))]         # 11 .. 690: four of them in the second slice (column >= 384)
    assert sum(c >= 384 for c in cols) == 4 and max(cols) < 768
    for j, qi in enumerate(bad):
        Q[qi, cols[j]] = np.inf if j % 2 == 0 else -np.inf
    mid, k = METRIC_IDS["dot_product"], 20
    ix = _index(Vb)
    try:
        mi, ms, mst = ix.topk_views(Q, k, mid)           # (a list that overflowed is answered by the exact re-run inside the call)
        mi, ms, mst = mi.copy(), ms.copy(), mst.copy()
        assert int(np.abs(mst).sum()) == 0                # (the statistics are those of the re-run here: up to four queries, the VALU scan)
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
# 6. lifecycle and the facade
# ------------------------------------------------------------------------------------------------
def test_append_and_compact_equal_a_fresh_index():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 768
    Vb, Vw = _plain(d)
    rng = np.random.default_rng(12)
    extra32 = rng.standard_normal((3_001, d)).astype(np.float32)           # float32 rows: converted to float8 on the way in
    extra_b, extra_w = _f8(extra32)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    n0 = 9_000
    ix = GpuIndex(Vb.view(torch.uint8)[:n0].clone().view(torch.float8_e4m3fn))
    try:
        ix.set_option("f8_ks_min_q", 5)
        ix.append(extra32[:1])
        ix.append(extra32[1:])
        assert ix.n == n0 + 3_001 and ix.V.dtype == torch.float8_e4m3fn
        assert np.array_equal(ix.host_matrix()[n0:], extra_w)
        keep = np.flatnonzero(rng.random(ix.n) < 0.9)
        ix.compact(keep)
        assert ix.n == keep.size > 8192 and ix.V.dtype == torch.float8_e4m3fn
        whole = torch.cat([Vb.view(torch.uint8)[:n0], extra_b.view(torch.uint8)])
        fresh = GpuIndex(whole[torch.from_numpy(keep).cuda()].contiguous().view(torch.float8_e4m3fn))
        try:
            fresh.set_option("f8_ks_min_q", 5)
            assert np.array_equal(ix.host_matrix(), fresh.host_matrix())
            i1, s1 = ix.topk(Q, 30, METRIC_IDS["cosine_similarity"])
            m1 = ix.stat("mfma")
            i2, s2 = fresh.topk(Q, 30, METRIC_IDS["cosine_similarity"])
            assert m1 == 1 and fresh.stat("mfma") == 1
            assert np.array_equal(i1, i2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
        finally:
            fresh.close()
    finally:
        ix.close()


def test_facade_batch_equals_single_queries():
    import torch
    from hyperdb import HyperDB
    rng = np.random.default_rng(21)
    n, d = 9_001, 768
    V32 = rng.standard_normal((n, d)).astype(np.float32)
    docs = [{"id": i, "text": f"doc {i}"} for i in range(n)]
    Q = rng.standard_normal((8, d)).astype(np.float32)
    db = HyperDB(docs, V32, fp_precision="float8_e4m3fn")
    assert db._index.V.dtype == torch.float8_e4m3fn and db._index.dtype == 5
    plain = db.query_batch(Q, top_k=10)                  # the option is off: two VALU passes
    assert db._index.stat("mfma") == 0
    db._index.set_option("f8_ks_min_q", 5)                # ... and through the K slices
    batch = db.query_batch(Q, top_k=10)
    assert db._index.stat("mfma") == 1
    for qi in range(8):
        assert [(gd, gi) for gd, _, gi in plain[qi]] == [(gd, gi) for gd, _, gi in batch[qi]]
        one = db.query(Q[qi], top_k=10)
        assert db._index.stat("mfma") == 0
        assert len(batch[qi]) == len(one) == 10
        for (gd, gs, gi), (wd, ws, wi) in zip(batch[qi], one):
            assert gd == wd and gi == wi
            assert abs(float(gs) - float(ws)) <= TOL * max(1.0, abs(float(ws)))
