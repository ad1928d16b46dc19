"""Range search on the GPU (hdb_range_host / hdb_range_fetch): every row at or above a per-query threshold, as CSR.

Integer data (|x| <= 2, d = 32, dot product, integer bias) score exactly in every arithmetic of the library: EQUALITY with the numpy
model of the contract (_native.range_host).  Float data: the project's bands against the float64 model, thresholds inside a gap."""
import ctypes

import numpy as np
import pytest
from test_maxsim import _make_index          # (matrix, storage name) -> GpuIndex

pytestmark = pytest.mark.gpu

D = 32
_cache = {}


def _int_case(n, nq, bits):
    """-> (V, Q, bias, mask, thresholds, {sort: the model's answer}), once per shape.  Thresholds by query: -inf, the largest score
    several rows share (inclusive >=, ties in row order), a value about 1 % of the rows pass, one above the maximum (empty).  Two
    chunks (nq = 257): -inf goes to the last query only, so its segment outgrows the room the first chunk left: the buffer grows."""
    from hyperdb._native import range_host
    key = (n, nq, bits)
    if key not in _cache:
        rng = np.random.default_rng(1000 * n + nq)
        V = rng.integers(-2, 3, size=(n, D)).astype(np.int64)
        Q = rng.integers(-2, 3, size=(nq, D)).astype(np.int64)
        bias = rng.integers(0, 4, size=n).astype(np.float32) if n >= 3 else None
        mask = (rng.random(n) < 0.9).astype(np.uint8) if n >= 3 else None
        M = (V > 0).astype(np.int64) if bits else V
        S = (Q @ M.T).astype(np.float64) + (0 if bias is None else bias)
        thr = np.empty(nq, np.float32)
        for q in range(nq):
            kind = q % 4
            if nq == 257:
                kind = 0 if q == 256 else (3 if kind == 0 else kind)
            s = np.sort(S[q][mask != 0] if mask is not None else S[q])[::-1]
            if kind == 0 or s.size == 0:
                thr[q] = -np.inf
            elif kind == 1:
                vals, counts = np.unique(s, return_counts=True)
                thr[q] = vals[counts >= 2].max() if (counts >= 2).any() else s[0]
            elif kind == 2:
                thr[q] = s[min(s.size - 1, s.size // 100)] + 0.5
            else:
                thr[q] = s[0] + 1.0
        want = {sort: range_host(M, Q, thr, "dot_product", bias=bias, mask=mask, sort=sort) for sort in (False, True)}
        _cache[key] = (V, Q.astype(np.float32), bias, mask, thr, want)
    return _cache[key]


@pytest.mark.parametrize("nq", [1, 4, 5, 257])
@pytest.mark.parametrize("n", [1, 3, 4095, 4096, 4097, 8195])
@pytest.mark.parametrize("storage", ["float32", "float16", "bfloat16", "int8", "bits"])
def test_integer_data_equal_the_model(storage, n, nq):
    """lims, idx and scores equal the model for both orders, on every storage, at the tile edges and an n that is no multiple of 4,
    through the VALU scan, the matrix cores and two chunks; mask and bias are set from three rows on."""
    from hyperdb._native import METRIC_IDS
    V, Q, bias, mask, thr, want = _int_case(n, nq, storage == "bits")
    ix = _make_index(V, storage)
    try:
        ix.set_bias(bias)
        ix.set_row_mask(mask)
        for sort in (False, True):
            lims, idx, sc = ix.range(Q, thr, METRIC_IDS["dot_product"], sort=sort)
            wl, wi, ws = want[sort]
            assert np.array_equal(lims, wl), (sort, np.flatnonzero(lims != wl)[:4].tolist())
            assert np.array_equal(idx, wi), (sort, np.flatnonzero(idx != wi)[:4].tolist())
            assert np.array_equal(sc.astype(np.float64), ws), sort
            assert (ix.stat("range"), ix.stat("range_total"), ix.stat("range_chunks"), ix.stat("range_long"), ix.stat("path")) == \
                   (1, int(wl[-1]), 2 if nq == 257 else 1, 0, 2)
    finally:
        ix.close()


@pytest.mark.parametrize("eligible", [8192, 8193, 8195])
def test_the_sort_boundary(eligible):
    """One query at -inf over 8195 rows of which a mask keeps `eligible`: a segment of HDB_RANGE_LDS_SORT = 8192 entries is the last
    one the LDS sort takes, 8193 and 8195 take the long sort; the answer is the model's either way."""
    from hyperdb._native import GpuIndex, METRIC_IDS, range_host
    rng = np.random.default_rng(eligible)
    V = rng.integers(-2, 3, size=(8195, D)).astype(np.float32)
    Q = rng.integers(-2, 3, size=(1, D)).astype(np.float32)
    mask = np.ones(8195, np.uint8)
    mask[rng.permutation(8195)[:8195 - eligible]] = 0
    ix = GpuIndex(V)
    try:
        ix.set_row_mask(mask)
        lims, idx, sc = ix.range(Q, -np.inf, METRIC_IDS["dot_product"])
        wl, wi, ws = range_host(V, Q, -np.inf, "dot_product", mask=mask)
        assert lims.tolist() == [0, eligible] and np.array_equal(idx, wi) and np.array_equal(sc.astype(np.float64), ws)
        assert ix.stat("range_long") == (1 if eligible > 8192 else 0)
    finally:
        ix.close()


def _float_case(nq):
    """Gaussian rows, n = 3000; per query 30 noisy copies of it at growing distance: a wide gap in the scores near the 99th percentile."""
    if ("float", nq) not in _cache:
        rng = np.random.default_rng(77 + nq)
        V = rng.standard_normal((3000, D))
        Q = rng.standard_normal((nq, D))
        for q in range(nq):
            V[100 * q + 10:100 * q + 40] = Q[q] + rng.standard_normal((30, D)) * np.linspace(0.05, 0.6, 30)[:, None]
        _cache[("float", nq)] = (V.astype(np.float32), Q.astype(np.float32))
    return _cache[("float", nq)]


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("metric", ["cosine_similarity", "euclidean_metric", "manhattan_distance", "pearson_correlation"])
def test_float_data_against_float64(metric, dtype, nq):
    """Each query's threshold is the midpoint of the widest gap between consecutive float64 scores of ranks 20 .. 40 (the 99th
    percentile of 3000 rows is rank 30).  The gap exceeds twice the tolerance -- asserted before any GPU call -- so the band around the
    threshold is empty: the returned set IS the reference set, every score within tolerance, the order non-increasing with rows
    ascending among equal float32 scores."""
    from hyperdb._native import GpuIndex, METRIC_IDS, range_host, _host_scores
    V32, Q = _float_case(nq)
    V = V32.astype(dtype)
    thr = np.empty(nq, np.float64)
    tol_of = (lambda s: 1e-3) if dtype == np.float16 else (lambda s: 1e-5 * max(1.0, abs(s)))
    for q in range(nq):
        s = np.sort(_host_scores(V, Q[q], metric))[::-1][20:41]
        g = int(np.argmax(s[:-1] - s[1:]))
        thr[q] = 0.5 * (s[g] + s[g + 1])
        assert s[g] - s[g + 1] > 2 * tol_of(thr[q]), (q, s[g] - s[g + 1])
    wl, wi, ws = range_host(V, Q, thr, metric)
    ix = GpuIndex(V)
    try:
        lims, idx, sc = ix.range(Q, thr, METRIC_IDS[metric])
    finally:
        ix.close()
    assert np.array_equal(lims, wl)
    for q in range(nq):
        a, b = int(lims[q]), int(lims[q + 1])
        assert 20 < b - a <= 40
        assert set(idx[a:b].tolist()) == set(wi[a:b].tolist()), q
        ref = dict(zip(wi[a:b].tolist(), ws[a:b].tolist()))
        for r, s in zip(idx[a:b].tolist(), sc[a:b].tolist()):
            assert abs(s - ref[r]) <= tol_of(ref[r]), (q, r, s, ref[r])
        s32, rows = sc[a:b], idx[a:b]
        assert (s32[1:] <= s32[:-1]).all() and (rows[1:][s32[1:] == s32[:-1]] > rows[:-1][s32[1:] == s32[:-1]]).all()


@pytest.mark.parametrize("nq", [4, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("metric,use_mfma", [("dot_product", 1), ("cosine_similarity", 1), ("euclidean_metric", 0)])
def test_score_bits_are_those_of_topk_exact(metric, use_mfma, dtype, nq):
    """9000 Gaussian rows (above 8192: five queries take the matrix cores): each query's segment equals, in indices and float32
    bits, the first `count` entries of hdb_topk_exact of the same batch at k = count."""
    from hyperdb._native import GpuIndex, METRIC_IDS, _host_scores
    rng = np.random.default_rng(5 + nq)
    V = rng.standard_normal((9000, D)).astype(dtype)
    Q = rng.standard_normal((nq, D)).astype(np.float32)
    thr = np.empty(nq)
    for q in range(nq):
        s = np.sort(_host_scores(V, Q[q], metric))[::-1]
        thr[q] = 0.5 * (s[20 + 300 * q] + s[21 + 300 * q])        # about 21, 321, .. 1221 rows pass
    ix = GpuIndex(V)
    try:
        ix.set_option("use_mfma", use_mfma)
        lims, idx, sc = ix.range(Q, thr, METRIC_IDS[metric])
        assert ix.stat("mfma") == (1 if use_mfma and nq == 5 else 0)
        for q in range(nq):
            a, b = int(lims[q]), int(lims[q + 1])
            assert 1 <= b - a <= 2048
            ti, ts, _ = ix.topk_device(Q, b - a, METRIC_IDS[metric], exact=True)
            assert np.array_equal(idx[a:b], ti[q].cpu().numpy()), q
            assert np.array_equal(sc[a:b].view(np.uint32), ts[q].cpu().numpy().view(np.uint32)), q
    finally:
        ix.close()


def test_edges():
    """A row whose score is NaN is never returned; a NaN query raises ValueError; a budget below the need fails with the total in the
    message and the next call with the budget restored is correct; append invalidates the fetch; HyperDB.query_range with a metadata
    filter returns the documents query(top_k = size) returns above the threshold."""
    from hyperdb import HyperDB, _native
    from hyperdb._native import GpuIndex, HyperDBNativeError, METRIC_IDS, range_host
    rng = np.random.default_rng(3)
    V = rng.integers(-2, 3, size=(500, D)).astype(np.float32)
    V[7, 3] = np.nan
    Q = rng.integers(-2, 3, size=(2, D)).astype(np.float32)
    want = range_host(V, Q, -np.inf, "dot_product")
    ix = GpuIndex(V)
    try:
        lims, idx, sc = ix.range(Q, -np.inf, METRIC_IDS["dot_product"])
        assert lims.tolist() == [0, 499, 998] and 7 not in idx.tolist()
        assert np.array_equal(idx, want[1]) and np.array_equal(sc.astype(np.float64), want[2])
        bad = Q.copy()
        bad[1, 0] = np.nan
        with pytest.raises(ValueError):
            ix.range(bad, 0.0, METRIC_IDS["dot_product"])
        ix.set_option("range_bytes", 998 * 20 - 1)
        with pytest.raises((MemoryError, HyperDBNativeError), match="998 results"):
            ix.range(Q, -np.inf, METRIC_IDS["dot_product"])
        ix.set_option("range_bytes", 998 * 20)
        lims, idx, sc = ix.range(Q, -np.inf, METRIC_IDS["dot_product"])
        assert np.array_equal(lims, want[0]) and np.array_equal(idx, want[1]) and np.array_equal(sc.astype(np.float64), want[2])
        out_i, out_s = np.empty(998, np.int64), np.empty(998, np.float32)
        fetch = lambda: _native.lib().hdb_range_fetch(ix._h, out_i.ctypes.data_as(ctypes.c_void_p), out_s.ctypes.data_as(ctypes.c_void_p))
        assert fetch() == 0 and np.array_equal(out_i, idx)
        ix.append(V[:3])
        assert fetch() == -1
    finally:
        ix.close()
    Vd = rng.integers(-2, 3, size=(300, D)).astype(np.float32)
    docs = [{"name": f"d{i}", "kind": "a" if i % 3 else "b"} for i in range(300)]
    db = HyperDB(documents=docs, vectors=Vd, metadata_keys=["kind"])
    q = rng.integers(-2, 3, size=D).astype(np.float32)
    filters = [("metadata", {"kind": "a"})]
    full = db.query(q, top_k=200, filters=filters, metric="dot_product")          # (the filter keeps 200 of the 300 documents)
    cut = float(full[30][1])                                      # (inclusive: every document tied with the 31st comes back)
    res = db.query_range(q, cut, filters=filters, metric="dot_product")
    assert res == [(doc, s) for doc, s, _ in full if s >= cut] and len(res) >= 31
    assert db.query_range(q, cut, filters=filters, metric="dot_product", return_similarities=False) == [doc for doc, _ in res]
