"""The opt-in int8 shadow (hdb_index_quantize, hdb_quant.hip): a quantized row scan whose survivors are rescored exactly.

The promise is bit identity: the top-k of a quantized call -- indices AND float32 score bits -- is the one the VALU scan gives
(hdb_scores + bias on the host, masked rows -inf, ordered by score descending then row ascending), and the one hdb_topk returns
with use_quant = 0, use_mfma = 0, use_fused = 0.  Every quantized case also checks that the filter was real: the call took the
path (stat "quant") and rescored between k and HDB_CAND_CAP rows.  The correctness tests set quant_min_n = 0 so that the path is
taken whatever the measured crossover is.
"""
import ctypes
import inspect

import numpy as np
import pytest

from hyperdb import _native
import hyperdb.ranking_algorithm as ranking
from hyperdb.hyperdb import HyperDB

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric")
CAP = 8192


# ---------------------------------------------------------------------------------------------- CPU (no GPU needed)
def test_library_exports_quantize():
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "hdb_index_quantize")
    assert "hdb_index_quantize" in _native.EXPORTS
    assert _native.lib().hdb_version() >= 101


def test_entry_points_accept_quantize():
    assert "quantize" in inspect.signature(ranking.register_vectors).parameters
    assert inspect.signature(ranking.register_vectors).parameters["quantize"].default is None
    assert "quantize" in inspect.signature(HyperDB.__init__).parameters
    assert inspect.signature(HyperDB.__init__).parameters["quantize"].default is None


def test_quantize_mode_validation():
    assert _native.quant_mode(None) == _native.HDB_QUANT_NONE
    assert _native.quant_mode("int8") == _native.HDB_QUANT_I8
    for bad in ("int4", "INT8", 8, True, ["int8"]):
        with pytest.raises(ValueError):
            _native.quant_mode(bad)
    with pytest.raises(ValueError):
        ranking.register_vectors(np.zeros((4, 8), np.float32), quantize="fp8")
    with pytest.raises(ValueError):
        HyperDB(quantize="int16")


# ---------------------------------------------------------------------------------------------- GPU helpers
def _torch():
    import torch
    return torch


def _matrix(n, d, dtype, seed):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(dtype)


def _queries(nq, d, seed):
    return np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)


def _reference(ix, Q, k, metric, bias=None, mask=None):
    """Top-k of the VALU scan: hdb_scores, bias added in float32, masked rows -inf, (score desc, row asc)."""
    torch = _torch()
    out_i, out_s = [], []
    for q in Q:
        s = ix.scores(q, M[metric]).clone()
        if bias is not None:
            s = s + bias
        s = torch.where(torch.isnan(s), torch.full_like(s, -float("inf")), s) + 0.0
        if mask is not None:
            s = torch.where(mask != 0, s, torch.full_like(s, -float("inf")))
        v, i = torch.sort(s, descending=True, stable=True)
        out_i.append(i[:k].cpu().numpy().astype(np.int64))
        out_s.append(v[:k].cpu().numpy().astype(np.float32))
    return np.stack(out_i), np.stack(out_s)


def _same(a_idx, a_sc, b_idx, b_sc):
    return np.array_equal(np.asarray(a_idx), np.asarray(b_idx)) and \
        np.array_equal(np.asarray(a_sc, np.float32).view(np.int32), np.asarray(b_sc, np.float32).view(np.int32))


def _quant_call(ix, Q, k, metric):
    """hdb_topk through the shadow: (idx, score, status) on the host, plus the filter's candidate count."""
    idx, sc, st = ix.topk_device(Q, k, M[metric])
    idx, sc, st = idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()
    return idx, sc, st, ix.stat("quant"), ix.stat("quant_cands")


def _plain_call(ix, Q, k, metric):
    ix.set_option("use_quant", 0)
    ix.set_option("use_mfma", 0)
    ix.set_option("use_fused", 0)
    try:
        idx, sc, st = ix.topk_device(Q, k, M[metric])
        return idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()
    finally:
        ix.set_option("use_quant", 1)
        ix.set_option("use_mfma", 1)
        ix.set_option("use_fused", 1)


def _quantized_index(V):
    ix = _native.GpuIndex(V)
    ix.quantize("int8")
    ix.set_option("quant_min_n", 0)
    return ix


def _check_case(ix, Q, k, metric, bias=None, mask=None, what=""):
    idx, sc, st, took, cands = _quant_call(ix, Q, k, metric)
    assert took == 1, f"{what}: the call did not take the int8 shadow"
    assert (st == 0).all(), f"{what}: status {st}"
    assert k <= cands <= CAP, f"{what}: {cands} candidates"
    ri, rs = _reference(ix, Q, k, metric, bias, mask)
    assert _same(idx, sc, ri, rs), f"{what}: differs from hdb_scores"
    pi, ps, pst = _plain_call(ix, Q, k, metric)
    assert (pst == 0).all() and _same(idx, sc, pi, ps), f"{what}: differs from the plain VALU top-k"
    return cands


SHAPES = [
    ("f16", 384, 20000), ("f16", 384, 1000000), ("f16", 768, 20000), ("f16", 300, 20000), ("f16", 300, 1000000),
    ("f32", 384, 20000), ("f32", 384, 1000000), ("f32", 768, 20000), ("f32", 100, 20000), ("f32", 100, 1000000),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,d,n", SHAPES, ids=[f"{a}-d{b}-n{c}" for a, b, c in SHAPES])
def test_bit_identity(dt, d, n):
    torch = _torch()
    V = _matrix(n, d, torch.float16 if dt == "f16" else torch.float32, seed=d + n)
    ix = _quantized_index(V)
    try:
        g = torch.Generator(device="cuda").manual_seed(7)
        bias = (torch.rand(n, generator=g, device="cuda") * 0.05).to(torch.float32)
        mask = (torch.rand(n, generator=g, device="cuda") < 0.05).to(torch.uint8)
        ks = (1, 10, 100, 128)
        case = 0
        for metric in METRICS:
            for variant in ("plain", "bias", "mask", "both"):
                nq = 1 + case % 4
                k = ks[(case // 4 + case) % 4]
                case += 1
                Q = _queries(nq, d, seed=case + d)
                b = bias if variant in ("bias", "both") else None
                m = mask if variant in ("mask", "both") else None
                if metric == "dot_product" and b is not None:
                    b = b * 20.0                          # (a bias on the scale of the dot products)
                ix.set_bias(b)
                ix.set_row_mask(m)
                _check_case(ix, Q, k, metric, b, m, what=f"{metric} {variant} nq={nq} k={k}")
                ix.set_bias(None)
                ix.set_row_mask(None)
    finally:
        ix.close()


@pytest.mark.gpu
def test_full_size_10m():
    torch = _torch()
    n, d = 10_000_000, 384
    V = _matrix(n, d, torch.float16, seed=11)
    ix = _quantized_index(V)
    try:
        Q = _queries(1, d, seed=3)
        cands = _check_case(ix, Q, 100, "cosine_similarity", what="10M x 384 fp16 cosine")
        print(f"10M x 384 fp16 cosine k=100: quant_cands = {cands}, shadow {ix.stat('quant_bytes') / 1e9:.2f} GB")
    finally:
        ix.close()
        del V
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- adversarial data
def _host_index(Vh, quant=True):
    ix = _native.GpuIndex(Vh)
    if quant:
        ix.quantize("int8")
        ix.set_option("quant_min_n", 0)
    return ix


@pytest.mark.gpu
def test_duplicates_straddling_kth():
    rng = np.random.default_rng(1)
    V = rng.standard_normal((50000, 384)).astype(np.float16)
    q = rng.standard_normal((1, 384)).astype(np.float32)
    k = 100
    order = np.argsort(-(V.astype(np.float32) @ q[0]), kind="stable")
    V[order[k - 3:k + 3]] = V[order[k - 3]]              # six identical rows around the k-th place ...
    V[[5, 49990]] = V[order[k - 3]]                      # ... and two more far apart (tie order = row order)
    ix = _host_index(V)
    try:
        for metric in METRICS:
            _check_case(ix, q, k, metric, what=f"duplicates {metric}")
    finally:
        ix.close()


@pytest.mark.gpu
def test_near_ties_below_int8_resolution():
    rng = np.random.default_rng(2)
    n, d = 40000, 384
    V = rng.standard_normal((n, d)).astype(np.float32)
    base = V[123].copy()
    s_r = np.abs(base).max() / 127.0
    rows = rng.choice(n, 300, replace=False)
    V[rows] = base + 1e-4 * s_r * rng.standard_normal((300, d)).astype(np.float32)
    q = (base + 0.01 * rng.standard_normal(d)).astype(np.float32).reshape(1, d)
    ix = _host_index(V)
    try:
        for metric in METRICS:
            idx, sc, st, took, cands = _quant_call(ix, q, 100, metric)
            ri, rs = _reference(ix, q, 100, metric)
            assert took == 1 and _same(idx, sc, ri, rs), metric
            # through the host entry point too (its exact re-run covers a failed floor check)
            hi, hs = ix.topk(q, 100, M[metric])
            assert _same(hi, hs, ri, rs), metric
    finally:
        ix.close()


@pytest.mark.gpu
def test_outlier_scaled_row_at_the_boundary():
    rng = np.random.default_rng(3)
    n, d, k = 30000, 384, 100
    V = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    q[5] = 0.0
    order = np.argsort(-(V @ q), kind="stable")
    j = 777
    V[j] = V[order[k - 1]]
    V[j, 5] = 400.0                                      # s_r is this one element: every other code rounds to ~0
    ix = _host_index(V)
    try:
        _check_case(ix, q.reshape(1, d), k, "dot_product", what="outlier dot")
        idx, sc, st, took, cands = _quant_call(ix, q.reshape(1, d), k, "dot_product")
        assert j in set(idx[0].tolist()) or order[k - 1] in set(idx[0].tolist())
        for metric in ("cosine_similarity", "euclidean_metric"):
            idx, sc, st, took, cands = _quant_call(ix, q.reshape(1, d), k, metric)
            ri, rs = _reference(ix, q.reshape(1, d), k, metric)
            assert took == 1 and _same(idx, sc, ri, rs), metric
    finally:
        ix.close()


@pytest.mark.gpu
def test_candidate_overflow_reruns_exactly():
    rng = np.random.default_rng(4)
    n, d = 20000, 384
    base = rng.standard_normal(d).astype(np.float32)
    V = (base + 1e-3 * rng.standard_normal((n, d))).astype(np.float32)      # near-identical rows: everything is a candidate
    q = rng.standard_normal((1, d)).astype(np.float32)
    ix = _host_index(V)
    try:
        idx, sc, st, took, cands = _quant_call(ix, q, 100, "cosine_similarity")
        assert took == 1
        assert st[0] & (_native.Q_OVERFLOW | _native.Q_UNDERFLOW), "the overflow must be reported on the device API"
        hi, hs = ix.topk(q, 100, M["cosine_similarity"])
        ri, rs = _reference(ix, q, 100, "cosine_similarity")
        assert _same(hi, hs, ri, rs)
    finally:
        ix.close()


@pytest.mark.gpu
def test_mask_keeping_fewer_than_k_rows():
    rng = np.random.default_rng(5)
    n, d = 30000, 384
    V = rng.standard_normal((n, d)).astype(np.float16)
    q = rng.standard_normal((2, d)).astype(np.float32)
    mask = np.zeros(n, np.uint8)
    mask[rng.choice(n, 50, replace=False)] = 1
    ix = _host_index(V)
    plain = _host_index(V, quant=False)
    try:
        ix.set_row_mask(mask)
        plain.set_row_mask(mask)
        hi, hs = ix.topk(q, 100, M["cosine_similarity"])
        pi, ps = plain.topk(q, 100, M["cosine_similarity"])
        assert _same(hi, hs, pi, ps)                     # today's answer: the kept rows first, then -inf entries
        keep = set(np.flatnonzero(mask).tolist())
        for r in range(2):
            assert set(hi[r, :50].tolist()) == keep and np.isfinite(hs[r, :50]).all()
            assert np.isneginf(hs[r, 50:]).all()
    finally:
        ix.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- lifecycle
@pytest.mark.gpu
def test_extend_finds_new_rows():
    rng = np.random.default_rng(6)
    n, d = 30000, 384
    V = rng.standard_normal((n, d)).astype(np.float16)
    q = rng.standard_normal((1, d)).astype(np.float32)
    ix = _host_index(V)
    try:
        _check_case(ix, q, 100, "cosine_similarity", what="before append")
        new = (q[0] + 0.05 * rng.standard_normal((40, d))).astype(np.float16)   # all belong in the top-k
        ix.append(new)
        idx, sc, st, took, cands = _quant_call(ix, q, 100, "cosine_similarity")
        assert set(range(n, n + 40)) <= set(idx[0].tolist())
        _check_case(ix, q, 100, "cosine_similarity", what="after append")
        ix.append(rng.standard_normal((5000, d)).astype(np.float16))         # a second append (capacity growth)
        _check_case(ix, q, 100, "euclidean_metric", what="after second append")
    finally:
        ix.close()


@pytest.mark.gpu
def test_compaction_and_update():
    rng = np.random.default_rng(7)
    n, d = 40000, 300
    V = rng.standard_normal((n, d)).astype(np.float16)
    q = rng.standard_normal((2, d)).astype(np.float32)
    ix = _host_index(V)
    try:
        keep = np.sort(rng.choice(n, 30000, replace=False))
        ix.compact(keep)
        _check_case(ix, q, 100, "cosine_similarity", what="after compaction")
        # a different matrix of the same shape: a stale shadow would filter by the old rows (status != 0 or wrong rows)
        ix.update(-ix.V.clone())
        _check_case(ix, q, 100, "cosine_similarity", what="after update (negated)")
        _check_case(ix, q, 100, "dot_product", what="after update (negated, dot)")
        ix.quantize(None)
        ix.topk_device(q, 100, M["cosine_similarity"])
        assert ix.stat("quant") == 0 and ix.stat("quant_bytes") == 0
    finally:
        ix.close()


@pytest.mark.gpu
def test_facade_remove_document_and_compaction():
    rng = np.random.default_rng(8)
    n, d = 24000, 128
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    docs = [f"doc {i}" for i in range(n)]
    db = HyperDB(docs, vecs, quantize="int8")
    ref = HyperDB(docs, vecs)
    try:
        db._index.set_option("quant_min_n", 0)
        for h in (ref._index,):
            h.set_option("use_mfma", 0)
            h.set_option("use_fused", 0)
        q = rng.standard_normal(d).astype(np.float32)
        assert db.query(q, top_k=50) == ref.query(q, top_k=50)
        assert db._index.stat("quant") == 1
        victims = list(range(0, 14000, 2))               # more than a quarter of the rows: tombstones, then a compaction
        for db_ in (db, ref):
            db_.remove_document(victims)
        assert db._index.n == ref._index.n
        db.clear_cache()
        ref.clear_cache()
        out, want = db.query(q, top_k=50), ref.query(q, top_k=50)
        assert out == want
        assert db._index.stat("quant") == 1
        more = rng.standard_normal((100, d)).astype(np.float32)
        db.add([f"new {i}" for i in range(100)], more)
        ref.add([f"new {i}" for i in range(100)], more)
        q2 = more[3] + 0.01
        assert db.query(q2, top_k=20, metric="dot_product") == ref.query(q2, top_k=20, metric="dot_product")
        assert db._index.stat("quant") == 1
    finally:
        db._index.close()
        ref._index.close()


# ---------------------------------------------------------------------------------------------- fallbacks
@pytest.mark.gpu
def test_infinite_element_declines_the_path():
    rng = np.random.default_rng(9)
    V = rng.standard_normal((20000, 384)).astype(np.float32)
    V[77, 3] = np.inf
    q = rng.standard_normal((1, 384)).astype(np.float32)
    ix = _host_index(V)
    plain = _host_index(V, quant=False)
    try:
        hi, hs = ix.topk(q, 50, M["dot_product"])
        assert ix.stat("quant") == 0
        pi, ps = plain.topk(q, 50, M["dot_product"])
        assert _same(hi, hs, pi, ps)
    finally:
        ix.close()
        plain.close()


@pytest.mark.gpu
def test_nan_query_raises():
    rng = np.random.default_rng(10)
    V = rng.standard_normal((20000, 384)).astype(np.float16)
    q = rng.standard_normal((1, 384)).astype(np.float32)
    q[0, 9] = np.nan
    ix = _host_index(V)
    try:
        with pytest.raises(ValueError):
            ix.topk(q, 10, M["cosine_similarity"])
    finally:
        ix.close()


@pytest.mark.gpu
def test_float64_index_is_unsupported():
    V = np.random.default_rng(11).standard_normal((1000, 64))
    ix = _native.GpuIndex(V)
    try:
        rc = _native.lib().hdb_index_quantize(ix._h, _native.HDB_QUANT_I8, None)
        assert rc == -3                                  # HDB_ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            ix.quantize("int8")
        with pytest.raises(ValueError):
            ix.quantize("int3")
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------- facade and group
@pytest.mark.gpu
def test_facade_and_group_match():
    torch = _torch()
    rng = np.random.default_rng(12)
    n, d = 20000, 384
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    docs = [{"id": i} for i in range(n)]
    db = HyperDB(docs, vecs, quantize="int8")
    ref = HyperDB(docs, vecs)
    try:
        db._index.set_option("quant_min_n", 0)
        ref._index.set_option("use_mfma", 0)
        ref._index.set_option("use_fused", 0)
        for metric in METRICS:
            q = rng.standard_normal(d).astype(np.float32)
            assert db.query(q, top_k=25, metric=metric) == ref.query(q, top_k=25, metric=metric), metric
            assert db._index.stat("quant") == 1
    finally:
        db._index.close()
        ref._index.close()
    # two shards on device 0 against the single quantized index
    one = _native.GpuIndex(vecs)
    grp = ranking.register_vectors(vecs, devices=[0, 0], quantize="int8")
    try:
        one.quantize("int8")
        one.set_option("quant_min_n", 0)
        grp.index.set_option("quant_min_n", 0)
        Q = rng.standard_normal((3, d)).astype(np.float32)
        for metric in METRICS:
            gi, gs = grp.index.topk(Q, 40, M[metric])
            assert grp.index.stat("quant") == 1
            oi, os_ = one.topk(Q, 40, M[metric])
            assert _same(gi, gs, oi, os_), metric
        # the drop-in entry point on the registered handle
        idx, sc = ranking.hyperDB_ranking_algorithm_sort(grp, Q[0], top_k=40, metric="cosine_similarity")
        oi, os_ = one.topk(Q[:1], 40, M["cosine_similarity"])
        assert list(idx) == list(oi[0]) and np.array_equal(np.asarray(sc, np.float64), os_[0].astype(np.float64))
    finally:
        one.close()
        grp.close()
        torch.cuda.empty_cache()
