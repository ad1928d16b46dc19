"""GPU tests (-m gpu) of the opt-in int8 shadow of a bfloat16 index (option bf16_quant, hdb_quant.hip "bfloat16 rows").

The promise is the explicit shadow's, bit identity: the top-k of a 1-4-query dot / cosine / euclidean call through the shadow --
indices AND float32 score bits -- is the one the VALU scan gives (hdb_scores + bias on the host, masked rows -inf, ordered by score
descending then row ascending) and the one the SAME handle returns with use_quant = 0 and every other option at its default: a
default bfloat16 index answers 1-4 queries on the VALU scan, so the shadow returns the bits of the default path.  Every case checks
that the filter was real: the call took the path (stat "quant") and rescored between k and HDB_CAND_CAP rows.

Shapes are the smallest at which each code path exists (the shadow needs more than HDB_CAND_CAP = 8192 rows): N = 20 003 has a ragged
last tile; d = 128 is one 256-byte step, 384 three unrolled steps, 200 a runtime loop with dead pieces (25 pieces), 100 the
generic non-vector kernel (200-byte rows), 520 has no plane.  Every index is built with bf16_quant = 1, quantize("int8"),
quant_min_n = 0 and plane_min_n = 0 on Gaussian data rounded to bfloat16.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ("dot_product", "cosine_similarity", "euclidean_metric")
CAP = 8192
N = 20_003


def _native():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hyperdb import _native
    return _native


def _bf16(a32):
    """float32 array -> (bf16 CUDA tensor, its exact float32 widening on the host)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.bfloat16)
    return t.cuda(), t.float().numpy()


_MATS = {}


def _matrix(d, n=N):
    """One (bf16 device tensor, widened host matrix) per shape, shared by the tests and never modified."""
    if (d, n) not in _MATS:
        rng = np.random.default_rng(1000 * d + n)
        _MATS[(d, n)] = _bf16(rng.standard_normal((n, d)).astype(np.float32))
    return _MATS[(d, n)]


def _queries(nq, d, seed):
    return np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)


def _shadow_index(V, plane=True):
    nat = _native()
    ix = nat.GpuIndex(V)
    ix.set_option("bf16_quant", 1)
    if not plane:
        ix.set_option("use_plane", 0)
    ix.quantize("int8")
    ix.set_option("quant_min_n", 0)
    ix.set_option("plane_min_n", 0)
    return ix


def _reference(ix, Q, k, metric, bias=None, mask=None):
    """Top-k of the VALU scan: hdb_scores, bias added in float32, masked rows -inf, (score desc, row asc)."""
    import torch
    M = _native().METRIC_IDS
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


def _device_call(ix, Q, k, metric):
    M = _native().METRIC_IDS
    idx, sc, st = ix.topk_device(Q, k, M[metric])
    return idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()


def _default_call(ix, Q, k, metric):
    """The same handle without its shadow, every other option at its default: the default bfloat16 path."""
    ix.set_option("use_quant", 0)
    try:
        out = _device_call(ix, Q, k, metric)
        assert ix.stat("quant") == 0
        return out
    finally:
        ix.set_option("use_quant", 1)


def _check_case(ix, Q, k, metric, ref, what, plane_expected=None):
    """ref: (indices, scores) of _reference for these queries at some k' >= k (a prefix is the top-k)."""
    idx, sc, st = _device_call(ix, Q, k, metric)
    took, cands, plane = ix.stat("quant"), ix.stat("quant_cands"), ix.stat("plane")
    assert took == 1, f"{what}: the call did not take the int8 shadow"
    assert ix.stat("mfma") == 0 and ix.stat("fused") == 0 and ix.stat("path") == 1, what
    assert (st == 0).all(), f"{what}: status {st}"
    assert k <= cands <= CAP, f"{what}: {cands} candidates"
    assert _same(idx, sc, ref[0][:, :k], ref[1][:, :k]), f"{what}: differs from hdb_scores"
    if plane_expected is not None:
        assert plane == (1 if plane_expected else 0), f"{what}: plane {plane}"
        if plane_expected:
            surv = ix.stat("plane_survivors")
            assert surv >= cands, f"{what}: {surv} plane survivors, {cands} candidates"
            ix.set_option("use_plane", 0)
            try:
                oi, os_, ost = _device_call(ix, Q, k, metric)
                assert ix.stat("quant") == 1 and ix.stat("plane") == 0
                assert (ost == 0).all() and _same(idx, sc, oi, os_), f"{what}: differs with use_plane = 0"
            finally:
                ix.set_option("use_plane", 1)
    pi, ps, pst = _default_call(ix, Q, k, metric)
    assert (pst == 0).all() and _same(idx, sc, pi, ps), f"{what}: differs from the default bfloat16 path"
    return cands


# ------------------------------------------------------------------------------------------------
# 1. bit identity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (128, 384, 200, 100, 520))
def test_bit_identity(d):
    import torch
    Vb, _ = _matrix(d)
    ix = _shadow_index(Vb)
    try:
        assert ix.stat("quant_bytes") == N * ((d + 15) // 16 * 16 + 12)
        assert (ix.stat("plane_bytes") > 0) == (d <= 512)
        g = torch.Generator(device="cuda").manual_seed(7)
        bias = (torch.rand(N, generator=g, device="cuda") * 0.05).to(torch.float32)
        mask = (torch.rand(N, generator=g, device="cuda") < 0.5).to(torch.uint8)
        Q4 = _queries(4, d, seed=d + 1)
        for metric in METRICS:
            for variant in ("plain", "bias", "mask", "both"):
                b = bias if variant in ("bias", "both") else None
                m = mask if variant in ("mask", "both") else None
                if metric == "dot_product" and b is not None:
                    b = b * 20.0                          # (a bias on the scale of the dot products)
                ix.set_bias(b)
                ix.set_row_mask(m)
                ref = _reference(ix, Q4, 128, metric, b, m)          # once per setting: every (nq, k) below is a prefix of it
                for nq in (1, 2, 3, 4):
                    for k in (1, 10, 100, 128):
                        plane = nq == 1 and metric != "euclidean_metric" and d <= 512
                        _check_case(ix, Q4[:nq], k, metric, (ref[0][:nq], ref[1][:nq]), f"d={d} {metric} {variant} nq={nq} k={k}",
                                    plane_expected=plane)
                ix.set_bias(None)
                ix.set_row_mask(None)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 2. the bounds are sound
# ------------------------------------------------------------------------------------------------
def test_bounds_are_sound():
    nat = _native()
    M = nat.METRIC_IDS
    Vb, _ = _matrix(384)
    ix = _shadow_index(Vb)
    try:
        q = _queries(1, 384, seed=5)[0]
        mask = (np.random.default_rng(6).random(N) < 0.5).astype(np.uint8)
        for metric in ("dot_product", "cosine_similarity"):
            exact = ix.scores(q, M[metric]).cpu().numpy()
            hi, hi5 = ix.quant_bounds(q, M[metric])
            assert not np.isnan(hi).any() and not np.isnan(hi5).any()
            assert (hi5 >= hi).all(), f"{metric}: hi5 < hi at rows {np.flatnonzero(hi5 < hi)[:8]}"
            assert (hi >= exact).all(), f"{metric}: hi below the exact score at rows {np.flatnonzero(hi < exact)[:8]}"
            ix.set_row_mask(mask)
            hi, hi5 = ix.quant_bounds(q, M[metric])
            assert np.isneginf(hi[mask == 0]).all() and np.isneginf(hi5[mask == 0]).all()
            assert (hi5[mask != 0] >= hi[mask != 0]).all() and (hi[mask != 0] >= exact[mask != 0]).all()
            ix.set_row_mask(None)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 3. adversarial data (bfloat16 values)
# ------------------------------------------------------------------------------------------------
def test_duplicates_straddling_kth():
    rng = np.random.default_rng(1)
    _, Vw = _bf16(rng.standard_normal((50_000, 384)).astype(np.float32))
    q = rng.standard_normal((1, 384)).astype(np.float32)
    k = 100
    order = np.argsort(-(Vw @ q[0]), kind="stable")
    Vw[order[k - 3:k + 3]] = Vw[order[k - 3]]            # six identical rows around the k-th place ...
    Vw[[5, 49_990]] = Vw[order[k - 3]]                   # ... and two more far apart (tie order = row order)
    Vb, _ = _bf16(Vw)
    ix = _shadow_index(Vb)
    try:
        for metric in METRICS:
            _check_case(ix, q, k, metric, _reference(ix, q, k, metric), f"duplicates {metric}")
    finally:
        ix.close()


def test_near_ties_below_int8_resolution():
    """300 rows that differ from one row by one bfloat16 ulp in a few elements: a bfloat16 ulp of an element is at most 2^-8 of its
    magnitude, the int8 step of the row 2^-7 of its largest one, so the codes cannot tell most of them apart."""
    import torch
    nat = _native()
    M = nat.METRIC_IDS
    rng = np.random.default_rng(2)
    n, d = 40_000, 384
    Vb, Vw = _bf16(rng.standard_normal((n, d)).astype(np.float32))
    bits = Vb.cpu().view(torch.int16).numpy().copy()
    rows = rng.choice(n, 300, replace=False)
    near = np.repeat(bits[123][None, :], 300, axis=0)
    for r in range(300):
        cols = rng.choice(d, 8, replace=False)
        near[r, cols] += rng.choice(np.array([-1, 1], np.int16), 8)          # one ulp up or down (no element is near 0 or the type's end)
    bits[rows] = near
    Vb = torch.from_numpy(bits).view(torch.bfloat16).cuda()
    base = Vb[123].float().cpu().numpy()
    assert np.isfinite(Vb.float().cpu().numpy()).all()
    q = (base + 0.01 * rng.standard_normal(d)).astype(np.float32).reshape(1, d)
    ix = _shadow_index(Vb)
    try:
        for metric in METRICS:
            idx, sc, st = _device_call(ix, q, 100, metric)
            ri, rs = _reference(ix, q, 100, metric)
            assert ix.stat("quant") == 1 and _same(idx, sc, ri, rs), metric
            # through the host entry point too (its exact re-run covers a failed floor check)
            hi, hs = ix.topk(q, 100, M[metric])
            assert _same(hi, hs, ri, rs), metric
    finally:
        ix.close()


def test_candidate_overflow_reruns_exactly():
    nat = _native()
    M = nat.METRIC_IDS
    rng = np.random.default_rng(4)
    n, d = 20_000, 384
    base = rng.standard_normal(d).astype(np.float32)
    Vb, _ = _bf16((base + 1e-3 * rng.standard_normal((n, d))).astype(np.float32))      # near-identical rows: everything is a candidate
    q = rng.standard_normal((1, d)).astype(np.float32)
    ix = _shadow_index(Vb)
    try:
        idx, sc, st = _device_call(ix, q, 100, "cosine_similarity")
        assert ix.stat("quant") == 1
        assert int(st[0]) & (nat.Q_OVERFLOW | nat.Q_UNDERFLOW), f"status {st}: the overflow must be reported on the device API"
        hi, hs = ix.topk(q, 100, M["cosine_similarity"])
        ri, rs = _reference(ix, q, 100, "cosine_similarity")
        assert _same(hi, hs, ri, rs)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 4. matrices that are not finite
# ------------------------------------------------------------------------------------------------
def test_infinite_row_declines_the_shadow():
    nat = _native()
    M = nat.METRIC_IDS
    Vb, _ = _matrix(384)
    Wb = Vb.clone()
    Wb[77, 3] = float("inf")
    q = _queries(1, 384, seed=9)
    ix = _shadow_index(Wb)
    plain = nat.GpuIndex(Wb)
    try:
        hi, hs = ix.topk(q, 50, M["dot_product"])
        assert ix.stat("quant") == 0
        pi, ps = plain.topk(q, 50, M["dot_product"])
        assert _same(hi, hs, pi, ps)
    finally:
        ix.close()
        plain.close()


def test_nan_row_raises_as_without_a_shadow():
    nat = _native()
    M = nat.METRIC_IDS
    Vb, _ = _matrix(384)
    Wb = Vb.clone()
    Wb[4321, 17] = float("nan")
    import hyperdb.ranking_algorithm as ranking
    q = _queries(1, 384, seed=10)
    # the ranking entry points refuse a matrix that holds a NaN (the reference's ValueError), with a shadow as without one
    reg = ranking.register_vectors(Wb, quantize="int8")
    ref = ranking.register_vectors(Wb)
    try:
        reg.index.set_option("quant_min_n", 0)
        for h in (ref, reg):
            with pytest.raises(ValueError, match="NaN"):
                ranking.hyperDB_ranking_algorithm_sort(h, q[0].copy(), top_k=10, metric="cosine_similarity")
            with pytest.raises(ValueError, match="NaN"):
                ranking.rank_batch(h, np.repeat(q, 3, axis=0), top_k=10, metric="cosine_similarity")
    finally:
        reg.close()
        ref.close()
    # the library itself ranks a NaN score as -inf: the shadow is declined (finite()) and the answer is the shadowless index's
    ix = _shadow_index(Wb)
    plain = nat.GpuIndex(Wb)
    try:
        hi, hs = ix.topk(q, 10, M["cosine_similarity"])
        assert ix.stat("quant") == 0
        pi, ps = plain.topk(q, 10, M["cosine_similarity"])
        assert _same(hi, hs, pi, ps)
    finally:
        ix.close()
        plain.close()


# ------------------------------------------------------------------------------------------------
# 5. lifecycle
# ------------------------------------------------------------------------------------------------
def test_lifecycle_keeps_the_shadow_current():
    import torch
    nat = _native()
    M = nat.METRIC_IDS
    d, n0 = 128, 20_000
    rng = np.random.default_rng(12)
    Vb, _ = _bf16(rng.standard_normal((n0, d)).astype(np.float32))
    Q = rng.standard_normal((4, d)).astype(np.float32)
    extra32 = rng.standard_normal((3_001, d)).astype(np.float32)           # float32 rows: rounded to bf16 on the way in
    extra32[1_500] = 3.0 * Q[0]                                            # the best match of query 0, dot and cosine
    extra_b, _ = _bf16(extra32)
    ix = _shadow_index(Vb.clone())

    def check(rows_b, what):
        """The shadow call on ix against a fresh bfloat16 index without a shadow over the same rows."""
        assert ix.n == rows_b.shape[0] and ix.stat("quant_bytes") == ix.n * (d + 12), what
        fresh = nat.GpuIndex(rows_b.contiguous())
        try:
            for metric in METRICS:
                for nq in (1, 4):
                    gi, gs, gst = _device_call(ix, Q[:nq], 30, metric)
                    assert ix.stat("quant") == 1 and (gst == 0).all(), (what, metric, nq)
                    assert 30 <= ix.stat("quant_cands") <= CAP, (what, metric, nq)
                    if nq == 1 and metric != "euclidean_metric":
                        assert ix.stat("plane") == 1, (what, metric)
                    fi, fs, fst = _device_call(fresh, Q[:nq], 30, metric)
                    assert fresh.stat("quant") == 0 and (fst == 0).all()
                    assert _same(gi, gs, fi, fs), (what, metric, nq)
        finally:
            fresh.close()

    try:
        check(Vb, "built")
        ix.append(extra32[:1])
        ix.append(extra32[1:])
        assert ix.V.dtype == torch.bfloat16
        all_b = torch.cat([Vb, extra_b])
        check(all_b, "after append")
        for metric in ("dot_product", "cosine_similarity"):
            gi, _, _ = _device_call(ix, Q[:1], 30, metric)
            assert ix.stat("quant") == 1 and gi[0, 0] == n0 + 1_500, metric
        keep = np.flatnonzero(rng.random(ix.n) < 0.9)
        keep = np.union1d(keep, [n0 + 1_500])
        ix.compact(keep)
        kept_b = all_b[torch.from_numpy(keep).cuda()]
        check(kept_b, "after compact")
        gi, _, _ = _device_call(ix, Q[:1], 30, "cosine_similarity")
        assert gi[0, 0] == int(np.searchsorted(keep, n0 + 1_500))
        new32 = rng.standard_normal((15_001, d)).astype(np.float32)
        new_b, _ = _bf16(new32)
        ix.update(torch.from_numpy(new32).cuda())                          # float32 data into a bf16 index: rounded the same way
        check(new_b, "after update")
        ix.quantize(None)
        _device_call(ix, Q[:1], 30, "cosine_similarity")
        assert ix.stat("quant") == 0 and ix.stat("quant_bytes") == 0 and ix.stat("plane_bytes") == 0
        ix.quantize("int8")                                                # (bf16_quant is still set on the handle)
        check(new_b, "built again")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 6. the default stays pinned
# ------------------------------------------------------------------------------------------------
def test_without_the_option_nothing_changes():
    import torch
    nat = _native()
    M = nat.METRIC_IDS
    Vb, _ = _matrix(128)
    q = _queries(1, 128, seed=3)
    ix = nat.GpuIndex(Vb[:20_000].clone())
    try:
        with pytest.raises(NotImplementedError, match="bf16"):
            ix.quantize("int8")
        assert ix.stat("quant_bytes") == 0
        # the option alone builds nothing: no automatic shadow for bfloat16
        ix.set_option("bf16_quant", 1)
        ix.set_option("quant_min_n", 0)
        ix.topk(q, 30, M["cosine_similarity"])
        assert ix.stat("quant_auto") == 0 and ix.stat("quant") == 0 and ix.stat("quant_bytes") == 0
        ix.set_option("bf16_quant", 0)
        with pytest.raises(NotImplementedError, match="bf16"):
            ix.quantize("int8")
    finally:
        ix.close()
    f8 = nat.GpuIndex(nat.to_f8(Vb[:1_000].float().cpu().numpy() * 0.25))
    try:
        assert f8.V.dtype == torch.float8_e4m3fn
        f8.set_option("bf16_quant", 1)                                     # means nothing on other dtypes
        with pytest.raises(NotImplementedError):
            f8.quantize("int8")
    finally:
        f8.close()


# ------------------------------------------------------------------------------------------------
# 7. entry points
# ------------------------------------------------------------------------------------------------
def test_register_vectors_with_quantize():
    nat = _native()
    import hyperdb.ranking_algorithm as ranking
    Vb, _ = _matrix(128)
    q = _queries(1, 128, seed=21)[0]
    reg = ranking.register_vectors(Vb, quantize="int8")
    ref = ranking.register_vectors(Vb)
    try:
        reg.index.set_option("quant_min_n", 0)
        for metric in METRICS:
            gi, gs = ranking.hyperDB_ranking_algorithm_sort(reg, q.copy(), top_k=40, metric=metric)
            assert reg.index.stat("quant") == 1, metric
            ri, rs = ranking.hyperDB_ranking_algorithm_sort(ref, q.copy(), top_k=40, metric=metric)
            assert ref.index.stat("quant") == 0
            assert list(gi) == list(ri) and np.array_equal(np.asarray(gs), np.asarray(rs)), metric
    finally:
        reg.close()
        ref.close()


def test_register_vectors_two_shards_with_quantize():
    nat = _native()
    M = nat.METRIC_IDS
    import hyperdb.ranking_algorithm as ranking
    Vb, _ = _matrix(128)
    Q = _queries(3, 128, seed=22)
    grp = ranking.register_vectors(Vb, devices=[0, 0], quantize="int8")
    ref = ranking.register_vectors(Vb, devices=[0, 0])
    try:
        assert all(s.quant == nat.HDB_QUANT_I8 and s.stat("quant_bytes") > 0 for s in grp.index.shards)
        grp.index.set_option("quant_min_n", 0)
        for metric in METRICS:
            gi, gs = grp.index.topk(Q, 40, M[metric])
            assert all(s.stat("quant") == 1 for s in grp.index.shards), metric
            ri, rs = ref.index.topk(Q, 40, M[metric])
            assert all(s.stat("quant") == 0 for s in ref.index.shards)
            assert _same(gi, gs, ri, rs), metric
    finally:
        grp.close()
        ref.close()


def test_facade_bfloat16_with_quantize():
    import torch
    from hyperdb import HyperDB
    rng = np.random.default_rng(23)
    n, d = 9_001, 128
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    docs = [{"id": i, "text": f"doc {i}"} for i in range(n)]
    Q = rng.standard_normal((4, d)).astype(np.float32)
    db = HyperDB(docs, vecs, fp_precision="bfloat16", quantize="int8")
    ref = HyperDB(docs, vecs, fp_precision="bfloat16")
    try:
        assert db._index.V.dtype == torch.bfloat16 and db._index.stat("quant_bytes") == n * (d + 12)
        db._index.set_option("quant_min_n", 0)

        def both(what):
            for metric in METRICS:
                assert db.query(Q[0], top_k=20, metric=metric) == ref.query(Q[0], top_k=20, metric=metric), (what, metric)
                assert db._index.stat("quant") == 1 and ref._index.stat("quant") == 0, (what, metric)
                assert db.query_batch(Q, top_k=20, metric=metric) == ref.query_batch(Q, top_k=20, metric=metric), (what, metric)
                assert db._index.stat("quant") == 1, (what, metric)
            flt = [("skip_doc", 100)]
            assert db.query(Q[1], top_k=20, filters=flt) == ref.query(Q[1], top_k=20, filters=flt), what
            assert db._index.stat("quant") == 1, what

        both("built")
        more = rng.standard_normal((50, d)).astype(np.float32)
        more[7] = 3.0 * Q[2]
        for h in (db, ref):
            h.add([{"id": n + i, "text": f"new {i}"} for i in range(50)], more)
            h.remove_document([3, 500, 8_000])
            h.clear_cache()
        assert db._index.n == ref._index.n and db._index.stat("quant_bytes") == db._index.n * (d + 12)
        both("after add and remove_document")
        top = db.query(Q[2], top_k=3)
        assert top[0][0]["id"] == n + 7 and db._index.stat("quant") == 1
    finally:
        db._index.close()
        ref._index.close()
